"""A float64 (or float32, as a yardstick) reference for ANY graph.Model — TEST INFRASTRUCTURE ONLY.

`run(model, x, labels, sw, ...)` walks model._topo through layer.inbound and evaluates every layer kind that
Engine._lo_* lowers with torch autograd on the CPU: one training step's logits, loss, {weight name: gradient} and the new
BatchNorm moving statistics.  The operator definitions are oracle/torch_ref.py's (TF SAME padding, the legacy bilinear
resize matrices, the fused-epsilon floor, the Keras weighted cross-entropy); this file adds only the graph walk, so a
graph of three layers gets the same reference as the whole network (tests/test_block_cases_host.py checks the walk on the
real Deeplabv3 graphs against oracle/dl3_oracle.py).  Tensors are NHWC between layers, like the graph's shapes."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_ref import _fused_eps, _resize_matrix, _same

# moving_variance update factor on the biased batch variance, by Engine(bn_variance=...): restated, not imported
_VAR_FACTOR = {
    "keras224": lambda n, eps: (n / (n - 1.0) if n > 1 else 1.0) * (n / (n - (1.0 + eps)) if n > 1.0 + eps else 1.0),
    "bessel": lambda n, eps: n / (n - 1.0) if n > 1 else 1.0,
    "biased": lambda n, eps: 1.0,
}


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _pads(size, k, stride, rate, padding):
    return _same(size, k, stride, rate) if padding == "same" else (0, 0)


def _conv(l, x, P):
    c = l.cfg
    k, s = c["k"], c["stride"]
    w = P[l.name + "/kernel:0"].permute(3, 2, 0, 1)   # HWIO -> OIHW
    b = P[l.name + "/bias:0"] if c["use_bias"] else None
    x = _nchw(x)
    if k > 1:
        pt, pb = _pads(x.shape[2], k, s, 1, c["padding"])
        pl, pr = _pads(x.shape[3], k, s, 1, c["padding"])
        x = F.pad(x, (pl, pr, pt, pb))
    return _nhwc(F.conv2d(x, w, b, stride=s))


def _depthwise(l, x, P):
    c = l.cfg
    s, r = c["stride"], c["rate"]
    w = P[l.name + "/depthwise_kernel:0"].permute(2, 3, 0, 1)   # (3,3,C,1) -> (C,1,3,3)
    x = _nchw(x)
    pt, pb = _pads(x.shape[2], 3, s, r, c["padding"])
    pl, pr = _pads(x.shape[3], 3, s, r, c["padding"])
    x = F.pad(x, (pl, pr, pt, pb))
    return _nhwc(F.conv2d(x, w, None, stride=s, dilation=r, groups=x.shape[1]))


def _phase_shift(y, r, co):
    """out[n, ia*r+q, ib*r+p, ch] = I[n, ia, ib, ch*r*r + p*r + q]  (the reference's own shift, not depth_to_space)"""
    N, a, b, _ = y.shape
    return y.reshape(N, a, b, co, r, r).permute(0, 1, 5, 2, 4, 3).reshape(N, a * r, b * r, co)


def _resize(x, Ho, Wo):
    Ry, Rx = _resize_matrix(Ho, x.shape[1], x.dtype), _resize_matrix(Wo, x.shape[2], x.dtype)
    cols = torch.einsum("nhwc,xw->nhxc", x, Rx)
    return torch.einsum("yh,nhxc->nyxc", Ry, cols)


def weighted_xent(probs, labels, sw):
    """Keras categorical cross-entropy on probabilities [B,HW,C] with the void column dropped from the one-hot,
    renormalise-and-clip, temporal sample weights: sum(l * w) / count(w != 0)"""
    C = probs.shape[-1]
    t = torch.as_tensor(np.asarray(labels).reshape(probs.shape[0], -1)).long()
    w = torch.as_tensor(np.asarray(sw).reshape(probs.shape[0], -1)).to(probs.dtype)
    onehot = F.one_hot(t, C + 1)[..., :C].to(probs.dtype)
    q = (probs / probs.sum(dim=-1, keepdim=True)).clamp(1e-7, 1 - 1e-7)
    ell = -(onehot * torch.log(q)).sum(dim=-1)
    return (ell * w).sum() / max(float((w != 0).sum()), 1.0)


def run(model, x, labels, sw, dtype=torch.float64, bn_mode="batch", dropout_masks=None, bn_variance="keras224",
        weights=None, keep=()):
    """one training step of `model` on raw input x [B,H,W,C], labels [B,HW] (void == classes), sample weights [B,HW].
    bn_mode: "batch" (batch statistics; the moving statistics of every layer with `trainable` set are updated) or
    "frozen" (moving statistics normalise, nothing is updated).  dropout_masks: {Dropout layer name: keep mask
    [B,H,W,C]}; a Dropout without a mask is the identity (Engine(dropout=False)).  weights: {name: array} overriding the
    layers' host copies; keep: names of layers whose outputs come back in `values`.  -> namespace(logits, loss, grads,
    new_stats, values): numpy arrays; grads holds every non-moving weight (zeros where autograd reached none), new_stats
    {BatchNorm name: (moving_mean, moving_variance)}."""
    dropout_masks = dropout_masks or {}
    P, moving = {}, {}
    for l in model.layers:
        for n, w in l.weights.items():
            w = np.asarray((weights or {}).get(n, w))
            if "/moving_" in n:
                moving[n] = torch.tensor(w, dtype=dtype)
            else:
                P[n] = torch.tensor(w, dtype=dtype).requires_grad_(True)
    val, new_stats, logits = {}, {}, None
    for l in model._topo:
        k = l.kind
        ins = [] if l is model.input.layer else [val[id(t)] for t in l.inbound]
        if k == "InputLayer":
            y = torch.tensor(np.asarray(x), dtype=dtype)
        elif k == "Prescale":
            y = ins[0] / 127.5 - 1.0
        elif k == "Reshape":
            y = ins[0].reshape((ins[0].shape[0],) + tuple(l.output.shape))
        elif k == "Activation":
            fn = l.cfg["fn"]
            if fn == "softmax":
                logits = ins[0]
                y = torch.softmax(ins[0], dim=-1)
            else:
                y = torch.relu(ins[0]) if fn == "relu" else ins[0].clamp(0.0, 6.0)
        elif k == "Add":
            y = ins[0] + ins[1]
        elif k == "Concatenate":
            y = torch.cat(ins, dim=-1)
        elif k == "ZeroPadding2D":
            (pt, pb), (pl, pr) = l.cfg["pad"]
            y = F.pad(ins[0], (0, 0, pl, pr, pt, pb))
        elif k == "Conv2D":
            y = _conv(l, ins[0], P)
        elif k == "DepthwiseConv2D":
            y = _depthwise(l, ins[0], P)
        elif k == "Subpixel":
            y = _phase_shift(_conv(l, ins[0], P), l.cfg["r"], l.cfg["out_filters"])
        elif k == "BatchNormalization":
            n, eps = l.name, l.cfg["eps"]
            g, b = P[n + "/gamma:0"], P[n + "/beta:0"]
            mm, mv = moving[n + "/moving_mean:0"], moving[n + "/moving_variance:0"]
            v = ins[0]
            if bn_mode == "batch":
                mean = v.mean(dim=(0, 1, 2))
                var = ((v - mean) ** 2).mean(dim=(0, 1, 2))    # biased
                if l.trainable:
                    rows, mo = float(v.numel() // v.shape[-1]), l.cfg["momentum"]
                    f = _VAR_FACTOR[bn_variance](rows, float(eps))
                    with torch.no_grad():
                        new_stats[n] = ((mo * mm + (1.0 - mo) * mean).numpy().copy(),
                                        (mo * mv + (1.0 - mo) * var * f).numpy().copy())
            else:
                assert bn_mode == "frozen", bn_mode
                mean, var = mm, mv
            y = (v - mean) / torch.sqrt(var + _fused_eps(eps)) * g + b
        elif k == "AveragePooling2D":
            y = ins[0].mean(dim=(1, 2), keepdim=True)
        elif k == "ResizeBilinear":
            y = _resize(ins[0], *l.cfg["size"])
        elif k == "Dropout":
            m = dropout_masks.get(l.name)
            y = ins[0] if m is None else ins[0] * torch.tensor(np.asarray(m), dtype=dtype) * (1.0 / (1.0 - l.cfg["rate"]))
        else:
            raise NotImplementedError("graph_ref: layer kind %s (%s)" % (k, l.name))
        assert tuple(y.shape[1:]) == tuple(l.output.shape), (l.name, tuple(y.shape), l.output.shape)
        val[id(l.output)] = y
    assert logits is not None and model.output.layer.cfg.get("fn") == "softmax", "the graph must end in a softmax"
    loss = weighted_xent(val[id(model.output)], labels, sw)
    loss.backward()
    grads = {n: (np.zeros(tuple(t.shape), t.detach().numpy().dtype) if t.grad is None else t.grad.numpy().copy())
             for n, t in P.items()}
    values = {l.name: val[id(l.output)].detach().numpy().copy() for l in model._topo if l.name in keep}
    return types.SimpleNamespace(logits=logits.detach().numpy().copy(), loss=float(loss.detach()), grads=grads,
                                 new_stats=new_stats, values=values)


def l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
