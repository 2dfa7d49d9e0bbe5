"""Multi-scale and flip inference [deeplab-semantics]: DeepLab's evaluation protocol — the class
probabilities of one image averaged over input scales and left-right flips — with every step on the device.

A pass at scale s runs a SIBLING of the model, the same graph built for the input size scaled_size(H, s) x
scaled_size(W, s), on the model's current weights:
    dl3_tta_resize_image   the batch, resized (and mirrored) straight into the sibling engine's input buffer
    the sibling's forward plan + dl3_softmax_fwd   its own output head, unchanged
    dl3_tta_accumulate     the probabilities resized back to (H, W) (un-mirrored) into one fp32 accumulator
The first pass stores, the last one divides by the pass count; dl3_argmax / crf.dense_crf_softmax read the accumulator
where a mask is wanted.  No numpy on the path: the host sees the result only.

Two deviations from tensorflow/models research/deeplab/model.py predict_labels_multi_scale, both named in DESIGN.md §12:
the pass size is a multiple of 16 instead of (H - 1) s + 1, and probabilities, not logits, are interpolated."""
import math

import numpy as np

from . import capi
from . import graph as G

DEFAULT_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
F32, U8 = 0, 1   # DL3_TTA_F32 / DL3_TTA_U8 of include/dl3.h


def scaled_size(n, s):
    """extent of the pass at scale s for a model extent n: n itself at s == 1, else the nearest multiple of 16 to s n
    (halves up), at least 16"""
    if s == 1:
        return int(n)
    return max(16, 16 * int(math.floor(s * n / 16.0 + 0.5)))


def check_scales(scales):
    try:
        out = tuple(float(s) for s in scales)
    except TypeError:
        raise ValueError("scales must be a sequence of positive numbers, got %r" % (scales,))
    if not out or any(not (s > 0 and math.isfinite(s)) for s in out):
        raise ValueError("scales must be a non-empty sequence of positive numbers, got %r" % (scales,))
    return out


def pass_list(size, scales=DEFAULT_SCALES, flip=True):
    """[(scale, hs, ws, flipped)] in execution order: the scales as given, within a scale the unflipped pass first"""
    H, W = int(size[0]), int(size[1])
    out = []
    for s in check_scales(scales):
        hs, ws = scaled_size(H, s), scaled_size(W, s)
        out.append((s, hs, ws, False))
        if flip:
            out.append((s, hs, ws, True))
    return out


def check_args(model, scales, output, crf, factory):
    """everything that can be refused before any device work; returns the pass list"""
    passes = pass_list(model.input.shape[:2], scales, True)
    if output not in ("probs", "mask"):
        raise ValueError("predict_multiscale: output must be 'probs' or 'mask', got %r" % (output,))
    if crf and output != "mask":
        raise ValueError("predict_multiscale: crf=True needs output='mask'")
    H, W = model.input.shape[:2]
    own = {(hs, ws) for _, hs, ws, _ in passes} - {(H, W)}
    if own and factory is None and getattr(model, "_tta_rebuild", None) is None:
        raise ValueError("predict_multiscale: this Model was not built by Deeplabv3() or SegModel.create_seg_model; pass "
                         "factory=callable(input_shape) -> Model to build it for another input size")
    return passes


# ---------------------------------------------------------------------------------------------- launch wrappers
def resize_image(src, dst, flip=False):
    """dl3_tta_resize_image on the current stream: src [B,Hi,Wi,3] uint8 or float32 cuda tensor -> dst float32 cuda
    tensor of B*Ho*Wo*3 elements shaped [B,Ho,Wo,3]"""
    import torch
    B, Hi, Wi, _ = src.shape
    _, Ho, Wo, _ = dst.shape
    assert src.is_contiguous() and dst.is_contiguous() and dst.dtype == torch.float32
    assert src.dtype in (torch.uint8, torch.float32) and src.shape[3] == 3 and dst.shape[3] == 3 and dst.shape[0] == B
    capi.call("dl3_tta_resize_image", src.data_ptr(), U8 if src.dtype == torch.uint8 else F32, dst.data_ptr(), B, Hi, Wi,
              Ho, Wo, int(bool(flip)), capi.stream())
    return dst


def accumulate(probs, acc, flip=False, first=False, n_passes_if_last=0):
    """dl3_tta_accumulate on the current stream: probs [B,Hi,Wi,C] -> acc [B,Ho,Wo,C], float32 cuda tensors"""
    import torch
    B, Hi, Wi, C = probs.shape
    _, Ho, Wo, _ = acc.shape
    assert probs.is_contiguous() and acc.is_contiguous() and probs.dtype == acc.dtype == torch.float32
    assert acc.shape[0] == B and acc.shape[3] == C
    capi.call("dl3_tta_accumulate", probs.data_ptr(), acc.data_ptr(), B, Hi, Wi, Ho, Wo, C, int(bool(flip)),
              int(bool(first)), int(n_passes_if_last), capi.stream())
    return acc


# ---------------------------------------------------------------------------------------------- sibling models
def build_sibling(builder, input_shape):
    """builder(input_shape) -> Model with graph's global seed stream and auto-name counters put back as they were: a later
    weights=None construction draws the weights and names it would have drawn had the sibling never been built"""
    rng, state, uids = G._rng, G._rng.bit_generator.state, dict(G._uids)
    try:
        sib = builder(tuple(input_shape))
    finally:
        G._rng = rng
        rng.bit_generator.state = state
        G._uids.clear()
        G._uids.update(uids)
    if not isinstance(sib, G.Model):
        raise ValueError("factory must return a Model, got %r" % (type(sib).__name__,))
    if tuple(sib.input.shape) != tuple(input_shape):
        raise ValueError("factory(%r) returned a model with input shape %r" % (tuple(input_shape), tuple(sib.input.shape)))
    return sib


def sibling(model, hs, ws, factory=None):
    """the model's sibling for input (hs, ws), built once and kept on the model (Model.clear_multiscale drops them)"""
    cache = model.__dict__.setdefault("_tta_siblings", {})
    key = (int(hs), int(ws))
    sib = cache.get(key)
    if sib is None:
        builder = factory if factory is not None else getattr(model, "_tta_rebuild", None)
        if builder is None:
            raise ValueError("predict_multiscale: no way to build this Model for another input size; pass factory=")
        sib = build_sibling(builder, key + (model.input.shape[2],))
        if [tuple(w.shape) for l in sib.layers for w in l.weights.values()] != \
                [tuple(w.shape) for l in model.layers for w in l.weights.values()]:
            raise ValueError("predict_multiscale: the model built for input %r does not have this model's weights" % (key,))
        cache[key] = sib
    return sib


def hand_over(src, dst):
    """the weights and moving statistics of engine `src` into engine `dst` (another input size of the same graph),
    device to device: two arena copies where both engines lay their weights out alike (always, unless `layer.trainable`
    differs between the models), else one copy per weight.  dst re-derives what it folds from them (ops_prep)."""
    a = [(k, off, n, tuple(shp)) for k, off, n, shp, _ in src.slots.values()]
    b = [(k, off, n, tuple(shp)) for k, off, n, shp, _ in dst.slots.values()]
    if a == b:
        dst.params.copy_(src.params)
        dst.state.copy_(src.state)
    else:
        if [(n, shp) for _, _, n, shp in a] != [(n, shp) for _, _, n, shp in b]:
            raise ValueError("predict_multiscale: the sibling's weights do not match the model's")
        for (ka, oa, n, _), (kb, ob, _, _) in zip(a, b):
            dst._arena(kb)[ob:ob + n].copy_(src._arena(ka)[oa:oa + n])
    dst.dirty = True


def averaged_probs(model, xb, passes, factory=None):
    """one batch through every pass: the averaged probabilities, a float32 cuda tensor [b,H,W,C] (a fresh tensor)"""
    import torch
    from .engine import pixels_to_device
    b = int(xb.shape[0])
    H, W = model.input.shape[:2]
    main = model._engine(b, False)   # brings the model's current weights to this engine's arenas
    xd = pixels_to_device(xb, main.device)
    if tuple(xd.shape) != (b, H, W, 3):
        raise ValueError("predict_multiscale: x must be [B,%d,%d,3], got %r" % (H, W, tuple(xd.shape)))
    acc, fresh = None, set()
    for i, (_, hs, ws, flipped) in enumerate(passes):
        if (hs, ws) == (H, W):
            eng = main
        else:
            eng = sibling(model, hs, ws, factory)._engine(b, False)
            if id(eng) not in fresh:   # once per call and sibling engine: the weights of THIS call
                hand_over(main, eng)
                fresh.add(id(eng))
        resize_image(xd, eng.xbuf.t.view(b, hs, ws, 3), flipped)
        probs = eng.probs_device()
        if acc is None:
            acc = torch.empty(b, H, W, probs.shape[3], dtype=torch.float32, device=main.device)
        accumulate(probs, acc, flipped, first=(i == 0), n_passes_if_last=len(passes) if i == len(passes) - 1 else 0)
    return acc


def predict_multiscale(model, x, scales=DEFAULT_SCALES, flip=True, batch_size=8, output="probs", crf=False, factory=None):
    """Model.predict_multiscale (graph.py)"""
    passes = check_args(model, scales, output, crf, factory)
    if not flip:
        passes = [p for p in passes if not p[3]]
    import torch
    from .engine import argmax_rows, pixels_to_device
    x = G.raw_pixels(x)
    H, W = model.input.shape[:2]
    if int(batch_size) <= 0:
        raise ValueError("predict_multiscale: batch_size must be positive, got %r" % (batch_size,))
    if len(x.shape) != 4 or tuple(x.shape[1:]) != (H, W, 3) or x.shape[0] == 0:
        raise ValueError("predict_multiscale: x must be [B,%d,%d,3] with B >= 1, got %r" % (H, W, tuple(x.shape)))
    outs = []
    for s in G.batches(x.shape[0], batch_size):
        xb = x[s]
        acc = averaged_probs(model, xb, passes, factory)
        b, C = acc.shape[0], acc.shape[3]
        if output == "probs":
            outs.append(acc.cpu().numpy().reshape((b,) + tuple(model.output.shape)))
        elif crf:
            from .crf import dense_crf_softmax
            outs.append(dense_crf_softmax(xb if torch.is_tensor(xb) else pixels_to_device(xb, acc.device), probs=acc)
                        .to(torch.int32).cpu().numpy())
        else:
            outs.append(argmax_rows(acc, b * H * W, C).reshape(b, H, W).cpu().numpy())
    return np.concatenate(outs, axis=0)


def clear_multiscale(model):
    """drop the sibling models and, with them, their engines' device memory"""
    sibs = model.__dict__.pop("_tta_siblings", None) or {}
    for sib in sibs.values():
        sib._engines.clear()
        sib._active = None
        sib._train_eng = None
