"""Dense-CRF post-processing on the device: the exact mean-field inference of the model the reference's do_crf
configures in pydensecrf (utils.py:74-91) — unary energies from the labels, a Gaussian position kernel, a bilateral
position + colour kernel, symmetric normalisation, Potts compatibility, parallel updates — summed over ALL pixel pairs by
dl3_crf_inference (csrc/crf.hip) instead of pydensecrf's permutohedral lattice [pydensecrf-semantics].
Results agree with pydensecrf only as far as its lattice approximates these sums.

The label unary energies are built on the host in numpy (O(N L)); every parameter comes from utils.CRF_PARAMS.

dense_crf_softmax takes the network's own class scores instead of a label mask: the unary energies are
unary_from_softmax of the probabilities, formed on the device (dl3_crf_unary_*, csrc/crfunary.hip) with one label per
class, so the MAP index IS the class id — no np.unique, no host unary, no padding energy, no restore table.
"""
import numpy as np

from . import capi

MAX_LABELS = 32
PAD_ENERGY = 1e30  # unary of the labels an image of a batch does not have: exp(-1e30 - max) == 0 exactly


def unary_from_labels(labels, n_labels, gt_prob, zero_unsure=True):
    """pydensecrf.utils.unary_from_labels [pydensecrf-semantics]: float32 [n_labels, N].  The given label of a pixel costs
    -log(gt_prob), every other one -log((1 - gt_prob) / (n_labels - 1)).  With zero_unsure label 0 means "no label"
    (all energies -log(1 / n_labels)) and label k >= 1 owns row k - 1; row n_labels - 1 is then written only through the
    negative index of label 0 and overwritten by the unsure value."""
    labels = np.asarray(labels).reshape(-1)
    n_energy = -np.log((1.0 - gt_prob) / (n_labels - 1))
    p_energy = -np.log(gt_prob)
    U = np.full((n_labels, labels.size), n_energy, dtype="float32")
    U[labels - 1 if zero_unsure else labels, np.arange(U.shape[1])] = p_energy
    if zero_unsure:
        U[:, labels == 0] = -np.log(1.0 / n_labels)
    return U


def kernel_params():
    """{sx, sy, w_gauss, sxy, srgb, w_bilateral} of dl3_crf_inference from utils.CRF_PARAMS"""
    from .utils import CRF_PARAMS as P
    sx, sy = P["gaussian_sxy"]
    return np.array([sx, sy, P["gaussian_compat"], P["bilateral_sxy"], P["bilateral_srgb"], P["bilateral_compat"]],
                    np.float32)


def inference(images, U, iters, want_q=False, want_energy=False):
    """dl3_crf_inference on the current stream: images uint8 cuda [B,H,W,3], U float32 cuda [B,L,N] ->
    (map int32 [B,N], Q or None, energy or None), device tensors"""
    import torch
    B, H, W = images.shape[:3]
    L = U.shape[1]
    dev = images.device
    ws = torch.empty(int(capi.lib().dl3_crf_workspace_bytes(B, H, W, L)) or 16, dtype=torch.uint8, device=dev)
    par = torch.from_numpy(kernel_params())  # read by the host side of the launch
    MAP = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    Q = torch.empty(B, L, H * W, dtype=torch.float32, device=dev) if want_q else None
    E = torch.empty(B, L, H * W, dtype=torch.float32, device=dev) if want_energy else None
    capi.call("dl3_crf_inference", images.data_ptr(), U.data_ptr(), B, H, W, L, par.data_ptr(), int(iters),
              Q.data_ptr() if want_q else None, E.data_ptr() if want_energy else None, MAP.data_ptr(), ws.data_ptr(),
              ws.numel(), torch.cuda.current_stream().cuda_stream)
    return MAP, Q, E


def dense_crf(images, masks, zero_unsure=True, return_q=False):
    """do_crf for a batch of images of one size.  images [B,H,W,3] (cast to uint8 as the reference does), masks [B,H,W]
    integer; numpy arrays or cuda tensors.  Per image: colors, labels = np.unique(mask) as in do_crf, the unary energies
    padded to the batch's largest label count with a large finite energy (those labels keep probability exactly 0, so an
    image's result does not depend on its batch), one dl3_crf_inference launch sequence for the batch, and the
    reference's label restore (utils.restore_crf_labels, quirk included).

    Returns int64 masks [B,H,W] — a cuda tensor when `masks` is one (the pixels never visit the host; only the small
    integer masks do, for np.unique and the unary), else a numpy array — and with return_q also Q [B,L,H*W] (rows of the
    padding labels are 0).  An image whose mask has a single value comes back unchanged (the unary divides by
    n_labels - 1; pydensecrf does not define that case)."""
    import torch
    from .utils import CRF_PARAMS, restore_crf_labels
    if not torch.cuda.is_available():
        raise capi.DL3Error("the device dense-CRF needs a GPU (HIP device); there is no CPU fallback")
    on_device = torch.is_tensor(masks)
    mh = masks.detach().cpu().numpy() if on_device else np.asarray(masks)
    if mh.ndim != 3:
        raise ValueError("masks must be [B,H,W], got shape %r" % (mh.shape,))
    B, H, W = mh.shape
    if tuple(images.shape) != (B, H, W, 3):
        raise ValueError("images must be [B,H,W,3] matching the masks, got %r for masks %r" % (tuple(images.shape), mh.shape))
    dev = masks.device if on_device else torch.device("cuda", torch.cuda.current_device())
    im = images_u8(images, dev)
    uniq = [np.unique(mh[b], return_inverse=True) for b in range(B)]
    L = max(len(c) for c, _ in uniq)
    if L > MAX_LABELS:
        raise capi.DL3Error("dense_crf: a mask with %d distinct values; the device kernels take at most %d labels"
                            % (L, MAX_LABELS))
    out = torch.from_numpy(mh.astype(np.int64)).to(dev) if not on_device else masks.to(torch.int64).clone()
    Qout = torch.zeros(B, L, H * W, dtype=torch.float32, device=dev) if return_q else None
    live = [b for b in range(B) if len(uniq[b][0]) > 1]
    if live:
        U = np.full((len(live), L, H * W), PAD_ENERGY, np.float32)
        for n, b in enumerate(live):
            colors, labels = uniq[b]
            U[n, :len(colors)] = unary_from_labels(labels.reshape(-1), len(colors), CRF_PARAMS["gt_prob"], zero_unsure)
        idx = torch.tensor(live, device=dev)
        MAP, Q, _ = inference(im[idx] if len(live) < B else im, torch.from_numpy(U).to(dev), CRF_PARAMS["iterations"],
                              want_q=return_q)
        MAP = MAP.to(torch.int64)
        for n, b in enumerate(live):
            # restore_crf_labels acts on values: run the reference's loop on the indices present and apply it as a table
            present = torch.unique(MAP[n]).cpu().numpy()
            table = np.arange(L, dtype=np.int64)
            table[present] = restore_crf_labels(present.copy(), uniq[b][0])
            out[b] = torch.from_numpy(table).to(dev)[MAP[n]].reshape(H, W)
            if return_q:
                Qout[b] = Q[n]
    if not on_device:
        out = out.cpu().numpy()
        Qout = Qout.cpu().numpy() if return_q else None
    return (out, Qout) if return_q else out


def unary_from_softmax(sm, scale=None, clip=1e-5):
    """pydensecrf.utils.unary_from_softmax [pydensecrf-semantics]: probabilities [C, ...] -> float32 [C, N] energies
    -log(p).  With `scale` the probabilities are mixed with the uniform distribution first, p = scale * p +
    (1 - scale) / C (how much the scores are trusted); with `clip` they are then clipped to [clip, 1], which bounds the
    energy of a class the network rules out.  The host twin of dl3_crf_unary_*."""
    sm = np.asarray(sm)
    C = sm.shape[0]
    if scale is not None:
        sm = scale * sm + (1.0 - scale) / C
    if clip is not None:
        sm = np.clip(sm, clip, 1.0)
    with np.errstate(divide="ignore"):
        return (-np.log(sm)).reshape(C, -1).astype(np.float32)


def _none_as_zero(v):
    """scale / clip of the C ABI: a value <= 0 stands for None"""
    return 0.0 if v is None else float(v)


def images_u8(images, dev):
    """the CRF's image operand: uint8 [B,H,W,3] on `dev`, cast as dense_crf casts it"""
    import torch
    if torch.is_tensor(images):
        return images.to(dev).to(torch.uint8).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(images).astype("uint8"))).to(dev)


def unary_plain(x, is_prob, scale=None, clip=1e-5):
    """dl3_crf_unary_plain on the current stream: x float32 cuda [B,N,C] (logits, or probabilities with is_prob) ->
    U float32 cuda [B,C,N]"""
    import torch
    B, N, C = x.shape
    U = torch.empty(B, C, N, dtype=torch.float32, device=x.device)
    capi.call("dl3_crf_unary_plain", x.data_ptr(), int(bool(is_prob)), U.data_ptr(), B, N, C, _none_as_zero(scale),
              _none_as_zero(clip), torch.cuda.current_stream().cuda_stream)
    return U


def dense_crf_softmax(images, probs=None, logits=None, scale=None, clip=1e-5, return_q=False):
    """The dense CRF on the network's class scores, for a batch of images of one size: images [B,H,W,3] (cast to uint8),
    and exactly one of `probs` (what Model.predict returns) / `logits`, [B,H,W,C] or [B,H*W,C]; numpy arrays or cuda
    tensors.  One dl3_crf_unary_plain launch (unary_from_softmax with `scale` / `clip`) and one dl3_crf_inference launch
    sequence with L = C labels and utils.CRF_PARAMS.

    Returns the MAP class ids, int64 [B,H,W] — a cuda tensor when the scores are one, else a numpy array — and with
    return_q also Q [B,C,H*W].  C > 32 raises capi.DL3Error; with a single class every pixel is class 0."""
    import torch
    from .utils import CRF_PARAMS
    if (probs is None) == (logits is None):
        raise ValueError("dense_crf_softmax takes exactly one of probs= and logits=")
    x = logits if probs is None else probs
    if not torch.cuda.is_available():
        raise capi.DL3Error("the device dense-CRF needs a GPU (HIP device); there is no CPU fallback")
    if len(images.shape) != 4 or images.shape[3] != 3:
        raise ValueError("images must be [B,H,W,3], got shape %r" % (tuple(images.shape),))
    B, H, W = (int(n) for n in images.shape[:3])
    on_device = torch.is_tensor(x)
    if tuple(x.shape[:-1]) not in ((B, H, W), (B, H * W)):
        raise ValueError("scores must be [B,H,W,C] or [B,H*W,C] matching images %r, got %r"
                         % (tuple(images.shape), tuple(x.shape)))
    C = int(x.shape[-1])
    if C > MAX_LABELS:
        raise capi.DL3Error("dense_crf_softmax: %d classes; the device kernels take at most %d labels" % (C, MAX_LABELS))
    dev = x.device if on_device else torch.device("cuda", torch.cuda.current_device())
    if on_device:
        xd = x.to(torch.float32).reshape(B, H * W, C).contiguous()
    else:
        xd = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(B, H * W, C))).to(dev)
    im = images_u8(images, dev)
    if C == 1:
        out = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
        Q = torch.ones(B, 1, H * W, dtype=torch.float32, device=dev) if return_q else None
    else:
        U = unary_plain(xd, probs is not None, scale, clip)
        MAP, Q, _ = inference(im, U, CRF_PARAMS["iterations"], want_q=return_q)
        out = MAP.to(torch.int64).reshape(B, H, W)
    if not on_device:
        out = out.cpu().numpy()
        Q = Q.cpu().numpy() if return_q else None
    return (out, Q) if return_q else out
