"""Trimap evaluation: confusion matrices restricted to bands around the object boundaries — the trimap
experiment of the DeepLabV3+ paper — with every step on the device.

Whole-image mIoU is decided by the object interiors; the output heads and the dense CRF differ at the boundaries.  A label
map gives every pixel a *ring*: the smallest integer w such that a seed — a void pixel and / or a pixel with a 4-neighbour
of another label — lies within distance w (Chebyshev: the (2w+1)^2 square dilation of the common trimap scripts; or
Euclidean), clamped to wmax + 1.  The pixels are then counted into disjoint bins by ring, one confusion matrix per bin:
    dl3_trimap_rings       labels -> rings (uint8), two launches: row distances, then the minimum over the rows
    dl3_trimap_confusion   (prediction, label, ring) -> band[K+1][C][C] int64, accumulated across calls
`cumulative(band)` turns the bins into the matrices of the bands of width widths[k]; its last slice is the whole-image
confusion matrix.  The definitions are this package's own (the paper gives none that could be followed bit for bit).

Out of scope: distribute(), trimap inside fit's validation logs, plotting, widths above 254."""
import ctypes

import numpy as np

from . import capi

METRICS = {"chebyshev": 0, "euclidean": 1}   # DL3_TRIMAP_CHEBYSHEV / DL3_TRIMAP_EUCLIDEAN of include/dl3.h
SEEDS = {"void": 1, "edges": 2}              # DL3_TRIMAP_SEED_VOID / DL3_TRIMAP_SEED_EDGES
MAX_WIDTH, MAX_BANDS, MAX_CLASSES = 254, 8, 255
DEFAULT_WIDTHS = (1, 2, 4, 8, 16, 32)


# ---------------------------------------------------------------------------------------------- argument checks
def _as_int(v, what):
    try:
        if isinstance(v, bool) or int(v) != v:
            raise TypeError
        return int(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be an integer, got %r" % (what, v))


def check_metric(metric):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError("metric must be 'chebyshev' or 'euclidean', got %r" % (metric,))
    return METRICS[metric]


def check_seeds(seeds):
    """'void', 'edges' or a collection of them -> the seed bit mask"""
    names = (seeds,) if isinstance(seeds, str) else seeds
    try:
        names = tuple(names)
    except TypeError:
        raise ValueError("seeds must be 'void', 'edges' or a collection of them, got %r" % (seeds,))
    if not names or any(not isinstance(s, str) or s not in SEEDS for s in names):
        raise ValueError("seeds must be 'void', 'edges' or a collection of them, got %r" % (seeds,))
    bits = 0
    for s in names:
        bits |= SEEDS[s]
    return bits


def check_wmax(wmax):
    wmax = _as_int(wmax, "wmax")
    if not 1 <= wmax <= MAX_WIDTH:
        raise ValueError("wmax must be in 1..%d, got %d" % (MAX_WIDTH, wmax))
    return wmax


def check_widths(widths):
    """1 to 8 strictly increasing integer widths in 1..254 -> a tuple"""
    try:
        ws = tuple(widths)
    except TypeError:
        raise ValueError("widths must be a sequence of integers, got %r" % (widths,))
    ws = tuple(_as_int(w, "a width") for w in ws)
    if not 1 <= len(ws) <= MAX_BANDS:
        raise ValueError("widths must hold 1 to %d values, got %d" % (MAX_BANDS, len(ws)))
    if ws[0] < 1 or ws[-1] > MAX_WIDTH or any(b <= a for a, b in zip(ws, ws[1:])):
        raise ValueError("widths must be strictly increasing within 1..%d, got %r" % (MAX_WIDTH, ws))
    return ws


def check_classes(n_classes):
    C = _as_int(n_classes, "n_classes")
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("n_classes must be in 1..%d, got %d" % (MAX_CLASSES, C))
    return C


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _check_maps(a, what):
    """a host array or a tensor [B,H,W] -> (the array or tensor, (B, H, W))"""
    if not _is_tensor(a):
        a = np.asarray(a)
        if a.dtype.kind not in "biuf":
            raise ValueError("%s must be a numeric array [B,H,W], got dtype %s" % (what, a.dtype))
    shp = tuple(int(s) for s in a.shape)
    if len(shp) != 3 or min(shp) < 1:
        raise ValueError("%s must be [B,H,W] with every extent >= 1, got shape %r" % (what, shp))
    if shp[0] * shp[1] * shp[2] >= 2 ** 31:
        raise ValueError("%s: B*H*W must stay below 2^31, got %r" % (what, shp))
    return a, shp


# ---------------------------------------------------------------------------------------------- device inputs
def _device_labels(labels, C):
    """float32 [B*H*W] on the device; values outside 0..C-1 become void = C (as utils.calculate_iou does)"""
    import torch
    if _is_tensor(labels):
        t = labels.to("cuda").reshape(-1)
        return torch.where((t >= 0) & (t < C), t, torch.full_like(t, C)).to(torch.float32).contiguous()
    a = labels.reshape(-1)
    a = np.where((a >= 0) & (a < C), a, C).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _device_pred(pred):
    """int32 [B*H*W] on the device (values outside 0..C-1 are skipped by the kernel)"""
    import torch
    if _is_tensor(pred):
        return pred.to("cuda").reshape(-1).to(torch.int32).contiguous()
    a = pred.reshape(-1)
    if a.dtype.kind == "f":
        a = np.where(np.isfinite(a), a, -1)
    a = np.clip(a, -1, 2 ** 31 - 1).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---------------------------------------------------------------------------------------------- launch wrappers
def rings(labels, shape, C, wmax, metric, seeds):
    """dl3_trimap_rings on the current stream: labels, a float32 cuda tensor of B*H*W values (void = C) -> uint8 [B,H,W]"""
    import torch
    B, H, W = shape
    assert labels.dtype == torch.float32 and labels.is_contiguous() and labels.numel() == B * H * W
    out = torch.empty(B, H, W, dtype=torch.uint8, device=labels.device)
    ws = torch.empty(capi.lib().dl3_trimap_workspace_bytes(B, H, W), dtype=torch.uint8, device=labels.device)
    capi.call("dl3_trimap_rings", labels.data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, W, C, wmax, metric, seeds,
              capi.stream())
    return out


def accumulate(pred, labels, shape, C, widths, metric, seeds, band):
    """the launch pair on the current stream: pred (int32) and labels (float32, void = C), cuda tensors of B*H*W values,
    are ADDED to band, a contiguous int64 [K+1,C,C] cuda tensor.  Nothing waits for the device."""
    import torch
    B, H, W = shape
    assert pred.dtype == torch.int32 and pred.is_contiguous() and pred.numel() == B * H * W
    r = rings(labels, shape, C, widths[-1], metric, seeds)
    w = (ctypes.c_int * len(widths))(*widths)
    capi.call("dl3_trimap_confusion", pred.data_ptr(), labels.data_ptr(), r.data_ptr(), band.data_ptr(), B, H, W, C, w,
              len(widths), capi.stream())
    return band


def check_band(out, K, C):
    if out is None:
        return
    import torch
    if (not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != (K + 1, C, C) or not out.is_contiguous()
            or not out.is_cuda):
        raise ValueError("out must be a contiguous int64 [%d,%d,%d] cuda tensor" % (K + 1, C, C))


# ---------------------------------------------------------------------------------------------- the public surface
def boundary_rings(labels, n_classes, wmax, metric="chebyshev", seeds=("void", "edges")):
    """labels [B,H,W] (a host array or a device tensor; values outside 0..n_classes-1 are void) -> the ring of every
    pixel, a uint8 device tensor [B,H,W] with wmax + 1 = "beyond".  Argument errors are ValueErrors raised before any
    device work."""
    C, wmax, m, s = check_classes(n_classes), check_wmax(wmax), check_metric(metric), check_seeds(seeds)
    labels, shape = _check_maps(labels, "labels")
    return rings(_device_labels(labels, C), shape, C, wmax, m, s)


def band_confusion(pred, labels, n_classes, widths=DEFAULT_WIDTHS, metric="chebyshev", seeds=("void", "edges"), out=None):
    """pred and labels [B,H,W] (host arrays or device tensors) -> the disjoint banded confusion matrices, an int64 device
    tensor [K+1,C,C]: bin k holds the pixels whose ring is above widths[k-1] and at most widths[k], bin K the rest.  out:
    a contiguous int64 [K+1,C,C] cuda tensor the counts are ADDED to (the caller zeroed it).  Argument errors are
    ValueErrors raised before any device work."""
    C, ws, m, s = check_classes(n_classes), check_widths(widths), check_metric(metric), check_seeds(seeds)
    labels, shape = _check_maps(labels, "labels")
    pred, pshape = _check_maps(pred, "pred")
    if pshape != shape:
        raise ValueError("pred and labels must have one shape, got %r and %r" % (pshape, shape))
    check_band(out, len(ws), C)
    import torch
    if out is None:
        out = torch.zeros(len(ws) + 1, C, C, dtype=torch.int64, device="cuda")
    return accumulate(_device_pred(pred), _device_labels(labels, C), shape, C, ws, m, s, out)


def cumulative(band):
    """disjoint bins [K+1,C,C] -> their running sum over k: slice k is the confusion matrix of the band of width
    widths[k], the last slice the whole-image matrix.  A tensor stays a tensor, anything else becomes a numpy array."""
    if _is_tensor(band):
        if band.dim() != 3:
            raise ValueError("band must be [K+1,C,C], got shape %r" % (tuple(band.shape),))
        return band.cumsum(0)
    band = np.asarray(band)
    if band.ndim != 3:
        raise ValueError("band must be [K+1,C,C], got shape %r" % (band.shape,))
    return np.cumsum(band, axis=0, dtype=np.int64)
