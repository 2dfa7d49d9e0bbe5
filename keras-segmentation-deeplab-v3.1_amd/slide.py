"""Sliding-window inference: masks and probabilities for images of ANY size, at their own resolution —
mmseg's `slide` mode, DeepLab's Cityscapes crop evaluation — with every step on the device.

An image is cut into overlapping windows of the model's input size (the last window of an axis is shifted back to end on
the image's edge), the network runs on every window, the class probabilities are averaged where windows overlap
(blend="uniform") or averaged with weights that fall off towards a window's border (blend="pyramid"), and the arg-max is
taken at the image's resolution:
    dl3_slide_gather       the windows of a chunk straight into the engine's input buffer, one launch per image
    the forward plan + dl3_softmax_fwd   the model's own output head, unchanged
    dl3_slide_accumulate   the chunk's probabilities into each image's fp32 canvas, one launch per image
    dl3_slide_finalize     canvas / weight sum -> probabilities or the first-maximum mask, once per image
The windows of a call form one list, image-major, then k, cut into forward batches exactly as predict() cuts its images:
chunks span image boundaries, so many small images still fill the batch.  An image is uploaded once in its own dtype when
its first window is scheduled; its canvas lives from then until its last window has been accumulated.  No numpy on the
path: only masks or final probabilities cross PCIe.  Probabilities, not logits, are averaged (Deviation 2 of §12).

Out of scope: combining with predict_multiscale, crf=, training, reading image files."""
import numpy as np

from . import capi

F32, U8 = 0, 1            # DL3_TTA_F32 / DL3_TTA_U8 of include/dl3.h
BLENDS = {"uniform": 0, "pyramid": 1}   # DL3_SLIDE_UNIFORM / DL3_SLIDE_PYRAMID


def default_stride(window):
    """two thirds of the window per axis, at least 1"""
    return max(1, (2 * int(window[0])) // 3), max(1, (2 * int(window[1])) // 3)


def check_stride(stride, window):
    H, W = int(window[0]), int(window[1])
    if stride is None:
        return default_stride((H, W))
    try:
        if np.ndim(stride) == 0:
            sh = sw = stride
        else:
            sh, sw = stride
        if int(sh) != sh or int(sw) != sw:
            raise TypeError
        sh, sw = int(sh), int(sw)
    except (TypeError, ValueError):
        raise ValueError("stride must be an integer or a pair of integers, got %r" % (stride,))
    if not (1 <= sh <= H and 1 <= sw <= W):
        raise ValueError("stride must be in [1, window] per axis, got %r for window %r" % ((sh, sw), (H, W)))
    return sh, sw


def _origins(size, win, stride):
    P = max(size, win)
    n = -(-(P - win) // stride) + 1
    return [min(k * stride, P - win) for k in range(n)]


def grid(size, window, stride=None):
    """(ny, nx, [(y0, x0), ...]): the windows of an image of `size` in k order, k = ky * nx + kx"""
    Hi, Wi = int(size[0]), int(size[1])
    if Hi < 1 or Wi < 1:
        raise ValueError("size must be positive, got %r" % (size,))
    H, W = int(window[0]), int(window[1])
    sh, sw = check_stride(stride, (H, W))
    ys, xs = _origins(Hi, H, sh), _origins(Wi, W, sw)
    return len(ys), len(xs), [(y, x) for y in ys for x in xs]


def pyramid_weights(n):
    """the pyramid blend's weights along an axis of extent n: min(r + 1, n - r)"""
    return [min(r + 1, n - r) for r in range(n)]


# ---------------------------------------------------------------------------------------------- argument checks
def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _check_image(a, rank, what):
    """one image, or a batch of equally sized ones: a uint8 / float32 array or tensor; other host dtypes become float32"""
    if not _is_tensor(a):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
    else:
        import torch
        if a.dtype not in (torch.uint8, torch.float32):
            a = a.to(torch.float32)
    shp = tuple(a.shape)
    if len(shp) != rank or shp[-1] != 3 or min(shp) < 1:
        raise ValueError("predict_sliding: x must be %s with every extent >= 1, got shape %r" % (what, shp))
    return a


def check_args(model, x, stride, blend, batch_size, output):
    """everything that can be refused before any device work -> (images [(array or tensor [Hi,Wi,3])...], stacked, stride)"""
    H, W = model.input.shape[:2]
    stride = check_stride(stride, (H, W))
    if blend not in BLENDS:
        raise ValueError("predict_sliding: blend must be 'uniform' or 'pyramid', got %r" % (blend,))
    if output not in ("mask", "probs"):
        raise ValueError("predict_sliding: output must be 'mask' or 'probs', got %r" % (output,))
    try:
        ok = int(batch_size) == batch_size and int(batch_size) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("predict_sliding: batch_size must be a positive integer, got %r" % (batch_size,))
    if isinstance(x, (list, tuple)):
        if len(x) == 0:
            raise ValueError("predict_sliding: x must hold at least one image")
        return [_check_image(im, 3, "a list of [Hi,Wi,3] images") for im in x], False, stride
    x = _check_image(x, 4, "[B,Hi,Wi,3]")
    return [x[i] for i in range(x.shape[0])], True, stride


# ---------------------------------------------------------------------------------------------- launch wrappers
def gather(img, window, stride, k0, nw, dst, pad_value=127.5):
    """dl3_slide_gather on the current stream: img [Hi,Wi,3] uint8 / float32 cuda tensor -> dst, nw * H * W * 3 floats"""
    import torch
    Hi, Wi, _ = img.shape
    assert img.is_contiguous() and dst.is_contiguous() and dst.dtype == torch.float32
    assert img.dtype in (torch.uint8, torch.float32) and dst.numel() == nw * window[0] * window[1] * 3
    capi.call("dl3_slide_gather", img.data_ptr(), U8 if img.dtype == torch.uint8 else F32, Hi, Wi, window[0], window[1],
              stride[0], stride[1], int(k0), int(nw), float(pad_value), dst.data_ptr(), capi.stream())
    return dst


def accumulate(probs, acc, window, stride, k0, blend):
    """dl3_slide_accumulate on the current stream: probs [nw,H,W,C] -> the canvas acc [Hi,Wi,C], float32 cuda tensors"""
    nw, H, W, C = probs.shape
    Hi, Wi, _ = acc.shape
    assert probs.is_contiguous() and acc.is_contiguous() and (H, W) == tuple(window) and acc.shape[2] == C
    capi.call("dl3_slide_accumulate", probs.data_ptr(), acc.data_ptr(), None, Hi, Wi, H, W, C, stride[0], stride[1], int(k0),
              int(nw), BLENDS[blend], capi.stream())
    return acc


def finalize(acc, window, stride, blend, output):
    """dl3_slide_finalize on the current stream: the canvas in place -> probabilities [Hi,Wi,C], or an int32 mask [Hi,Wi]"""
    import torch
    Hi, Wi, C = acc.shape
    mask = torch.empty(Hi, Wi, dtype=torch.int32, device=acc.device) if output == "mask" else None
    capi.call("dl3_slide_finalize", acc.data_ptr(), None, None if output == "mask" else acc.data_ptr(),
              None if mask is None else mask.data_ptr(), Hi, Wi, window[0], window[1], C, stride[0], stride[1], BLENDS[blend],
              capi.stream())
    return acc if mask is None else mask


# ---------------------------------------------------------------------------------------------- the call
def window_list(sizes, window, stride):
    """[(image, k)] of a call: image-major, then k"""
    out = []
    for i, size in enumerate(sizes):
        ny, nx, _ = grid(size, window, stride)
        out.extend((i, k) for k in range(ny * nx))
    return out


def chunks(windows, batch_size):
    """the window list cut as predict() cuts its batches: min(batch_size, n) consecutive windows, a short last chunk"""
    bs = min(int(batch_size), len(windows))
    return [windows[i:i + bs] for i in range(0, len(windows), bs)]


def _runs(chunk):
    """[(image, first k, count, offset in the chunk)] of a chunk's consecutive windows per image"""
    runs = []
    for j, (i, k) in enumerate(chunk):
        if runs and runs[-1][0] == i:
            runs[-1][2] += 1
        else:
            runs.append([i, k, 1, j])
    return runs


def predict_sliding(model, x, stride=None, blend="uniform", batch_size=8, output="mask", pad_value=127.5):
    """Model.predict_sliding (graph.py)"""
    images, stacked, stride = check_args(model, x, stride, blend, batch_size, output)
    import torch
    from .engine import pixels_to_device
    H, W = model.input.shape[:2]
    window = (H, W)
    sizes = [tuple(int(s) for s in im.shape[:2]) for im in images]
    windows = window_list(sizes, window, stride)
    last_k = {}
    for i, k in windows:
        last_k[i] = k
    live = {}                       # image -> (device image, canvas) while its windows are in flight
    outs = [None] * len(images)
    for chunk in chunks(windows, batch_size):
        b = len(chunk)
        eng = model._engine(b, False)       # brings the model's current weights to this engine's arenas
        v = eng.logits_view
        if (v.buf.H, v.buf.W) != (H, W):
            raise ValueError("predict_sliding: the model's output is %dx%d, not its input size %dx%d" % (v.buf.H, v.buf.W, H, W))
        runs = _runs(chunk)
        xb = eng.xbuf.t
        for i, k0, nw, off in runs:
            if i not in live:
                live[i] = (pixels_to_device(images[i], eng.device),
                           torch.zeros(sizes[i] + (v.C,), dtype=torch.float32, device=eng.device))
            gather(live[i][0], window, stride, k0, nw, xb[off * H * W * 3:(off + nw) * H * W * 3], pad_value)
        probs = eng.probs_device()
        for i, k0, nw, off in runs:
            accumulate(probs[off:off + nw], live[i][1], window, stride, k0, blend)
            if k0 + nw - 1 == last_k[i]:
                _, acc = live.pop(i)
                outs[i] = finalize(acc, window, stride, blend, output).cpu().numpy()
    return np.stack(outs, axis=0) if stacked else outs
