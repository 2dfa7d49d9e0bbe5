"""numpy restatement of sliding-window inference, twice:

float64 (`dtype=np.float64`), the mathematical truth: the weights are exact integers, the weighted sum and the weight sum
are float64 sums (53 bits: exact to ~1e-16 relative), one float64 division.

float32 (`dtype=np.float32`), the bit target of dl3_slide_accumulate / dl3_slide_finalize: every operation a separately
rounded IEEE fp32 operation in the order of include/dl3.h (numpy's element-wise float32 loops round each operation).  Per
canvas element, over the windows that cover its pixel in ascending k:
    w = fl(float(wy) * float(wx));  t = fl(w * p);  acc = fl(acc + t);  ws = fl(ws + w)
and at the end prob = fl(acc / ws).  Both start from +0.0.

The grid, per axis with image extent `size`, window `win`, stride 1 <= s <= win:
    P = max(size, win);  n = ceil((P - win) / s) + 1;  window k starts at min(k s, P - win);  k = ky * nx + kx.

How far the float32 blend may be from the float64 one (`blend_bound`), with u = 2^-24 the fp32 unit roundoff, for a pixel
covered by n windows whose probabilities are at most M (non-negative):
  * the numerator.  Term i is rounded once as a product and then takes part in at most n - 1 rounded additions (the first
    addition, 0 + t, is exact), so acc32 = sum_i w_i p_i (1 + e_i) with |e_i| <= (1 + u)^n - 1 =: g_n, and
    |acc32 - acc| <= g_n acc.
  * the denominator.  The weights are integers; their sum takes n - 1 rounded additions: |ws32 - ws| <= g_(n-1) ws (it is
    exact whenever ws < 2^24, which is every case here, but the bound does not rely on it).
  * the quotient: one more rounding, u.
  prob = acc / ws <= M, so |prob32 - prob| <= (g_n + g_(n-1) + u) M up to second-order terms: 2 n u M.  The float64 side's
  own roundings (~1e-16 relative) and the second-order terms are covered by a factor 1 + 2^-10.
blend_bound = (1 + 2^-10) 2 n u M.  Nothing in it comes from an output."""
import numpy as np

U32 = 2.0 ** -24


def _pair(v):
    return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def default_stride(window):
    return max(1, (2 * int(window[0])) // 3), max(1, (2 * int(window[1])) // 3)


def axis_origins(size, win, stride):
    P = max(size, win)
    n = -(-(P - win) // stride) + 1
    return [min(k * stride, P - win) for k in range(n)]


def grid(size, window, stride=None):
    """(ny, nx, [(y0, x0), ...]) with the windows in k order, k = ky * nx + kx"""
    H, W = _pair(window)
    sh, sw = default_stride((H, W)) if stride is None else _pair(stride)
    ys, xs = axis_origins(int(size[0]), H, sh), axis_origins(int(size[1]), W, sw)
    return len(ys), len(xs), [(y, x) for y in ys for x in xs]


def gather(x, window, stride=None, pad_value=127.5):
    """the windows of one image [Hi,Wi,3], or of every image of a batch [B,Hi,Wi,3] / a list of images one behind the other
    (image-major, then k): float32 [n,H,W,3]; rows >= Hi and columns >= Wi hold pad_value"""
    if isinstance(x, (list, tuple)) or np.ndim(x) == 4:
        return np.concatenate([gather(im, window, stride, pad_value) for im in x], axis=0)
    x = np.asarray(x)
    H, W = _pair(window)
    Hi, Wi = x.shape[:2]
    _, _, origins = grid((Hi, Wi), (H, W), stride)
    out = np.full((len(origins), H, W, 3), pad_value, np.float32)
    for k, (y0, x0) in enumerate(origins):
        crop = x[y0:y0 + H, x0:x0 + W].astype(np.float32)
        out[k, :crop.shape[0], :crop.shape[1]] = crop
    return out


def pyramid(n):
    """[min(r + 1, n - r) for r in range(n)]"""
    r = np.arange(n)
    return np.minimum(r + 1, n - r)


def weights(window, blend, dtype=np.float32):
    """[H,W] blend weights of a window"""
    H, W = _pair(window)
    if blend == "uniform":
        return np.ones((H, W), dtype)
    assert blend == "pyramid", blend
    w = pyramid(H).astype(dtype)[:, None] * pyramid(W).astype(dtype)[None, :]
    assert w.dtype == dtype
    return w


def coverage(size, window, stride=None):
    """[Hi,Wi] number of windows over each pixel"""
    H, W = _pair(window)
    n = np.zeros((int(size[0]), int(size[1])), np.int64)
    for y0, x0 in grid(size, (H, W), stride)[2]:
        n[y0:y0 + H, x0:x0 + W] += 1
    return n


def blend(probs, size, window, stride=None, blend="uniform", dtype=np.float32, parts=False):
    """probs [n,H,W,C] of one image's windows in k order -> probabilities [Hi,Wi,C] in `dtype`
    (parts=True: (acc, ws) in front of the division)"""
    probs = np.asarray(probs)
    H, W = _pair(window)
    Hi, Wi = int(size[0]), int(size[1])
    _, _, origins = grid((Hi, Wi), (H, W), stride)
    assert probs.shape[:3] == (len(origins), H, W), (probs.shape, len(origins), H, W)
    C = probs.shape[3]
    w = weights((H, W), blend, dtype)
    acc = np.zeros((Hi, Wi, C), dtype)
    ws = np.zeros((Hi, Wi), dtype)
    for k, (y0, x0) in enumerate(origins):
        h, wd = min(H, Hi - y0), min(W, Wi - x0)      # pad positions are never read
        t = w[:h, :wd, None] * probs[k, :h, :wd].astype(dtype)
        acc[y0:y0 + h, x0:x0 + wd] = acc[y0:y0 + h, x0:x0 + wd] + t
        ws[y0:y0 + h, x0:x0 + wd] = ws[y0:y0 + h, x0:x0 + wd] + w[:h, :wd]
    assert acc.dtype == dtype and ws.dtype == dtype
    if parts:
        return acc, ws
    out = acc / ws[:, :, None]
    assert out.dtype == dtype
    return out


def blend_bound(n, M=1.0):
    """largest |float32 blend - float64 blend| of a pixel under n windows (module docstring)"""
    return (1 + 2.0 ** -10) * 2.0 * n * U32 * M


def first_argmax(p):
    return np.argmax(p, axis=-1).astype(np.int32)
