"""numpy restatement of the multi-scale / flip inference operators [deeplab-semantics], twice:

float64 (`dtype=np.float64`), the mathematical truth.  The source coordinate of output index o on an axis of input extent
`n_in` and output extent `n_out` is o (n_in - 1) / (n_out - 1), held as the exact integer quotient and remainder, so
`lo` is exact and the weight is one correctly rounded quotient.

float32 (`dtype=np.float32`), the bit target of dl3_tta_resize_image / dl3_tta_accumulate: every operation a separately
rounded IEEE fp32 operation, in the order of include/dl3.h (numpy's element-wise float32 loops round each operation):
    scale = fl((n_in - 1) / (n_out - 1)), 0 where n_out == 1;  f = fl(o * scale);  lo = min(int(f), n_in - 1);
    hi = min(lo + 1, n_in - 1);  w = fl(f - lo)
    top = tl + (tr - tl) * wx;  bot = bl + (br - bl) * wx;  value = top + (bot - top) * wy

How far the float32 resize may be from the float64 one (`resize_bound`), with u = 2^-24 the fp32 unit roundoff, for a
source whose values are at most M in magnitude and whose neighbouring values (along either axis) differ by at most D:
  * coordinate.  scale carries one rounding and f = fl(o * scale) a second: |f - f_exact| <= 2 u f_exact <= 2 u (n_in - 1).
    w = fl(f - lo) is exact (lo <= f < lo + 1, Sterbenz).  The interpolant is a CONTINUOUS piecewise-linear function of the
    coordinate with slope at most D per source step — also across an integer, where the float32 side may pick the
    neighbouring cell with a weight near 0 instead of near 1, and at the clamp lo = n_in - 1 — so the value moves by at
    most 2 u (n_in - 1) D per axis: 2 u ((Hi - 1) + (Wi - 1)) D in all.
  * the three lerps.  a + (b - a) w with 0 <= w <= 1 rounds the difference (<= u D), the product (<= u D) and the sum
    (<= u M): 2 u D + u M each.  The two row lerps enter the column lerp with weights 1 - wy and wy, so together they
    count once; the column lerp adds its own: 2 (2 u D + u M).  Stated for three, as if the row errors added:
    3 (2 u D + u M).
  * the float64 side's own roundings (~1e-16 relative) and the second-order terms are covered by a factor 1 + 2^-10.
resize_bound = (1 + 2^-10) u (2 ((Hi - 1) + (Wi - 1)) D + 3 (2 D + M)).  Nothing in it comes from an output."""
import numpy as np

U32 = 2.0 ** -24


def scaled_size(n, s):
    """the pass extent: n at s == 1, else the multiple of 16 nearest to s n (halves up), at least 16"""
    if s == 1:
        return int(n)
    return max(16, 16 * int(np.floor(s * n / 16.0 + 0.5)))


def pass_list(size, scales, flip):
    out = []
    for s in scales:
        hs, ws = scaled_size(size[0], s), scaled_size(size[1], s)
        out.append((s, hs, ws, False))
        if flip:
            out.append((s, hs, ws, True))
    return out


def axis(n_in, n_out, dtype):
    """(lo, hi, w) of every output index of one axis"""
    o = np.arange(n_out, dtype=np.int64)
    if dtype == np.float32:
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        f = o.astype(np.float32) * np.float32(scale)
        lo = np.minimum(f.astype(np.int64), n_in - 1)
        w = f - lo.astype(np.float32)
        assert f.dtype == np.float32 and w.dtype == np.float32
    else:
        if n_out > 1:
            num = o * (n_in - 1)
            lo = num // (n_out - 1)
            w = (num - lo * (n_out - 1)).astype(np.float64) / np.float64(n_out - 1)
        else:
            lo, w = np.zeros(n_out, np.int64), np.zeros(n_out, np.float64)
        lo = np.minimum(lo, n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, w


def resize(src, Ho, Wo, dtype=np.float32):
    """src [B,Hi,Wi,C] -> [B,Ho,Wo,C], align_corners=True bilinear in `dtype`"""
    src = np.asarray(src).astype(dtype)
    _, Hi, Wi, _ = src.shape
    y0, y1, wy = axis(Hi, Ho, dtype)
    x0, x1, wx = axis(Wi, Wo, dtype)
    wx = wx[None, None, :, None]
    wy = wy[None, :, None, None]
    r0, r1 = src[:, y0], src[:, y1]
    tl, tr, bl, br = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    top = tl + (tr - tl) * wx
    bot = bl + (br - bl) * wx
    out = top + (bot - top) * wy
    assert out.dtype == dtype
    return out


def resize_image(src, Ho, Wo, flip=False, dtype=np.float32):
    """dl3_tta_resize_image: src [B,Hi,Wi,3] uint8 or float -> [B,Ho,Wo,3]; flip: column ox gets the value computed for
    column Wo - 1 - ox"""
    out = resize(src, Ho, Wo, dtype)
    return np.ascontiguousarray(out[:, :, ::-1]) if flip else out


def accumulate(probs, acc, Ho, Wo, flip=False, first=False, n_passes_if_last=0, dtype=np.float32):
    """dl3_tta_accumulate: probs [B,Hi,Wi,C] (a mirrored pass is read mirrored) resized to [B,Ho,Wo,C]; first: the
    result is the resized value and `acc` is not looked at, else acc + value; n_passes_if_last > 0: divided by it"""
    probs = np.asarray(probs)
    v = resize(probs[:, :, ::-1] if flip else probs, Ho, Wo, dtype)
    out = v if first else np.asarray(acc).astype(dtype).reshape(v.shape) + v
    if n_passes_if_last:
        out = out / dtype(n_passes_if_last)
    assert out.dtype == dtype
    return out


def resize_bound(Hi, Wi, M, D):
    """largest |float32 resize - float64 resize| (module docstring)"""
    return (1 + 2.0 ** -10) * U32 * (2.0 * ((Hi - 1) + (Wi - 1)) * D + 3.0 * (2.0 * D + M))


def first_argmax(p):
    return np.argmax(p, axis=-1).astype(np.int32)
