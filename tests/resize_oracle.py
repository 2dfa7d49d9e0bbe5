"""numpy restatement of cv2.resize for 8-bit images — INTER_LINEAR (the portable C++ path: float32 source coordinates,
11-bit coefficients, the two-pass integer rounding) and INTER_NEAREST — [cv2-semantics], written one destination
coordinate and one pixel at a time in plain Python loops.  It is the oracle the device front end (csrc/cvresize.hip,
dl3_cv_resize) is pinned against bit for bit; it shares no code with the package's augment.py."""
import math

import numpy as np

from tests import aug_oracle

COEF = 2048


def scale_of(src, dst):
    """cv2: scale = 1 / (dst / src) in double — the reciprocal of the quotient, not src / dst"""
    return 1.0 / (float(dst) / float(src))


def linear_coord(d, src, dst):
    """(s, f) of destination coordinate d before any border rule: f float32"""
    f = np.float32((d + 0.5) * scale_of(src, dst) - 0.5)
    s = int(math.floor(f))
    return s, np.float32(f - np.float32(s))


def coefs(f):
    """(c0, c1): rint of the float32 products, half to even"""
    c0 = int(np.rint(np.float32(np.float32(1.0) - f) * np.float32(COEF)))
    c1 = int(np.rint(np.float32(f) * np.float32(COEF)))
    return c0, c1


def column_taps(d, src, dst):
    """(first column, second column, a0, a1) of destination column d"""
    s, f = linear_coord(d, src, dst)
    if s < 0:
        s, f = 0, np.float32(0)
    if s >= src - 1:
        s, f = src - 1, np.float32(0)
    return (s, min(s + 1, src - 1)) + coefs(f)


def row_taps(d, src, dst):
    """(first row, second row, b0, b1) of destination row d: the fraction is kept, the rows are clipped"""
    s, f = linear_coord(d, src, dst)
    clip = lambda v: min(max(v, 0), src - 1)
    return (clip(s), clip(s + 1)) + coefs(f)


def nearest_index(d, src, dst):
    return min(int(math.floor(d * scale_of(src, dst))), src - 1)


def resize_linear(img, dst_hw):
    """cv2.resize(img, (w, h)) of a uint8 image [Hs,Ws] or [Hs,Ws,C]"""
    squeeze = img.ndim == 2
    p = (img[..., None] if squeeze else img).astype(np.int64)
    Hs, Ws, C = p.shape
    H, W = dst_hw
    if (H, W) == (Hs, Ws):
        return img.copy()
    cols = [column_taps(x, Ws, W) for x in range(W)]
    rows = [row_taps(y, Hs, H) for y in range(H)]
    out = np.zeros((H, W, C), np.uint8)
    for y, (y0, y1, b0, b1) in enumerate(rows):
        for x, (x0, x1, a0, a1) in enumerate(cols):
            for c in range(C):
                S0 = int(p[y0, x0, c]) * a0 + int(p[y0, x1, c]) * a1
                S1 = int(p[y1, x0, c]) * a0 + int(p[y1, x1, c]) * a1
                v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
                out[y, x, c] = v & 255   # what a store into uint8 keeps; the host tests show it never exceeds 255
    return out[..., 0] if squeeze else out


def resize_linear_wide(img, dst_hw):
    """the same result before the uint8 store (int64), for the range check of the host tests"""
    p = img.astype(np.int64)
    Hs, Ws = p.shape
    H, W = dst_hw
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        y0, y1, b0, b1 = row_taps(y, Hs, H)
        for x in range(W):
            x0, x1, a0, a1 = column_taps(x, Ws, W)
            S0 = int(p[y0, x0]) * a0 + int(p[y0, x1]) * a1
            S1 = int(p[y1, x0]) * a0 + int(p[y1, x1]) * a1
            out[y, x] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    return out


def resize_nearest(lab, dst_hw):
    """cv2.resize(lab, (w, h), interpolation=cv2.INTER_NEAREST) of an integer map [Hs,Ws]"""
    Hs, Ws = lab.shape
    H, W = dst_hw
    out = np.zeros((H, W), lab.dtype)
    for y in range(H):
        sy = nearest_index(y, Hs, H)
        for x in range(W):
            out[y, x] = lab[sy, nearest_index(x, Ws, W)]
    return out


def tables(src_hw, dst_hw):
    """the per-axis tables in the layout of include/dl3.h (dl3_cv_resize): xs, xa0, xa1, xn [W], ys, yb0, yb1, yn [H];
    ys is the row floor() gave, unclipped"""
    (Hs, Ws), (H, W) = src_hw, dst_hw
    cols = [column_taps(x, Ws, W) for x in range(W)]
    rows = [(linear_coord(y, Hs, H)[0],) + row_taps(y, Hs, H)[2:] for y in range(H)]
    return np.array([c[0] for c in cols] + [c[2] for c in cols] + [c[3] for c in cols] +
                    [nearest_index(x, Ws, W) for x in range(W)] + [r[0] for r in rows] + [r[1] for r in rows] +
                    [r[2] for r in rows] + [nearest_index(y, Hs, H) for y in range(H)], np.int32)


def present_bits(lab):
    """[8] int32: bit v set when value v (0..255) occurs in the map — np.unique(label), utils.py:317"""
    out = np.zeros(8, np.uint32)
    for v in np.unique(lab):
        if 0 <= int(v) < 256:
            out[int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    return out.view(np.int32)


def front_image(image, label, dst_hw, blur, crop):
    """one image through utils.py:319-327: [blur 5x5] -> resize to dst_hw (crop None) or the dst_hw crop at crop =
    (x, y); -> (image uint8 [H,W,3], label [H,W])"""
    H, W = dst_hw
    if blur:
        image = aug_oracle.gaussian_blur5(image)
    if crop is not None:
        x, y = crop
        return np.ascontiguousarray(image[y:y + H, x:x + W]), np.ascontiguousarray(label[y:y + H, x:x + W])
    return resize_linear(image, dst_hw), resize_nearest(label, dst_hw)


def front_batch(images, labels, dst_hw, blur, crops):
    res = [front_image(i, l, dst_hw, b, c) for i, l, b, c in zip(images, labels, blur, crops)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def chain_image(image, label, source_label, p, warp, histeq, n_classes):
    """the rest of utils.py:329-365 behind the front end, from aug_oracle's pieces: flips, gamma LUT, warpAffine, CLAHE,
    and the void relabel against np.unique of the SOURCE-size map (utils.py:317 runs before the resize) — which
    aug_oracle.augment_image, fed the resized map, would take from the resized one"""
    labels = np.unique(source_label)
    if p.hflip:
        image, label = image[:, ::-1], label[:, ::-1]
    if p.vflip:
        image, label = image[::-1], label[::-1]
    if p.gamma is not None:
        image = aug_oracle.gamma_lut(p.gamma)[image]
    if warp:
        image = aug_oracle.warp_affine(image, p.angle, p.scale)
        label = aug_oracle.warp_affine(label, p.angle, p.scale)
    if histeq:
        yuv = aug_oracle.bgr2yuv(image)
        yuv[..., 0] = aug_oracle.clahe(yuv[..., 0])
        image = aug_oracle.yuv2bgr(yuv)
    out = label.astype(np.int32)
    for j in np.setxor1d(np.unique(out), labels):
        out[out == j] = n_classes
    return np.ascontiguousarray(image), out.astype(label.dtype)


def float_bilinear(img, dst_hw):
    """half-pixel bilinear with edge clamp in float64: the yardstick the integer path is held against"""
    Hs, Ws = img.shape
    H, W = dst_hw
    p = img.astype(np.float64)
    out = np.zeros((H, W))
    for y in range(H):
        fy = (y + 0.5) * Hs / H - 0.5
        y0 = math.floor(fy)
        wy = fy - y0
        ya, yb = min(max(y0, 0), Hs - 1), min(max(y0 + 1, 0), Hs - 1)
        for x in range(W):
            fx = (x + 0.5) * Ws / W - 0.5
            x0 = math.floor(fx)
            wx = fx - x0
            xa, xb = min(max(x0, 0), Ws - 1), min(max(x0 + 1, 0), Ws - 1)
            out[y, x] = ((p[ya, xa] * (1 - wx) + p[ya, xb] * wx) * (1 - wy) +
                         (p[yb, xa] * (1 - wx) + p[yb, xb] * wx) * wy)
    return out
