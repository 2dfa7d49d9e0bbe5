"""numpy restatement of the training augmentation of the reference's SegmentationGenerator.__getitem__
(utils.py:310-369) with cv2's integer semantics [cv2-semantics]: the oracle the device kernels
(csrc/augment.hip) are pinned against bit for bit.  It takes the per-image parameters (augment.ImageParams) and derives
every table itself, one image at a time, in plain loops over whole arrays — no code is shared with augment.py's tables."""
import math

import numpy as np


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def gaussian_blur5(img):
    """cv2.GaussianBlur(img, (5, 5), 0) on uint8 [H,W,C]: [1,4,6,4,1]/16 both ways, (sum + 128) >> 8, reflect-101"""
    H, W = img.shape[:2]
    k = np.array([1, 4, 6, 4, 1], np.int64)
    p = img.astype(np.int64)
    rows = reflect101(np.arange(-2, H + 2), H)
    cols = reflect101(np.arange(-2, W + 2), W)
    q = p[rows][:, cols]
    acc = np.zeros(img.shape, np.int64)
    for i in range(5):
        for j in range(5):
            acc += k[i] * k[j] * q[i:i + H, j:j + W]
    return ((acc + 128) >> 8).astype(np.uint8)


def gamma_lut(factor):
    with np.errstate(all="ignore"):
        return np.array([((i / 255.0) ** factor) * 255 for i in np.arange(0, 256)]).astype(np.uint8)


def inverse_rotation(H, W, angle, scale):
    """getRotationMatrix2D((W//2, H//2), angle, scale) inverted as invertAffineTransform does"""
    a = angle * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = W // 2, H // 2
    M = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    return np.array([[A11, A12, -A11 * M[2] - A12 * M[5]], [A21, A22, -A21 * M[2] - A22 * M[5]]])


def warp_coords(H, W, angle, scale):
    """source coordinates of every output pixel in 1/32 pixels (int64 [H,W] each), cv2's fixed-point rounding"""
    A = inverse_rotation(H, W, angle, scale)
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    adelta, bdelta = np.rint(A[0, 0] * x * 1024), np.rint(A[1, 0] * x * 1024)
    X0 = np.rint((A[0, 1] * y + A[0, 2]) * 1024) + 16
    Y0 = np.rint((A[1, 1] * y + A[1, 2]) * 1024) + 16
    X = (X0[:, None].astype(np.int64) + adelta[None, :].astype(np.int64)) >> 5
    Y = (Y0[:, None].astype(np.int64) + bdelta[None, :].astype(np.int64)) >> 5
    return X, Y


def warp_affine(img, angle, scale):
    """cv2.warpAffine(img, getRotationMatrix2D((W//2, H//2), angle, scale), (W, H)), INTER_LINEAR, constant-0 border,
    uint8 [H,W] or [H,W,C]"""
    squeeze = img.ndim == 2
    p = img[..., None] if squeeze else img
    H, W = p.shape[:2]
    X, Y = warp_coords(H, W, angle, scale)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.full(p.shape, 16384, np.int64)
    for dy, dx, w in ((0, 0, (32 - fy) * (32 - fx) * 32), (0, 1, (32 - fy) * fx * 32), (1, 0, fy * (32 - fx) * 32),
                      (1, 1, fy * fx * 32)):
        ty, tx = sy + dy, sx + dx
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        tap = np.where(ok[..., None], p[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), 0)
        acc += w[..., None] * tap
    out = (acc >> 15).astype(np.uint8)
    return out[..., 0] if squeeze else out


def bgr2yuv(img):
    b, g, r = (img[..., i].astype(np.int64) for i in range(3))
    y = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
    u = ((b - y) * 8061 + (128 << 14) + 8192) >> 14
    v = ((r - y) * 14369 + (128 << 14) + 8192) >> 14
    return np.clip(np.stack([y, u, v], -1), 0, 255).astype(np.uint8)


def yuv2bgr(img):
    y, u, v = (img[..., i].astype(np.int64) for i in range(3))
    u, v = u - 128, v - 128
    b = y + ((u * 33292 + 8192) >> 14)
    g = y + ((u * -6472 + v * -9519 + 8192) >> 14)
    r = y + ((v * 18678 + 8192) >> 14)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def clahe_luts(plane):
    """the 8x8 tile LUTs of CLAHE(clipLimit=2.0) of a uint8 plane: [8, 8, 256] uint8, and the tile size (th, tw)"""
    H, W = plane.shape
    if H % 8 or W % 8:
        plane = plane[reflect101(np.arange(H + 8 - H % 8), H)][:, reflect101(np.arange(W + 8 - W % 8), W)]
    th, tw = plane.shape[0] // 8, plane.shape[1] // 8
    area = th * tw
    clip = max(int(2.0 * area / 256), 1)
    luts = np.zeros((8, 8, 256), np.uint8)
    scale = np.float32(255.0) / np.float32(area)
    for ty in range(8):
        for tx in range(8):
            h = np.bincount(plane[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            excess = int(np.maximum(h - clip, 0).sum())
            h = np.minimum(h, clip) + excess // 256
            residual = excess % 256
            if residual:
                step = max(256 // residual, 1)
                i = 0
                while i < 256 and residual > 0:
                    h[i] += 1
                    i += step
                    residual -= 1
            cs = np.cumsum(h).astype(np.float32)
            luts[ty, tx] = np.clip(np.rint(cs * scale), 0, 255).astype(np.uint8)
    return luts, (th, tw)


def clahe(plane):
    """cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(plane), uint8 [H,W]"""
    H, W = plane.shape
    luts, (th, tw) = clahe_luts(plane)

    def axis(n, t):
        f = np.arange(n, dtype=np.float32) * (np.float32(1.0) / np.float32(t)) - np.float32(0.5)
        t1 = np.floor(f)
        a = (f - t1).astype(np.float32)
        t1 = t1.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, 7), a, (np.float32(1.0) - a).astype(np.float32)

    x1, x2, xa, xa1 = axis(W, tw)
    y1, y2, ya, ya1 = axis(H, th)
    v = plane.astype(np.int64)
    Y1, Y2 = y1[:, None], y2[:, None]
    l11 = luts[Y1, x1[None, :], v].astype(np.float32)
    l12 = luts[Y1, x2[None, :], v].astype(np.float32)
    l21 = luts[Y2, x1[None, :], v].astype(np.float32)
    l22 = luts[Y2, x2[None, :], v].astype(np.float32)
    res = (l11 * xa1 + l12 * xa) * ya1[:, None] + (l21 * xa1 + l22 * xa) * ya[:, None]
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def augment_image(image, label, p, out_hw, warp, histeq, n_classes):
    """one image through utils.py:317-365 with parameters p (augment.ImageParams): uint8 image [H,W,3], label [H,W]
    (uint8 / int32) -> image uint8 [h,w,3], label [h,w] (the label's dtype; void relabel applied)"""
    labels = np.unique(label)                                              # :317
    if p.blur:
        image = gaussian_blur5(image)                                      # :319-320
    h, w = out_hw
    image = image[p.cy:p.cy + h, p.cx:p.cx + w]                            # :326-327
    label = label[p.cy:p.cy + h, p.cx:p.cx + w]
    if p.hflip:
        image, label = image[:, ::-1], label[:, ::-1]
    if p.vflip:
        image, label = image[::-1], label[::-1]
    if p.gamma is not None:
        image = gamma_lut(p.gamma)[image]                                  # :336-341
    if warp:
        image = warp_affine(image, p.angle, p.scale)                       # :342-353
        label = warp_affine(label, p.angle, p.scale)
    if histeq:
        yuv = bgr2yuv(image)                                               # :355-358
        yuv[..., 0] = clahe(yuv[..., 0])
        image = yuv2bgr(yuv)
    out = label.astype(np.int32)                                           # :360-365
    for j in np.setxor1d(np.unique(out), labels):
        out[out == j] = n_classes
    return np.ascontiguousarray(image), out.astype(label.dtype)


def augment_batch(images, labels, params, out_hw, warp, histeq, n_classes):
    """augment_image over a batch: (X float32 [B,h,w,3], labels [B,h,w])"""
    res = [augment_image(i, l, p, out_hw, warp, histeq, n_classes) for i, l, p in zip(images, labels, params)]
    return np.stack([r[0] for r in res]).astype(np.float32), np.stack([r[1] for r in res])
