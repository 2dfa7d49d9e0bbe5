"""Training augmentation of the reference's SegmentationGenerator.__getitem__ (utils.py:310-369) on the device.

The host draws the per-image parameters from one `random.Random(seed)` in the reference's call order and takes every
floating-point decision in float64 numpy, exactly as cv2 does it [cv2-semantics]: the gamma LUT (the reference's own
numpy expression), getRotationMatrix2D + invertAffineTransform, warpAffine's fixed-point tables (AB_SCALE = 1024,
1/32-pixel taps) and CLAHE's tile interpolation weights.  `launch` uploads them as flat int / float tables and runs
dl3_augment (csrc/augment.hip) on the current stream; the device does integer adds and shifts only.

cv2.resize (utils.py:322-324, :421-422) is opt-in (`Plan(..., device_resize=True)`): images of any size, different within
a batch, go through dl3_cv_resize (csrc/cvresize.hip) in front of dl3_augment.  `resize_tables` restates cv2's float32
source coordinates and 11-bit coefficients per axis; `front_tables` packs them with the per-image descriptors and checks
every descriptor against its pool, because the device trusts them.  `cv_resize` is the stand-alone wrapper.

Out of scope (raise): file reading, interpolations other than INTER_LINEAR / INTER_NEAREST, blur sizes other than 5; without
device_resize, cv2.resize from a source size different from the target.
"""
import math
from collections import namedtuple

import numpy as np

from . import capi

AB_SCALE = 1024
CLAHE_TILES = 8
RESIZE_COEF_SCALE = 2048     # cv2's INTER_RESIZE_COEF_SCALE (11 bits)
FRONT_DESC = 12              # ints per image descriptor of dl3_cv_resize

# one image's draws: blur applied?, crop origin, flips, gamma factor (None: no LUT), rotation angle (deg), zoom scale
ImageParams = namedtuple("ImageParams", "blur cx cy hflip vflip gamma angle scale")


class Plan:
    """The batch-independent half of an augmentation: source size (Hs, Ws), output size (H, W) and the options of the
    reference's generator (resize_shape / crop_shape are cv2's (width, height)).

    device_resize=True: the sources may have any size (src_hw None: they differ), cv2.resize / the per-image crop run in
    dl3_cv_resize together with the blur, and `inner` is the plan of the rest of the chain over the uniform H x W batch."""

    def __init__(self, src_hw, resize_shape=None, crop_shape=None, horizontal_flip=False, vertical_flip=False, blur=0,
                 brightness=0.0, rotation=0.0, zoom=0.0, do_ahisteq=False, device_resize=False):
        self.front = bool(device_resize)
        self.Hs, self.Ws = (int(src_hw[0]), int(src_hw[1])) if src_hw is not None else (None, None)
        self.blur = int(blur or 0)
        if self.blur and self.blur != 5:
            raise ValueError("blur: only the 5x5 Gaussian (blur=5) is implemented, got %r" % (blur,))
        self.crop = False
        self.crop_shape = (int(crop_shape[0]), int(crop_shape[1])) if crop_shape else None
        if self.front:
            shape = self.crop_shape or (resize_shape and (int(resize_shape[0]), int(resize_shape[1])))
            if shape:
                self.H, self.W = shape[1], shape[0]
            elif src_hw is not None:
                self.H, self.W = self.Hs, self.Ws
            else:
                raise ValueError("device_resize: images of different sizes need resize_shape or crop_shape "
                                 "('No image dimensions specified!', utils.py:305)")
            if self.H < 1 or self.W < 1:
                raise ValueError("device_resize: the output size must be positive, got %dx%d" % (self.W, self.H))
        elif src_hw is None:
            raise ValueError("Plan: src_hw is needed without device_resize")
        elif crop_shape:
            cw, ch = int(crop_shape[0]), int(crop_shape[1])
            if cw < self.Ws and ch < self.Hs:                 # _random_crop, utils.py:411-423
                self.crop, (self.H, self.W) = True, (ch, cw)
            else:                                             # its else branch resizes to crop_shape
                self._same_size(crop_shape, "crop_shape")
        elif resize_shape:                                    # cv2.resize, utils.py:322-324
            self._same_size(resize_shape, "resize_shape")
        else:
            self.H, self.W = self.Hs, self.Ws
        self.hflip, self.vflip = bool(horizontal_flip), bool(vertical_flip)
        self.brightness, self.rotation, self.zoom = float(brightness or 0), float(rotation or 0), float(zoom or 0)
        self.histeq = bool(do_ahisteq)
        self.warp = bool(self.rotation or self.zoom)
        self.active = bool(self.front or self.blur or self.crop or self.hflip or self.vflip or self.brightness or
                           self.warp or self.histeq)
        self.flags = (1 if self.warp else 0) | (2 if self.histeq else 0)
        # the chain behind the front end: blur and crop are done, the source IS the H x W batch
        self.inner = Plan((self.H, self.W), None, None, horizontal_flip, vertical_flip, 0, brightness, rotation, zoom,
                          do_ahisteq) if self.front else None

    def _same_size(self, shape, what):
        if (int(shape[1]), int(shape[0])) != (self.Hs, self.Ws):
            raise ValueError("%s %r differs from the %dx%d source: cv2.resize is out of scope, resize the images on the "
                             "host first" % (what, tuple(shape), self.Ws, self.Hs))
        self.H, self.W = self.Hs, self.Ws

    def crops(self, src_hw):
        """device_resize: does an image of this size take _random_crop's crop branch (utils.py:415)?  Otherwise it is
        resized to (H, W)"""
        return bool(self.crop_shape and self.W < int(src_hw[1]) and self.H < int(src_hw[0]))

    def draw(self, rnd, src_hw=None):
        """one image's parameters, drawn from `rnd` (random.Random) in the order of utils.py:319-350; src_hw: the image's
        own size (device_resize: whether it crops, and from which range, depends on it)"""
        blur = bool(self.blur and rnd.randint(0, 1))
        cx = cy = 0
        if self.front:
            if src_hw is None:
                src_hw = (self.Hs, self.Ws)
            if self.crops(src_hw):
                cx = rnd.randrange(int(src_hw[1]) - self.W)
                cy = rnd.randrange(int(src_hw[0]) - self.H)
        elif self.crop:
            cx = rnd.randrange(self.Ws - self.W)
            cy = rnd.randrange(self.Hs - self.H)
        hflip = bool(self.hflip and rnd.randint(0, 1))
        vflip = bool(self.vflip and rnd.randint(0, 1))
        gamma = None
        if self.brightness:
            gamma = 1.0 + rnd.gauss(0.0, self.brightness)
            if rnd.randint(0, 1):
                gamma = 1.0 / gamma
        angle = rnd.gauss(0.0, self.rotation) if self.rotation else 0.0
        scale = rnd.gauss(1.0, self.zoom) if self.zoom else 1.0
        return ImageParams(blur, cx, cy, hflip, vflip, gamma, angle, scale)


def gamma_lut(factor):
    """utils.py:339-340 (float64, truncated by astype(uint8)), vectorised: the reference's per-element list
    comprehension costs ~0.7 ms per image, i.e. most of a 512² batch's host time; tests/test_augment_host.py pins the two
    forms against each other"""
    with np.errstate(all="ignore"):
        return (((np.arange(0, 256) / 255.0) ** factor) * 255).astype(np.uint8)


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D [cv2-semantics]"""
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


def invert_affine(M):
    """cv2.invertAffineTransform [cv2-semantics], in float64"""
    M = np.asarray(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    A12, A21 = -M[0, 1] * D, -M[1, 0] * D
    b1 = -A11 * M[0, 2] - A12 * M[1, 2]
    b2 = -A21 * M[0, 2] - A22 * M[1, 2]
    return np.array([[A11, A12, b1], [A21, A22, b2]])


def warp_tables(H, W, angle, scale):
    """warpAffine's fixed-point tables for an H x W image [cv2-semantics]: (adelta[W], bdelta[W], X0[H], Y0[H]) int32;
    source X = (X0[y] + adelta[x]) >> 5 in 1/32 pixels, likewise Y"""
    A = invert_affine(rotation_matrix_2d((W // 2, H // 2), angle, scale))
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    adelta = np.rint(A[0, 0] * x * AB_SCALE)
    bdelta = np.rint(A[1, 0] * x * AB_SCALE)
    X0 = np.rint((A[0, 1] * y + A[0, 2]) * AB_SCALE) + AB_SCALE // 32 // 2
    Y0 = np.rint((A[1, 1] * y + A[1, 2]) * AB_SCALE) + AB_SCALE // 32 // 2
    return tuple(a.astype(np.int32) for a in (adelta, bdelta, X0, Y0))


def clahe_tile_size(H, W):
    """(tile height, tile width) of CLAHE(8x8) [cv2-semantics]: when H or W is not a multiple of 8 the plane is padded
    bottom / right by 8 - H % 8 and 8 - W % 8 (reflect-101)"""
    if H % CLAHE_TILES or W % CLAHE_TILES:
        H, W = H + CLAHE_TILES - H % CLAHE_TILES, W + CLAHE_TILES - W % CLAHE_TILES
    return H // CLAHE_TILES, W // CLAHE_TILES


def clahe_axis(n, t):
    """per coordinate of one axis: (lower tile, upper tile) int32 [n,2] and (a, 1-a) float32 [n,2] [cv2-semantics]"""
    inv = np.float32(1.0) / np.float32(t)
    f = np.arange(n, dtype=np.float32) * inv - np.float32(0.5)
    t1 = np.floor(f)
    a = (f - t1).astype(np.float32)
    t1 = t1.astype(np.int32)
    i = np.stack([np.maximum(t1, 0), np.minimum(t1 + 1, CLAHE_TILES - 1)], 1).astype(np.int32)
    w = np.stack([a, np.float32(1.0) - a], 1).astype(np.float32)
    return i, w


def tables(plan, params):
    """every table dl3_augment reads, packed into ONE int32 array (one upload); returns (array, offsets)"""
    B, H, W = len(params), plan.H, plan.W
    ip = np.zeros((B, 8), np.int32)
    lut = np.tile(np.arange(256, dtype=np.int32), (B, 1))
    for n, p in enumerate(params):
        ip[n, :5] = (p.blur, p.cx, p.cy, p.hflip, p.vflip)
        if p.gamma is not None:
            lut[n] = gamma_lut(p.gamma)
    parts = [("img", ip), ("lut", lut)]
    if plan.warp or plan.histeq:
        wt = np.empty((B, 2 * (W + H)), np.int32)
        for n, p in enumerate(params):
            wt[n] = np.concatenate(warp_tables(H, W, p.angle, p.scale))
        parts.append(("warp", wt))
    if plan.histeq:
        th, tw = clahe_tile_size(H, W)
        xi, xw = clahe_axis(W, tw)
        yi, yw = clahe_axis(H, th)
        parts.append(("clahe_i", np.concatenate([xi.ravel(), yi.ravel()])))
        parts.append(("clahe_f", np.concatenate([xw.ravel(), yw.ravel()]).view(np.int32)))
    offs, o = {}, 0
    for k, a in parts:
        offs[k] = o
        o += a.size
    return np.concatenate([a.ravel() for _, a in parts]).astype(np.int32), offs


def workspace_bytes(plan, B):
    return int(capi.lib().dl3_augment_workspace_bytes(B, plan.H, plan.W, plan.flags))


def launch(plan, tab, offs, images, labels, n_classes, X, labels_out, workspace, stream=None, present=None):
    """dl3_augment on `stream` (default: the current one).  tab: the device copy of `tables(...)[0]` (int32);
    images uint8 [B,Hs,Ws,3], labels uint8 / int32 [B,Hs,Ws] -> X float32 [B,H,W,3], labels_out [B,H,W].
    present: int32 [B,8] label sets from dl3_cv_resize (dl3_augment_present) instead of those of `labels`"""
    import torch
    B = images.shape[0]
    lcode = capi.LABEL_U8 if labels.dtype == torch.uint8 else capi.LABEL_I32
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    base = tab.data_ptr()

    def at(k):
        return base + 4 * offs[k] if k in offs else None

    wsz = workspace.numel() * workspace.element_size() if workspace is not None else 0
    head = (images.data_ptr(), labels.data_ptr(), lcode, B, plan.Hs, plan.Ws, plan.H, plan.W, plan.flags, at("img"),
            at("lut"), at("warp"), at("clahe_i"), at("clahe_f"), int(n_classes))
    tail = (X.data_ptr(), labels_out.data_ptr(), workspace.data_ptr() if workspace is not None else None, wsz, st)
    if present is None:
        capi.call("dl3_augment", *(head + tail))
    else:
        capi.call("dl3_augment_present", *(head + (present.data_ptr(),) + tail))


# ---------------------------------------------------------------- cv2.resize in front of the chain (dl3_cv_resize)
def resize_axis(src, dst, columns):
    """one axis of cv2.resize for 8-bit images [cv2-semantics]: (s, c0, c1, nearest), int32 [dst] each.  INTER_LINEAR:
    f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s; columns clamp s to [0, src-1] and zero f there, rows keep
    f (the device clamps both taps); c = rint(float32 weight * 2048).  INTER_NEAREST: min(floor(d * scale), src - 1).
    scale = 1 / (dst / src) in float64, the reciprocal of the quotient."""
    src, dst = int(src), int(dst)
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    if columns:
        lo, hi = s < 0, s >= src - 1
        f[lo | hi] = 0
        s[lo] = 0
        s[hi] = src - 1
    c0 = np.rint((np.float32(1.0) - f) * np.float32(RESIZE_COEF_SCALE))
    c1 = np.rint(f * np.float32(RESIZE_COEF_SCALE))
    near = np.minimum(np.floor(d * scale).astype(np.int64), src - 1)
    return tuple(a.astype(np.int32) for a in (s, c0, c1, near))


def resize_tables(src_hw, dst_hw):
    """the int32 tables dl3_cv_resize reads for one source size: xs[W], xa0[W], xa1[W], xn[W], ys[H], yb0[H], yb1[H],
    yn[H] concatenated (4W + 4H)"""
    return np.concatenate(resize_axis(src_hw[1], dst_hw[1], True) + resize_axis(src_hw[0], dst_hw[0], False))


FrontInfo = namedtuple("FrontInfo", "B H W max_hs max_ws blur_any pool_px")


def front_tables(sizes, dst_hw, crops=None, blur=None, px_offsets=None, pool_px=None):
    """descriptors + resize tables of one ragged batch for dl3_cv_resize, as ONE int32 array: (array, offsets, FrontInfo).
    sizes: (Hs, Ws) per image; crops: per image None (resize to dst_hw) or the (x, y) origin of the H x W crop; blur: per
    image flag; px_offsets: where each image starts in the pools, in pixels (default: back to back); pool_px: the pools'
    capacity in pixels (default: what the batch needs).  The tables are built once per distinct source size.
    Everything the device will trust is checked here."""
    H, W = int(dst_hw[0]), int(dst_hw[1])
    B = len(sizes)
    if B < 1 or H < 1 or W < 1:
        raise ValueError("front_tables: needs at least one image and a positive output size, got %d to %dx%d" % (B, W, H))
    crops = list(crops) if crops is not None else [None] * B
    blur = list(blur) if blur is not None else [False] * B
    sizes = [(int(h), int(w)) for h, w in sizes]
    if any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError("front_tables: empty source image among %r" % (sizes,))
    px = np.array([h * w for h, w in sizes], np.int64)
    if px_offsets is None:
        px_offsets = np.concatenate([[0], np.cumsum(px)[:-1]])
    px_offsets = np.asarray(px_offsets, np.int64)
    need = int((px_offsets + px).max())
    pool_px = need if pool_px is None else int(pool_px)
    if len(px_offsets) != B or len(crops) != B or len(blur) != B:
        raise ValueError("front_tables: one size, crop, blur flag and offset per image")
    if px_offsets.min() < 0 or need > pool_px or 3 * pool_px >= 2 ** 31:
        raise ValueError("front_tables: images of %d pixels do not fit a pool of %d (at most 2^31 bytes)" % (need, pool_px))
    desc = np.zeros((B, FRONT_DESC), np.int32)
    tabs, where, o = [], {}, B * FRONT_DESC
    for n, ((hs, ws), c) in enumerate(zip(sizes, crops)):
        desc[n, :5] = (3 * px_offsets[n], px_offsets[n], hs, ws, bool(blur[n]))
        if c is not None:
            cx, cy = int(c[0]), int(c[1])
            if cx < 0 or cy < 0 or cx + W > ws or cy + H > hs:
                raise ValueError("front_tables: crop %dx%d at (%d, %d) leaves the %dx%d image %d" % (W, H, cx, cy, ws, hs, n))
            desc[n, 5:8] = (1, cx, cy)
            continue
        if (hs, ws) not in where:
            t = resize_tables((hs, ws), (H, W))
            xs, xn, yn = t[:W], t[3 * W:4 * W], t[4 * W + 3 * H:]
            assert xs.min() >= 0 and xs.max() < ws and xn.min() >= 0 and xn.max() < ws and yn.min() >= 0 and yn.max() < hs
            where[(hs, ws)] = o - B * FRONT_DESC
            tabs.append(t)
            o += t.size
        desc[n, 8] = where[(hs, ws)]
    arr = np.concatenate([desc.ravel()] + tabs + ([] if tabs else [np.zeros(1, np.int32)])).astype(np.int32)
    info = FrontInfo(B, H, W, max(h for h, _ in sizes), max(w for _, w in sizes), int(any(blur)), pool_px)
    return arr, {"fdesc": 0, "ftab": B * FRONT_DESC}, info


def batch_tables(plan, sizes, params):
    """device_resize: the tables of the front end and of the chain behind it as ONE int32 array (one upload):
    (array, offsets, FrontInfo)"""
    crops = [(p.cx, p.cy) if plan.crops(hw) else None for hw, p in zip(sizes, params)]
    front, offs, info = front_tables(sizes, (plan.H, plan.W), crops, [p.blur for p in params])
    inner, ioffs = tables(plan.inner, [p._replace(blur=False, cx=0, cy=0) for p in params])
    offs.update({k: v + front.size for k, v in ioffs.items()})
    return np.concatenate([front, inner]), offs, info


def pack_pools(images, labels, img_pool=None, lab_pool=None):
    """the images ([Hs,Ws,3] uint8 each) and label maps back to back in two flat arrays (or into the given ones, which
    may be larger)"""
    n = sum(int(np.shape(i)[0]) * int(np.shape(i)[1]) for i in (images if images is not None else labels))
    if images is not None:
        img_pool = np.empty(3 * n, np.uint8) if img_pool is None else img_pool
        o = 0
        for i in images:
            i = np.asarray(i)
            img_pool[o:o + i.size] = i.reshape(-1)
            o += i.size
    if labels is not None:
        lab_pool = np.empty(n, np.asarray(labels[0]).dtype) if lab_pool is None else lab_pool
        o = 0
        for l in labels:
            l = np.asarray(l)
            lab_pool[o:o + l.size] = l.reshape(-1)
            o += l.size
    return img_pool, lab_pool


def front_workspace_bytes(info):
    return int(capi.lib().dl3_cv_resize_workspace_bytes(3 * info.pool_px, info.blur_any))


def launch_front(info, tab, offs, img_pool, lab_pool, images_out, labels_out, present, workspace, stream=None):
    """dl3_cv_resize on `stream` (default: the current one).  tab: the device copy of front_tables(...)[0] / batch_tables
    (...)[0]; img_pool uint8 [>= 3 * pool_px] and lab_pool uint8 / int32 [>= pool_px] device tensors (either may be None
    with its output) -> images_out uint8 [B,H,W,3], labels_out [B,H,W], present int32 [B,8] (may be None)"""
    import torch
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    for t, n, what in ((img_pool, 3 * info.pool_px, "image"), (lab_pool, info.pool_px, "label")):
        if t is not None and t.numel() < n:
            raise ValueError("launch_front: the %s pool holds %d elements, the descriptors cover %d" % (what, t.numel(), n))
    lcode = capi.LABEL_I32 if lab_pool is not None and lab_pool.dtype == torch.int32 else capi.LABEL_U8
    if lab_pool is not None and lab_pool.dtype not in (torch.uint8, torch.int32):
        raise ValueError("launch_front: label maps are uint8 or int32, got %s" % lab_pool.dtype)
    base = tab.data_ptr()
    wsz = workspace.numel() * workspace.element_size() if workspace is not None else 0

    def p(t):
        return t.data_ptr() if t is not None else None

    capi.call("dl3_cv_resize", p(img_pool), 3 * info.pool_px, p(lab_pool), lcode, info.B, info.max_hs, info.max_ws,
              info.H, info.W, info.blur_any, base + 4 * offs["fdesc"], base + 4 * offs["ftab"], p(images_out),
              p(labels_out), p(present), p(workspace), wsz, st)


def cv_resize(images, dsize, interpolation="linear"):
    """cv2.resize(image, dsize) on the device for a batch of images of any sizes: dsize is cv2's (width, height).
    interpolation="linear" (cv2's default): uint8 images [Hs,Ws,3] -> uint8 [N,h,w,3]; "nearest": uint8 / int32 maps
    [Hs,Ws] (other integer types are converted to int32) -> [N,h,w] in that type.  `images` is a list (or an array) of
    them; one bare image comes back as one image.  Host arrays in, host arrays out."""
    import torch
    if interpolation not in ("linear", "nearest"):
        raise ValueError("cv_resize: interpolation must be 'linear' or 'nearest', got %r" % (interpolation,))
    w, h = int(dsize[0]), int(dsize[1])
    if w < 1 or h < 1:
        raise ValueError("cv_resize: dsize must be positive, got %r" % (dsize,))
    linear = interpolation == "linear"
    one = isinstance(images, np.ndarray) and images.ndim == (3 if linear else 2)
    items = [np.asarray(i) for i in ([images] if one else images)]
    if not items:
        raise ValueError("cv_resize: no images")
    for i in items:
        if linear and (i.ndim != 3 or i.shape[2] != 3 or i.dtype != np.uint8):
            raise ValueError("cv_resize: 'linear' takes uint8 [H,W,3] images, got %s %r" % (i.dtype, i.shape))
        if not linear and (i.ndim != 2 or i.dtype.kind not in "iu"):
            raise ValueError("cv_resize: 'nearest' takes integer [H,W] maps, got %s %r" % (i.dtype, i.shape))
    if not linear:
        dt = np.uint8 if all(i.dtype == np.uint8 for i in items) else np.int32
        if dt == np.int32 and any(i.size and (i.min() < -2 ** 31 or i.max() >= 2 ** 31) for i in items):
            raise ValueError("cv_resize: map values do not fit int32")
        items = [i.astype(dt, copy=False) for i in items]
    tab, offs, info = front_tables([i.shape[:2] for i in items], (h, w))
    dtab = torch.from_numpy(tab).cuda()
    ipool, lpool = pack_pools(items if linear else None, None if linear else items)
    pool = torch.from_numpy(ipool if linear else lpool).cuda()
    out = torch.empty((len(items), h, w, 3) if linear else (len(items), h, w), dtype=pool.dtype, device="cuda")
    launch_front(info, dtab, offs, pool if linear else None, None if linear else pool, out if linear else None,
                 None if linear else out, None, None)
    res = out.cpu().numpy()
    return res[0] if one else res
