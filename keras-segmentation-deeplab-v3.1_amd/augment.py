"""Training augmentation of the reference's SegmentationGenerator.__getitem__ (utils.py:310-369) on the device.

The host draws the per-image parameters from one `random.Random(seed)` in the reference's call order and takes every
floating-point decision in float64 numpy, exactly as cv2 does it [cv2-semantics]: the gamma LUT (the reference's own
numpy expression), getRotationMatrix2D + invertAffineTransform, warpAffine's fixed-point tables (AB_SCALE = 1024,
1/32-pixel taps) and CLAHE's tile interpolation weights.  `launch` uploads them as flat int / float tables and runs
dl3_augment (csrc/augment.hip) on the current stream; the device does integer adds and shifts only.

Out of scope (raise): file reading, cv2.resize from a source size different from the target, blur sizes other than 5.
"""
import math
from collections import namedtuple

import numpy as np

from . import capi

AB_SCALE = 1024
CLAHE_TILES = 8

# one image's draws: blur applied?, crop origin, flips, gamma factor (None: no LUT), rotation angle (deg), zoom scale
ImageParams = namedtuple("ImageParams", "blur cx cy hflip vflip gamma angle scale")


class Plan:
    """The batch-independent half of an augmentation: source size (Hs, Ws), output size (H, W) and the options of the
    reference's generator (resize_shape / crop_shape are cv2's (width, height))."""

    def __init__(self, src_hw, resize_shape=None, crop_shape=None, horizontal_flip=False, vertical_flip=False, blur=0,
                 brightness=0.0, rotation=0.0, zoom=0.0, do_ahisteq=False):
        self.Hs, self.Ws = int(src_hw[0]), int(src_hw[1])
        self.blur = int(blur or 0)
        if self.blur and self.blur != 5:
            raise ValueError("blur: only the 5x5 Gaussian (blur=5) is implemented, got %r" % (blur,))
        self.crop = False
        if crop_shape:
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
        self.active = bool(self.blur or self.crop or self.hflip or self.vflip or self.brightness or self.warp or
                           self.histeq)
        self.flags = (1 if self.warp else 0) | (2 if self.histeq else 0)

    def _same_size(self, shape, what):
        if (int(shape[1]), int(shape[0])) != (self.Hs, self.Ws):
            raise ValueError("%s %r differs from the %dx%d source: cv2.resize is out of scope, resize the images on the "
                             "host first" % (what, tuple(shape), self.Ws, self.Hs))
        self.H, self.W = self.Hs, self.Ws

    def draw(self, rnd):
        """one image's parameters, drawn from `rnd` (random.Random) in the order of utils.py:319-350"""
        blur = bool(self.blur and rnd.randint(0, 1))
        cx = cy = 0
        if self.crop:
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


def launch(plan, tab, offs, images, labels, n_classes, X, labels_out, workspace, stream=None):
    """dl3_augment on `stream` (default: the current one).  tab: the device copy of `tables(...)[0]` (int32);
    images uint8 [B,Hs,Ws,3], labels uint8 / int32 [B,Hs,Ws] -> X float32 [B,H,W,3], labels_out [B,H,W]"""
    import torch
    B = images.shape[0]
    lcode = capi.LABEL_U8 if labels.dtype == torch.uint8 else capi.LABEL_I32
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    base = tab.data_ptr()

    def at(k):
        return base + 4 * offs[k] if k in offs else None

    wsz = workspace.numel() * workspace.element_size() if workspace is not None else 0
    capi.call("dl3_augment", images.data_ptr(), labels.data_ptr(), lcode, B, plan.Hs, plan.Ws, plan.H, plan.W,
              plan.flags, at("img"), at("lut"), at("warp"), at("clahe_i"), at("clahe_f"), int(n_classes), X.data_ptr(),
              labels_out.data_ptr(), workspace.data_ptr() if workspace is not None else None, wsz, st)
