"""The case table of tests/test_gpu_conv3x3.py (dense 3x3 convolutions, csrc/conv3x3.hip) and what a case needs on the
host: its seeded inputs, the mask nudge, and the launch predicates of conv3x3.hip restated in Python.  Importable without
a GPU: tests/test_conv3x3_cases_host.py checks the table here, against torch and against the predicates."""
import zlib
from collections import namedtuple

import numpy as np

from oracle import dl3_oracle as O

ACT_NAME = {None: "", 1: "relu", 2: "relu6"}
MASK_MARGIN = 1e-3   # no pre-activation of a test input lies this close to an activation threshold

# geom: (N, H, W, Cin, Cout, stride, pad_t, pad_l, Ho, Wo), the trailing arguments of every dl3_conv3x3_* launch
# api: "direct" = dl3_conv3x3_fwd / _bwd_weight / _bwd_data, "tap" = dl3_conv3x3_mfma_*
# ops: which launches the case drives: f forward, w weight gradient, d backward-data
# xform, act: the input view: "none", "affine", "act" or "affine+act" (tests/test_gpu_ops.py FORMS), act 1 relu / 2 relu6
# shift: "normal" or "positive" (uniform [0.3, 0.9]: act(shift) != 0, a padding tap that leaks the shift shows)
# grad: "bn" = the gradient operand cA*g + cB*yraw + cC, "plain" = g itself (cA == NULL)
# add: bwd-data with dx_add;  stats: with the statistic partials (forward and bwd-data);  xnull: bwd-data without x
# branch: the paths of conv3x3.hip the case is there for (BRANCH below holds the condition of each)
Case = namedtuple("Case", "id api geom ops xform act shift grad add stats xnull branch")


def same(N, H, W, Cin, Cout, stride):
    Ho, pt, _ = O.same_pads(H, 3, stride, 1)
    Wo, pl, _ = O.same_pads(W, 3, stride, 1)
    return (N, H, W, Cin, Cout, stride, pt, pl, Ho, Wo)


def explicit(N, H, W, Cin, Cout, stride):
    """ZeroPadding2D + VALID, the stride-2 form of the xception entry flow"""
    Ho, pt, _ = O.explicit_pads(H, 3, stride, 1)
    Wo, pl, _ = O.explicit_pads(W, 3, stride, 1)
    return (N, H, W, Cin, Cout, stride, pt, pl, Ho, Wo)


def _c(id, api, geom, ops, xform="none", act=None, shift="normal", grad="bn", add=False, stats=True, xnull=False,
       branch=()):
    return Case(id, api, geom, ops, xform, act, shift, grad, add, stats, xnull, tuple(branch))


S1 = same(1, 5, 7, 3, 32, 2)     # 12 output pixels
S2 = same(1, 8, 8, 3, 32, 1)     # 64 output pixels

# ---- dl3_conv3x3_fwd / dl3_conv3x3_bwd_weight on the matrix-pipe stem kernels (Cin <= 3, Cout == 32) -------------------
STEM = [
    _c("stem-ragged-only", "direct", S1, "fw", "affine", branch=("stem", "stem-wgrad", "np<32")),
    _c("stem-full-tiles-idle-waves", "direct", S2, "fw", "none", branch=("stem", "stem-wgrad", "np%32==0", "stride1")),
    _c("stem-cin1", "direct", same(2, 9, 6, 1, 32, 2), "fw", "affine", branch=("stem", "stem-wgrad")),
    _c("stem-cin2", "direct", same(1, 7, 9, 2, 32, 1), "fw", "none", branch=("stem", "stem-wgrad", "stride1")),
    _c("stem-valid", "direct", (1, 9, 11, 3, 32, 2, 0, 0, 4, 5), "fw", "affine", branch=("stem", "no-dead-tap", "np<32")),
    _c("stem-ragged-only-act-relu", "direct", S1, "fw", "act", 1, branch=("stem", "np<32")),
    _c("stem-full-tiles-act-relu", "direct", S2, "fw", "act", 1, branch=("stem", "np%32==0")),
    _c("stem-ragged-only-affine+act-relu6", "direct", S1, "fw", "affine+act", 2, "positive", branch=("stem", "np<32")),
    _c("stem-full-tiles-affine+act-relu6", "direct", S2, "fw", "affine+act", 2, "positive", branch=("stem", "np%32==0")),
    _c("stem-full-tiles-affine+act-relu", "direct", S2, "fw", "affine+act", 1, "positive", branch=("stem", "np%32==0")),
    _c("stem-ragged-only-plain-grad", "direct", S1, "fw", "affine", grad="plain", branch=("stem", "stem-wgrad", "np<32")),
]

# ---- one step outside each condition of the stem route: the direct kernel serves Cin = 3, Cout = 32 ---------------------
BOUNDARY = [
    _c("edge-h2", "direct", same(1, 2, 9, 3, 32, 1), "fw", "affine", branch=("not-stem",)),
    _c("edge-pad2", "direct", (1, 8, 8, 3, 32, 1, 2, 2, 10, 10), "fw", "affine", branch=("not-stem",)),
    _c("edge-overhang2", "direct", (1, 4, 4, 3, 32, 2, 1, 1, 3, 3), "fw", "affine", branch=("not-stem",)),
    _c("edge-overhang2-affine+act-relu6", "direct", (1, 4, 4, 3, 32, 2, 1, 1, 3, 3), "fw", "affine+act", 2, "positive",
       branch=("not-stem",)),
]

# ---- the direct vector-ALU kernels: channel widths (CQ = C/4, PL = 256/CQ), ragged input-channel chunks, grid stride ----
WIDTHS = (
    [_c("direct-cout%d" % co, "direct", same(2, 9, 11, 3, co, 2), "fw", "affine", branch=("not-stem",))
     for co in (4, 8, 16, 128, 256)] +
    [_c("direct-cout16-act-relu6", "direct", same(2, 9, 11, 3, 16, 2), "fw", "act", 2, grad="plain", branch=("not-stem",)),
     _c("direct-cin4-chunk1", "direct", same(2, 9, 11, 4, 16, 2), "fw", "affine+act", 1, branch=("chunk1",)),
     _c("direct-cin5-chunk2", "direct", same(2, 9, 11, 5, 16, 2), "fw", "affine", branch=("chunk2",))] +
    [_c("direct-dgrad-cin%d" % ci, "direct", same(2, 9, 11, ci, 8, 1), "fwd", "affine+act", 1) for ci in (4, 8, 16, 64)] +
    [_c("direct-loop-fwd", "direct", same(1, 96, 96, 3, 256, 1), "fw", "affine", branch=("not-stem", "loop-out")),
     _c("direct-loop-dgrad", "direct", same(1, 96, 96, 256, 4, 1), "d", "affine+act", 2, branch=("loop-in",))]
)

# ---- direct backward-data at stride 2 (32 -> 64 channels) -----------------------------------------------------------------
D_EVEN, D_ODD, D_EXPL = same(1, 16, 18, 32, 64, 2), same(1, 15, 17, 32, 64, 2), explicit(1, 16, 16, 32, 64, 2)
DGRAD = [
    _c("dgrad-s2-even-pad0", "direct", D_EVEN, "d", "affine+act", 1, branch=("s2-pad0",)),
    _c("dgrad-s2-odd-pad1", "direct", D_ODD, "d", "affine+act", 2, branch=("s2-pad1",)),
    _c("dgrad-s2-explicit", "direct", D_EXPL, "d", "affine+act", 1, branch=("s2-pad1",)),
    _c("dgrad-s2-even-pad0-add", "direct", D_EVEN, "d", "affine+act", 2, add=True, branch=("s2-pad0",)),
    _c("dgrad-s2-odd-pad1-add", "direct", D_ODD, "d", "affine+act", 1, add=True, branch=("s2-pad1",)),
    _c("dgrad-s2-explicit-add", "direct", D_EXPL, "d", "affine+act", 2, add=True, branch=("s2-pad1",)),
    _c("dgrad-s2-even-plain-grad", "direct", D_EVEN, "d", "affine+act", 1, grad="plain", branch=("s2-pad0",)),
    _c("dgrad-s2-odd-no-x", "direct", D_ODD, "d", "none", grad="plain", stats=False, xnull=True, branch=("s2-pad1",)),
    _c("dgrad-s2-even-act-relu6", "direct", D_EVEN, "d", "act", 2, branch=("s2-pad0",)),
    _c("dgrad-s2-explicit-affine-stats", "direct", D_EXPL, "d", "affine", add=True, branch=("s2-pad1",)),
]

# ---- the tap-gather MFMA kernels --------------------------------------------------------------------------------------------
TAP = (
    [_c("tap-s2-even-%dto%d" % (ci, co), "tap", same(1, 16, 18, ci, co, 2), "fwd", "affine+act", act, add=add,
        branch=("s2-pad0",)) for ci, co, act, add in ((32, 32, 1, False), (32, 64, 2, True), (64, 32, 2, False), (64, 64, 1, True))] +
    [_c("tap-s2-even-32to64-plain-grad", "tap", same(1, 16, 18, 32, 64, 2), "wd", "affine", grad="plain", branch=("s2-pad0",)),
     _c("tap-s2-even-64to32-no-stats", "tap", same(1, 16, 18, 64, 32, 2), "fd", "act", 1, stats=False, branch=("s2-pad0",)),
     _c("tap-second-step", "tap", same(1, 520, 512, 32, 32, 1), "fd", "affine+act", 1, add=True,
        branch=("tap-step2-out", "tap-step2-in"))]
)

DIRECT_CASES = STEM + BOUNDARY + WIDTHS + DGRAD
TAP_CASES = TAP
CASES = DIRECT_CASES + TAP_CASES


# ---- the launch arithmetic of conv3x3.hip, restated ---------------------------------------------------------------------------
def out_pixels(g):
    return g[0] * g[8] * g[9]


def in_pixels(g):
    return g[0] * g[1] * g[2]


def conv_blocks(NP):
    """conv3x3.hip conv_blocks(): one workgroup per 32 pixels, at most 2048"""
    return max(1, min(2048, (NP + 31) // 32))


def pixel_lanes(C):
    """PL = 256 / CQ with CQ = C / 4 (conv3x3_fwd_kernel, _wgrad_kernel: C = Cout; _dgrad_kernel: C = Cin)"""
    return 256 // (C // 4)


def tap_blocks(NP):
    """conv3x3.hip tap_blocks(): one workgroup per 256 pixels, at most 1024"""
    return max(1, min(1024, (NP + 255) // 256))


def direct_supported(C):
    """conv_check() / dl3_conv3x3_bwd_data: the channel count the threads are laid along is 4 * (a divisor of 256)"""
    return C % 4 == 0 and 256 % (C // 4) == 0 and C // 4 <= 256


def stem_fwd_route(g):
    """the condition of dl3_conv3x3_fwd under which conv3x3_stem_fwd_mfma_kernel is launched"""
    N, H, W, Cin, Cout, s, pt, pl, Ho, Wo = g
    return (9 * Cin <= 28 and Cout == 32 and N * Ho * Wo < 2 ** 31 and N * H * W * Cin < 2 ** 30 and pt <= 1 and pl <= 1
            and H >= 3 and W >= 3 and (Ho - 1) * s - pt + 2 <= H and (Wo - 1) * s - pl + 2 <= W)


def stem_wgrad_route(g):
    """the condition of dl3_conv3x3_bwd_weight under which conv3x3_stem_wgrad_kernel is launched"""
    return 9 * g[3] <= 32 and g[4] == 32 and out_pixels(g) < 2 ** 31 - 64 * 2048


def dead_taps(g):
    """number of (output pixel, tap) pairs that fall into the padding"""
    N, H, W, Cin, Cout, s, pt, pl, Ho, Wo = g
    iy = np.arange(Ho)[:, None] * s - pt + np.arange(3)
    ix = np.arange(Wo)[:, None] * s - pl + np.arange(3)
    return int(((iy < 0) | (iy >= H)).sum() * 3 * Wo + ((ix < 0) | (ix >= W)).sum() * 3 * Ho)


# the condition behind each branch tag of the table
BRANCH = {
    "stem": stem_fwd_route,
    "not-stem": lambda g: not stem_fwd_route(g),
    "stem-wgrad": stem_wgrad_route,
    # conv3x3_stem_fwd_mfma_kernel: nfull == 0, only the peeled ragged tile runs
    "np<32": lambda g: out_pixels(g) < 32,
    # ... no ragged tile, and more waves (4 per workgroup) than full tiles
    "np%32==0": lambda g: out_pixels(g) % 32 == 0 and 4 * conv_blocks(out_pixels(g)) > out_pixels(g) // 32,
    "stride1": lambda g: g[5] == 1,
    "no-dead-tap": lambda g: dead_taps(g) == 0,
    # conv3x3_fwd_kernel / _wgrad_kernel (Cout) and _dgrad_kernel (Cin): the grid is at its cap of 2048 workgroups and still
    # short of pixels (a workgroup covers PL pixels but the grid is sized for 32, so with PL < 32 the loop also repeats below
    # the cap: what the cap adds is a stride of 2048 * PL)
    "loop-out": lambda g: out_pixels(g) > 2048 * pixel_lanes(g[4]),
    "loop-in": lambda g: in_pixels(g) > 2048 * pixel_lanes(g[3]),
    # conv3x3_wgrad_kernel: the last chunk of CI_CHUNK = 3 input channels holds one / two
    "chunk1": lambda g: g[3] % 3 == 1,
    "chunk2": lambda g: g[3] % 3 == 2,
    # backward-data at stride 2: with pad 0 the parity test alone decides which taps are live
    "s2-pad0": lambda g: g[5] == 2 and g[6] == 0 and g[7] == 0,
    "s2-pad1": lambda g: g[5] == 2 and g[6] == 1 and g[7] == 1,
    # conv3x3_tap_mfma_kernel: the outer `base += gridDim.x * 256` loop takes a second step
    "tap-step2-out": lambda g: out_pixels(g) > 262144 and tap_blocks(out_pixels(g)) == 1024,
    "tap-step2-in": lambda g: in_pixels(g) > 262144 and tap_blocks(in_pixels(g)) == 1024,
}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def thresholds(act):
    return {None: (), 0: (), 1: (0.0,), 2: (0.0, 6.0)}[act]


def preact(x, s, t):
    """the pre-activation of the input view in float64, from the float32 operands the kernel reads"""
    x = np.asarray(x, np.float64)
    return x if s is None else np.asarray(s, np.float64) * x + np.asarray(t, np.float64)


def nudge(x, s, t, act):
    """x (float32) with every element whose pre-activation s*x + t lies within MASK_MARGIN of a threshold of `act` moved so
    that it lies 2 * MASK_MARGIN away from it, on the side it was on; returns (x, number of elements moved).  A condition
    on the inputs: the fp32 kernel and the float64 reference then agree on every activation mask."""
    x = np.array(x, np.float32)
    sv = np.ones(x.shape[-1]) if s is None else np.asarray(s, np.float64)
    tv = np.zeros(x.shape[-1]) if t is None else np.asarray(t, np.float64)
    moved = np.zeros(x.shape, bool)
    for thr in thresholds(act):
        z = preact(x, s, t)
        near = np.abs(z - thr) < MASK_MARGIN
        target = thr + np.where(z >= thr, 2 * MASK_MARGIN, -2 * MASK_MARGIN)
        xn = ((target - tv) / sv).astype(np.float32)
        x = np.where(near, xn, x)
        moved |= near
    return x, int(moved.sum())


def draw_view(case):
    """the seeded input view of a case: (x float32 [N,H,W,Cin] after the nudge, in_scale, in_shift, in_act, moved)"""
    N, H, W, Cin = case.geom[:4]
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    act = case.act if case.xform.endswith("act") else 0
    x = rng.normal(0, 4.0 if act == 2 else 1.5, (N, H, W, Cin)).astype(np.float32)
    s = t = None
    if case.xform.startswith("affine"):
        s = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
        t = (rng.uniform(0.3, 0.9, Cin) if case.shift == "positive" else rng.normal(0, 0.5, Cin)).astype(np.float32)
    x, moved = nudge(x, s, t, act)
    return x, s, t, act, moved
