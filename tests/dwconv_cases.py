"""The case table of tests/test_gpu_dwconv.py (depthwise 3x3 convolutions, csrc/dwconv.hip) and what a case needs on the
host: the planner of dwconv.hip (dw_plan, march_ok, resolve_impl, dl3_dwconv3x3_partials) and the row walk of its march
kernels (dw_phase, dw_walk and the arguments each kernel gives dw_walk) restated in Python, the branch each case was written for, and its seeded inputs (the view and the mask nudge are
those of tests/conv3x3_cases.py).  Importable without a GPU: tests/test_dwconv_cases_host.py checks the table here, against
torch, against the mirror and against the text of dwconv.hip."""
from collections import namedtuple

import numpy as np

from oracle import dl3_oracle as O
from tests.conv3x3_cases import MASK_MARGIN, draw_view, nudge, preact, thresholds  # noqa: F401  (shared with the GPU file)

AUTO, GATHER, MARCH = 0, 1, 2   # include/dl3.h DL3_IMPL_*
IMPL_NAME = {AUTO: "auto", GATHER: "gather", MARCH: "march"}

# geom: (N, H, W, C, stride, rate, pad_t, pad_l, Ho, Wo), the arguments of every dl3_dwconv3x3_* launch in front of impl
# impl: the impl argument;  ppb: the DL3_DW_PPB override the case runs under (None: unset)
# xform, act, shift: the input view, as in tests/conv3x3_cases.py
# grad: "bn" = the gradient operand cA*g + cB*yraw + cC, "plain" = g itself (cA == NULL)
# add: backward with dx_add;  stats: with stat_partial (forward) and dstat_partial (backward)
# dx: False = a weight-gradient-only launch (dx == NULL);  sx: through dl3_dwconv3x3_bwd_sx (and, for the bit comparison,
# through dl3_dwconv3x3_bwd as well)
# branch: the paths of dwconv.hip the case is there for (BRANCH below holds the condition of each)
Case = namedtuple("Case", "id geom impl ppb xform act shift grad add stats dx sx branch")


def same(N, H, W, C, stride, rate):
    Ho, pt, _ = O.same_pads(H, 3, stride, rate)
    Wo, pl, _ = O.same_pads(W, 3, stride, rate)
    return (N, H, W, C, stride, rate, pt, pl, Ho, Wo)


def padded(N, H, W, C, stride, rate, pt, pl):
    """explicit symmetric pads (pt, pl) + VALID: ZeroPadding2D in front of the convolution; (0, 0) is plain VALID"""
    keff = 2 * rate + 1
    return (N, H, W, C, stride, rate, pt, pl, (H + 2 * pt - keff) // stride + 1, (W + 2 * pl - keff) // stride + 1)


def _c(id, geom, branch, xform="affine+act", act=None, shift="normal", impl=AUTO, ppb=None, grad="bn", add=True, stats=True,
       dx=True, sx=False):
    if xform.endswith("act") and act is None:
        act = 2
    return Case(id, geom, impl, ppb, xform, act, shift, grad, add, stats, dx, sx, tuple(branch))


# ---- the planner of dwconv.hip, restated ------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def march_ok(g):
    """march_ok(): the geometries the launchers give to the march kernels"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    return stride == 1 and pt == rate and pl == rate and Ho == H and Wo == W


def auto_sized_for_march(g):
    """what dl3_dwconv3x3_partials(DL3_IMPL_AUTO), which is not told the pads, counts march rows for"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    return stride == 1 and Ho == H and Wo == W


def resolve_impl(impl, g):
    """resolve_impl(): the kernel family a launch takes, -1 where DL3_IMPL_MARCH was asked for and cannot be had"""
    if impl == AUTO:
        return MARCH if march_ok(g) else GATHER
    if impl == MARCH and not march_ok(g):
        return -1
    return impl


def auto_mismatch(impl, g):
    """the launch rule added with these tests: DL3_IMPL_AUTO is refused where the launcher would take the gather kernels
    and the caller's buffers hold the march row count"""
    return impl == AUTO and resolve_impl(impl, g) == GATHER and auto_sized_for_march(g)


Plan = namedtuple("Plan", "impl two nslab nxseg nphase Kmax TK nchunk ppb ny PB P")


def dw_plan(g, im, bwd, ppb_env=None):
    """dw_plan() for a resolved impl `im`; ppb_env is the value of DL3_DW_PPB (None: unset)"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    nslab = cdiv(C, 32)
    if im == MARCH:
        two = int(not bwd and 32 % rate == 0 and W >= 32)
        nxseg = cdiv(W, 64 if two else 32)
        nphase = rate if rate < H else H
        Kmax = cdiv(H, rate)
        TK = Kmax
        want = 1024
        while TK > 8 and N * nslab * nxseg * nphase * cdiv(Kmax, TK) < want:
            TK = (TK + 1) // 2
        nchunk = cdiv(Kmax, TK)
        ppb = 1
        if nchunk == 1 and Kmax < 12:
            ppb = 12 // Kmax
            ppb = min(ppb, nphase)
            while ppb > 1 and N * nslab * nxseg * cdiv(nphase, ppb) < 2048:
                ppb -= 1
            if ppb_env is not None:
                ppb = int(ppb_env)
            ppb = max(1, min(ppb, nphase))
        ny = cdiv(nphase, ppb) if ppb > 1 else nphase * nchunk
        return Plan(im, two, nslab, nxseg, nphase, Kmax, TK, nchunk, ppb, ny, 0, N * ny * nxseg)
    NP = N * H * W if bwd else N * Ho * Wo
    PB = min(cdiv(NP, 32), max(1, 4096 // nslab))
    return Plan(im, 0, nslab, 0, 0, 0, 0, 0, 0, 0, PB, PB)


def partials(g, impl, ppb_env=None):
    """dl3_dwconv3x3_partials(): the rows of the partial buffers, the larger of the forward and the backward plan"""
    im = impl
    if im == AUTO:
        im = MARCH if auto_sized_for_march(g) else GATHER
    return max(dw_plan(g, im, False, ppb_env).P, dw_plan(g, im, True, ppb_env).P)


Plans = namedtuple("Plans", "impl fwd bwd Pmax")


def plans(g, impl, ppb_env=None):
    """what a forward and a backward launch of (g, impl) run with: the two plans and the prows both hand their kernels"""
    im = resolve_impl(impl, g)
    assert im in (GATHER, MARCH), "refused: no plan"
    return Plans(im, dw_plan(g, im, False, ppb_env), dw_plan(g, im, True, ppb_env), partials(g, im, ppb_env))


def plan_of(case):
    return plans(case.geom, case.impl, case.ppb)


def fwd_kernel(case):
    p = plan_of(case)
    return "dw_gather_fwd" if p.impl == GATHER else "dw_march2_fwd" if p.fwd.two else "dw_march_fwd"


def s2_dispatch(g):
    """the condition under which dwconv3x3_bwd_impl (behind dw_prepare) launches dw_s2_bwd instead of dw_gather_bwd"""
    return g[4] == 2 and g[5] == 1 and g[6] <= 1 and g[7] <= 1


def bwd_kernel(case):
    if plan_of(case).impl == MARCH:
        return "dw_march_bwd"
    return "dw_s2_bwd" if s2_dispatch(case.geom) else "dw_gather_bwd"


# ---- the row walk of the march kernels (dw_phase, dw_walk), restated ---------------------------------------------------------
ROWS_PER_GROUP = {"dw_march_fwd": 4, "dw_march2_fwd": 3, "dw_march_bwd": 2}   # constexpr int R of each kernel
Walk = namedtuple("Walk", "a ch rows top_halo bot_halo fast tail")


def row_walk(g, kernel, p):
    """per (row phase a, chunk ch) of plan p, as dw_phase decodes them: the rows of the chunk, its halos, the number of
    straight-line groups dw_walk<R> runs in an all-active workgroup (`fast`) and of predicated groups behind them (`tail`; the
    first group is always predicated)"""
    N, H, W, C, stride, r = g[:6]
    R = ROWS_PER_GROUP[kernel]
    out = []
    for a in range(p.nphase):
        Ka = cdiv(H - a, r) if a < H else 0
        for ch in ([0] if p.ppb > 1 else range(p.nchunk)):
            k0 = ch * p.TK
            k1 = min(k0 + p.TK, Ka)
            if k0 >= k1:
                out.append(Walk(a, ch, 0, False, False, 0, 0))
                continue
            bot = k1 < Ka
            ks = k0 - 1 if k0 > 0 else k0
            ke = k1 if bot else k1 - 1
            kg, fast, tail = ks + R, 0, 0
            fast_last = k1 - 1 if kernel == "dw_march_bwd" else ke   # the argument each kernel gives dw_walk
            while kg + R - 1 <= fast_last:
                fast, kg = fast + 1, kg + R
            while kg <= ke:
                tail, kg = tail + 1, kg + R
            out.append(Walk(a, ch, k1 - k0, k0 > 0, bot, fast, tail))
    return out


def full_tiles(g, kernel):
    """workgroup tiles (x segment, channel slab) whose lanes are all inside the tensor: `allact` without the `fast` flag"""
    W, C = g[2], g[3]
    return (W // (64 if kernel == "dw_march2_fwd" else 32)) * (C // 32)


def walk_of(case, kernel):
    p = plan_of(case)
    if p.impl != MARCH or kernel not in (fwd_kernel(case), bwd_kernel(case)):
        return []
    return row_walk(case.geom, kernel, p.bwd if kernel == "dw_march_bwd" else p.fwd)


def fast_groups(case, kernel, ignore_c=False):
    """the straight-line groups `kernel` runs in the case, per all-active tile, summed over phases and chunks; 0 where the
    launchers clear the flag (dw_prepare: C % 32 != 0), no tile is all-active, or the backward has no dx"""
    g = case.geom
    if not ignore_c and (g[3] % 32 != 0 or full_tiles(g, kernel) == 0):
        return 0
    if ignore_c and g[2] // (64 if kernel == "dw_march2_fwd" else 32) == 0:
        return 0
    if kernel == "dw_march_bwd" and not case.dx:
        return 0
    return sum(w.fast for w in walk_of(case, kernel))


def _bwd_fast(sx, add):
    return lambda c: fast_groups(c, "dw_march_bwd") > 0 and c.sx == sx and c.add == add


def _two_pixel_lanes(g):
    """(xa, xb) of every lane of dw_march2_fwd"""
    W, r = g[2], g[5]
    return [(xs * 64 + (pl // r) * 2 * r + pl % r, xs * 64 + (pl // r) * 2 * r + pl % r + r)
            for xs in range(cdiv(W, 64)) for pl in range(32)]


def _loops(case, bwd):
    """a workgroup of the gather kernels makes a second grid-stride iteration"""
    g, p = case.geom, plan_of(case)
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    if p.impl != GATHER:
        return False
    if not bwd:
        return cdiv(N * Ho * Wo, 32) > p.fwd.PB
    if s2_dispatch(g):
        return cdiv(N * ((H + pt + 1) // 2) * ((W + pl + 1) // 2), 32) > p.bwd.PB
    return cdiv(N * H * W, 32) > p.bwd.PB


def _chunks(case, pred):
    """some chunk of some march kernel of the case satisfies pred (a halo exists only in a plan with nchunk > 1)"""
    return any(w.rows and pred(w) for k in ROWS_PER_GROUP for w in walk_of(case, k))


def _dead_rows(g):
    """stride-2 VALID: the last input row and column lie under no tap"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    return (Ho - 1) * stride - pt + 2 * rate < H - 1 and (Wo - 1) * stride - pl + 2 * rate < W - 1


# the condition behind each branch tag of the table, over a case
BRANCH = {
    # the straight-line bodies of the row loops
    "fwd1-fast": lambda c: fast_groups(c, "dw_march_fwd") > 0,
    "fwd2-fast": lambda c: fast_groups(c, "dw_march2_fwd") > 0,
    "bwd-fast-sx-add": _bwd_fast(True, True),
    "bwd-fast-sx-noadd": _bwd_fast(True, False),
    "bwd-fast-nosx-add": _bwd_fast(False, True),
    "bwd-fast-nosx-noadd": _bwd_fast(False, False),
    # the shape would run straight-line groups, C % 32 != 0 keeps the predicated body for the whole chunk
    "fast-off-ragged-c": lambda c: c.geom[3] % 32 != 0 and any(fast_groups(c, k, ignore_c=True) > 0 for k in ROWS_PER_GROUP),
    "fast-then-predicated-tail": lambda c: any(fast_groups(c, k) > 0 and any(w.fast and w.tail for w in walk_of(c, k))
                                               for k in ROWS_PER_GROUP),
    # row chunks of one phase, and the flush of a phase's last row
    "chunked-top-halo": lambda c: _chunks(c, lambda w: w.top_halo),
    "chunked-bottom-halo": lambda c: _chunks(c, lambda w: w.bot_halo),
    "last-row-flush": lambda c: _chunks(c, lambda w: not w.bot_halo and w.top_halo),
    # several row phases per workgroup
    "ppb>1-fwd1": lambda c: fwd_kernel(c) == "dw_march_fwd" and plan_of(c).fwd.ppb > 1,
    "ppb>1-fwd2": lambda c: fwd_kernel(c) == "dw_march2_fwd" and plan_of(c).fwd.ppb > 1,
    "ppb>1-bwd": lambda c: bwd_kernel(c) == "dw_march_bwd" and plan_of(c).bwd.ppb > 1,
    "ppb-uneven-last-group": lambda c: plan_of(c).impl == MARCH and plan_of(c).fwd.ppb > 1
    and plan_of(c).fwd.nphase % plan_of(c).fwd.ppb != 0,
    "rate>H": lambda c: plan_of(c).impl == MARCH and c.geom[5] > c.geom[1],
    "rate32-pair": lambda c: fwd_kernel(c) == "dw_march2_fwd" and c.geom[5] == 32,
    "xb-beyond-W": lambda c: fwd_kernel(c) == "dw_march2_fwd" and any(xa < c.geom[2] <= xb for xa, xb in _two_pixel_lanes(c.geom)),
    "idle-lanes": lambda c: plan_of(c).impl == MARCH and c.geom[2] < 32,
    "Pfwd>Pbwd": lambda c: plan_of(c).fwd.P > plan_of(c).bwd.P,
    "Pbwd>Pfwd": lambda c: plan_of(c).bwd.P > plan_of(c).fwd.P,
    # the gather kernels and dw_s2_bwd
    "gather-loop-fwd": lambda c: _loops(c, False),
    "gather-loop-bwd": lambda c: bwd_kernel(c) == "dw_gather_bwd" and _loops(c, True),
    "s2-loop": lambda c: bwd_kernel(c) == "dw_s2_bwd" and _loops(c, True),
    "gather-bwd-stride2": lambda c: bwd_kernel(c) == "dw_gather_bwd" and c.geom[4] == 2,
    "gather-bwd-stride3": lambda c: bwd_kernel(c) == "dw_gather_bwd" and c.geom[4] == 3,
    # stride 1, Ho == H with pad_t == 0: all the vertical padding lies below the map
    "gather-asym-pad": lambda c: plan_of(c).impl == GATHER and c.geom[4] == 1 and c.geom[6] == 0 and c.geom[8] == c.geom[1],
    "s2-pad10": lambda c: bwd_kernel(c) == "dw_s2_bwd" and c.geom[6:8] == (1, 0),
    "s2-pad01": lambda c: bwd_kernel(c) == "dw_s2_bwd" and c.geom[6:8] == (0, 1),
    "s2-valid-dead-row": lambda c: bwd_kernel(c) == "dw_s2_bwd" and c.geom[6:8] == (0, 0) and _dead_rows(c.geom),
    "s2-3x3": lambda c: bwd_kernel(c) == "dw_s2_bwd" and c.geom[1:3] == (3, 3),
    "s2-ragged-c": lambda c: bwd_kernel(c) == "dw_s2_bwd" and c.geom[3] % 32 != 0,
}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
F1, F1C = same(1, 24, 32, 32, 1, 3), same(1, 48, 40, 64, 1, 3)    # one-pixel forward: rate 3 does not divide 32
B1, B2 = same(1, 12, 32, 32, 1, 1), same(2, 20, 33, 64, 1, 2)     # backward with straight-line groups in two chunks
PP8, PP2 = same(1, 20, 40, 40, 1, 8), same(1, 16, 64, 32, 1, 2)   # two-pixel forward under DL3_DW_PPB
R32 = same(1, 40, 64, 32, 1, 32)

MARCH_CASES = [
    _c("fwd1-fast-r3", F1, ("fwd1-fast", "bwd-fast-nosx-add")),
    _c("fwd1-fast-r3-act-relu", F1, ("fwd1-fast", "bwd-fast-nosx-noadd"), "act", 1, add=False),
    _c("fwd1-fast-r3-two-chunks", F1C, ("fwd1-fast", "bwd-fast-nosx-noadd", "chunked-top-halo", "chunked-bottom-halo",
                                        "last-row-flush", "fast-then-predicated-tail"), "affine", grad="plain", add=False),
    _c("fwd1-fast-r3-two-chunks-relu6", F1C, ("fwd1-fast", "bwd-fast-sx-add", "chunked-top-halo", "chunked-bottom-halo"),
       "affine+act", 2, "positive", sx=True),
    _c("fwd1-ragged-c-r3", same(1, 24, 32, 40, 1, 3), ("fast-off-ragged-c",), "affine+act", 1),
    _c("fwd1-ragged-c-r3-dw-only", same(1, 24, 32, 40, 1, 3), ("fast-off-ragged-c",), "none", grad="plain", add=False,
       stats=False, dx=False),
    _c("bwd-fast-sx-add", B1, ("bwd-fast-sx-add", "chunked-top-halo", "chunked-bottom-halo", "last-row-flush",
                               "fast-then-predicated-tail"), sx=True),
    _c("bwd-fast-sx-noadd", B1, ("bwd-fast-sx-noadd", "chunked-top-halo"), "affine+act", 1, add=False, sx=True),
    _c("bwd-fast-nosx-add", B1, ("bwd-fast-nosx-add",), "act", 2, grad="plain"),
    _c("bwd-fast-nosx-noadd", B1, ("bwd-fast-nosx-noadd",), "affine", add=False, stats=False),
    _c("bwd-fast-dw-only", B1, ("chunked-bottom-halo",), "affine+act", 2, add=False, stats=False, dx=False),
    _c("bwd-fast-r2-sx-noadd", B2, ("bwd-fast-sx-noadd", "Pbwd>Pfwd", "xb-beyond-W"), "affine", add=False, sx=True),
    _c("bwd-fast-r2-sx-add-plain", B2, ("bwd-fast-sx-add", "Pbwd>Pfwd"), "act", 1, grad="plain", sx=True),
    _c("bwd-fast-r2-nosx-add", B2, ("bwd-fast-nosx-add", "last-row-flush"), "affine+act", 2, "positive"),
    _c("ppb3-fwd2-r8", PP8, ("ppb>1-fwd2", "ppb>1-bwd", "ppb-uneven-last-group", "xb-beyond-W"), "affine+act", 1, ppb=3),
    _c("ppb3-fwd2-r8-affine", PP8, ("ppb>1-fwd2", "ppb>1-bwd", "ppb-uneven-last-group"), "affine", ppb=3, grad="plain",
       add=False),
    _c("ppb2-fwd2-fast-r2", PP2, ("ppb>1-fwd2", "fwd2-fast", "ppb>1-bwd", "bwd-fast-nosx-add", "fast-then-predicated-tail"),
       "affine+act", 2, ppb=2),
    _c("ppb2-fwd2-fast-r2-act", PP2, ("ppb>1-fwd2", "fwd2-fast", "bwd-fast-sx-noadd"), "act", 2, ppb=2, add=False, sx=True),
    _c("fwd2-fast-r2-ppb1", PP2, ("fwd2-fast", "Pbwd>Pfwd"), "none"),
    _c("rate32", R32, ("rate32-pair",), "affine+act", 1),
    _c("rate32-ppb5", R32, ("rate32-pair", "ppb>1-fwd2", "ppb>1-bwd", "ppb-uneven-last-group"), "affine", ppb=5),
    _c("rate32-w40", same(1, 34, 40, 36, 1, 32), ("rate32-pair", "xb-beyond-W"), "act", 1, stats=False),
    _c("ppb5-fwd1-r12", same(1, 20, 40, 32, 1, 12), ("ppb>1-fwd1", "ppb>1-bwd", "ppb-uneven-last-group"), "affine+act", 2,
       "positive", ppb=5),
    _c("ppb2-fwd1-r12-dw-only", same(1, 20, 40, 32, 1, 12), ("ppb>1-fwd1", "ppb>1-bwd"), "act", 1, ppb=2, add=False,
       stats=False, dx=False),
    _c("rate-beyond-h", same(1, 8, 8, 16, 1, 12), ("rate>H", "idle-lanes"), "affine"),
    _c("idle-lanes-r2", same(2, 9, 8, 64, 1, 2), ("idle-lanes",), "affine+act", 1, grad="plain", add=False, stats=False),
    _c("pfwd-above-pbwd-r16", same(2, 17, 65, 1376, 1, 16), ("Pfwd>Pbwd", "ppb>1-bwd"), "affine+act", 2),
]

G_S2R2, G_S2P2, G_S3 = same(1, 11, 13, 40, 2, 2), padded(2, 9, 10, 32, 2, 1, 2, 2), same(1, 10, 11, 36, 3, 1)
G_ASYM = (1, 16, 16, 32, 1, 1, 0, 0, 16, 16)         # stride 1, Ho == H, all the padding at the bottom and on the right
G_ASYM_R2 = (2, 9, 12, 40, 1, 2, 0, 4, 9, 12)
GATHER_CASES = [
    _c("gather-loops", padded(1, 33, 64, 2048, 1, 2, 2, 2), ("gather-loop-fwd", "gather-loop-bwd"), "affine+act", 2,
       impl=GATHER),
    _c("gather-bwd-s2-r2", G_S2R2, ("gather-bwd-stride2",), "affine+act", 2, "positive"),
    _c("gather-bwd-s2-r2-affine-dw-only", G_S2R2, ("gather-bwd-stride2",), "affine", grad="plain", add=False, stats=False,
       dx=False),
    _c("gather-bwd-s2-pad2", G_S2P2, ("gather-bwd-stride2",), "act", 1, add=False),
    _c("gather-bwd-s2-pad2-plain", G_S2P2, ("gather-bwd-stride2",), "affine+act", 1, grad="plain", stats=False),
    _c("gather-bwd-s3", G_S3, ("gather-bwd-stride3",), "affine+act", 2),
    _c("gather-bwd-s3-act", G_S3, ("gather-bwd-stride3",), "act", 2, grad="plain", add=False),
    _c("gather-asym-pad", G_ASYM, ("gather-asym-pad",), "affine+act", 1, "positive", impl=GATHER),
    _c("gather-asym-pad-r2", G_ASYM_R2, ("gather-asym-pad",), "affine", impl=GATHER, add=False),
]

S2_CASES = [
    _c("s2-loop", same(1, 91, 91, 2048, 2, 1), ("s2-loop",), "affine+act", 2),
    _c("s2-pad10", same(2, 15, 16, 32, 2, 1), ("s2-pad10",), "affine+act", 2, "positive"),
    _c("s2-pad01", same(2, 16, 15, 32, 2, 1), ("s2-pad01",), "affine+act", 1, "positive"),
    _c("s2-pad10-affine", same(1, 7, 10, 24, 2, 1), ("s2-pad10", "s2-ragged-c"), "affine", add=False),
    _c("s2-pad01-act", same(1, 10, 7, 24, 2, 1), ("s2-pad01", "s2-ragged-c"), "act", 1, grad="plain"),
    _c("s2-valid-dead-row", padded(1, 8, 10, 32, 2, 1, 0, 0), ("s2-valid-dead-row",), "affine+act", 2, "positive"),
    _c("s2-valid-dead-row-ragged-c", padded(2, 6, 8, 40, 2, 1, 0, 0), ("s2-valid-dead-row", "s2-ragged-c"), "act", 2),
    _c("s2-3x3", same(1, 3, 3, 32, 2, 1), ("s2-3x3",), "affine+act", 1),
    _c("s2-3x3-ragged-c-plain", same(2, 3, 3, 20, 2, 1), ("s2-3x3", "s2-ragged-c"), "affine", grad="plain", stats=False),
    _c("s2-ragged-c-noadd", same(2, 15, 15, 40, 2, 1), ("s2-ragged-c",), "affine+act", 2, add=False, stats=False),
    _c("s2-ragged-c-dw-only", same(2, 16, 16, 40, 2, 1), ("s2-ragged-c",), "act", 2, add=False, stats=False, dx=False),
]

CASES = MARCH_CASES + GATHER_CASES + S2_CASES

# the geometries DL3_IMPL_AUTO is refused on (stride 1, Ho == H, Wo == W, pads that are not the rate), next to ones it takes
AUTO_REFUSED = [G_ASYM, G_ASYM_R2, (1, 16, 16, 32, 1, 1, 1, 0, 16, 16), (1, 12, 12, 32, 1, 2, 1, 1, 12, 12)]
AUTO_TAKEN = [B1, padded(1, 16, 16, 32, 1, 1, 0, 0), same(1, 15, 16, 32, 2, 1), padded(1, 14, 14, 32, 1, 1, 2, 2)]


# ---- references ------------------------------------------------------------------------------------------------------------------
def dw_abs_terms(xin, dY, g):
    """sum over (n, oy, ox) of |T(x) at tap (i, j)| * |dY|, [3][3][C] in float64: what the nine sums of the weight gradient
    add up in absolute value (the scale of their rounding error)"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = g
    ax, ag = np.abs(np.asarray(xin, np.float64)), np.abs(np.asarray(dY, np.float64))
    out = np.zeros((3, 3, C))
    for i in range(3):
        for j in range(3):
            sl = O._shifted(ax, Ho, Wo, stride, i * rate - pt, j * rate - pl)
            if sl is not None:
                (oys, oxs), (ys, xs) = sl
                out[i, j] = np.einsum("nhwc,nhwc->c", ax[:, ys, xs, :], ag[:, oys, oxs, :])
    return out
