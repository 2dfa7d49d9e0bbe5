"""-m gpu: the element-wise, BatchNorm-finaliser, resize, tap-gather, subsample, loss-tail and optimizer kernels of
csrc/bn.hip, csrc/misc.hip and csrc/losstail.hip on the paths the engine takes and tests/test_gpu_ops.py does not reach: padded leading
dimensions, column slices, ragged row counts, misaligned pointers, capped grids that loop, ties and clamps.

Every comparison is per element against the float64 restatement in tests/ops_oracle.py with one of its two derived
bounds (assert_elementwise: 2 * roundings * 2**-24 * magnitude; assert_reduction: chain * 2**-24 * sum|terms|); the
count of roundings / the chain length is read off the kernel and justified where it is used.  Every output lives in a
buffer pre-filled with a sentinel: what the contract does not write must still hold it afterwards."""
import math

import numpy as np
import pytest
import torch

from tests import ops_oracle as OO
from tests.gpu_util import call, dev, host, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    return capi.lib()


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for fam in sorted(OO.RATIOS):
        print("\nworst error / bound, %-22s %.3f" % (fam, OO.RATIOS[fam]), end="")
    print()


def _pars(rng, C, lo=0.5, hi=1.5):
    return rng.uniform(lo, hi, C).astype(np.float32), rng.normal(0, 1, C).astype(np.float32)


def _filled(rng, rows, ld, lead=0, sd=1.0):
    """an INPUT buffer [rows][ld] (+ lead, + tail) of random values: what lies outside a slice is finite but arbitrary"""
    return rng.normal(0, sd, lead + rows * ld + OO.GUARD_TAIL).astype(np.float32)


def _step(value):
    return torch.full((1,), value, dtype=torch.int64, device="cuda")


# ======================================================================================================= affine_add
def _affine_add(rng, M, C, lda, ca, ldb, cb, ldo, co, with_b_affine=True, act_a=2, act_b=1):
    a, b = _filled(rng, M, lda, sd=3.0), _filled(rng, M, ldb, sd=3.0)
    (sa, ta), (sb, tb) = _pars(rng, C), _pars(rng, C)
    if not with_b_affine:
        sb = tb = None
    out = dev(OO.guard_buffer(M, ldo))
    call("dl3_affine_add", ptr(dev(a), ca), lda, ptr(dev(sa)), ptr(dev(ta)), act_a, ptr(dev(b), cb), ldb,
         None if sb is None else ptr(dev(sb)), None if tb is None else ptr(dev(tb)), act_b, ptr(out, co), ldo, M, C,
         0.0, 0, None)
    h = host(out)
    idx = OO.region_index(M, ldo, co, C)
    OO.assert_guard(h, idx)
    ref, mag = OO.affine_add(a, lda, ca, sa, ta, act_a, b, ldb, cb, sb, tb, act_b, M, C)
    # longest path: sa*a (1), + ta (2), [the same for b in parallel], a + b (3); the activations are exact
    OO.assert_elementwise(h[idx], ref, mag, 3, "affine_add")
    return h[idx]


def test_affine_add_scalar_kernel_padded_slices(L):
    """affine_add_kernel (the scalar form): C = 37 is no multiple of 4, so the launcher cannot take affine_add4_kernel;
    both operands carry scale, shift and an activation (sb/tb/act_b never ran before); lda/ldb/ldo = 40/44/48 with
    column offsets 3/5/2 into the wider buffers.  70 x 37 = 2590 elements: 11 workgroups, the last one ragged."""
    _affine_add(np.random.default_rng(901), 70, 37, 40, 3, 44, 5, 48, 2)


def test_affine_add_pointer_alignment_fallback_is_bit_identical(L):
    """the same values at C = 40 twice: all pointers 16-byte aligned (affine_add4_kernel) and `a` one float into a row of
    44 (lda % 4 == 0 still, the pointer test of the launcher alone sends it to affine_add_kernel): bit-identical."""
    rng = np.random.default_rng(902)
    M, C, lda, ldb, ldo = 70, 40, 44, 48, 52
    vals = rng.normal(0, 3, (M, C)).astype(np.float32)
    b = _filled(rng, M, ldb, sd=3.0)
    (sa, ta), (sb, tb) = _pars(rng, C), _pars(rng, C)
    outs = []
    for ca in (0, 1):
        a = OO.put(_filled(rng, M, lda), vals, M, lda, ca, C)
        out = dev(OO.guard_buffer(M, ldo))
        call("dl3_affine_add", ptr(dev(a), ca), lda, ptr(dev(sa)), ptr(dev(ta)), 2, ptr(dev(b), 8), ldb, ptr(dev(sb)),
             ptr(dev(tb)), 1, ptr(out, 4), ldo, M, C, 0.0, 0, None)
        h = host(out)
        idx = OO.region_index(M, ldo, 4, C)
        OO.assert_guard(h, idx)
        ref, mag = OO.affine_add(a, lda, ca, sa, ta, 2, b, ldb, 8, sb, tb, 1, M, C)
        OO.assert_elementwise(h[idx], ref, mag, 3, "affine_add")   # roundings: see _affine_add
        outs.append(h[idx])
    assert np.array_equal(outs[0], outs[1])


def test_affine_add_vector_kernel_second_operand_transform(L):
    """affine_add4_kernel with sb/tb/act_b set and padded lds 44/48/52 at aligned column offsets 4/8/4"""
    _affine_add(np.random.default_rng(903), 70, 40, 44, 4, 48, 8, 52, 4)


@pytest.mark.parametrize("M,C,lda,ldb,ldo", [(4100, 257, 260, 257, 259), (4100, 1028, 1032, 1028, 1036)],
                         ids=["scalar", "vector"])
def test_affine_add_grid_stride_loop(L, M, C, lda, ldb, ldo):
    """ew_blocks caps the grid at 4096 workgroups of 256 threads = 1 048 576 work items.  Scalar: 4100 x 257 =
    1 053 700 elements > 1 048 576: second loop iteration.  Vector: 4100 x 1028 / 4 = 1 053 700 float4s: the same."""
    assert M * C // (4 if C % 4 == 0 else 1) > 4096 * 256
    _affine_add(np.random.default_rng(904), M, C, lda, 0, ldb, 0, ldo, 0)


@pytest.mark.parametrize("C", [37, 40], ids=["scalar", "vector"])
def test_affine_add_dropout_mask_with_padded_output(L, C):
    """Dropout at rate 0.5 into ldo = C + 12: the mask is indexed with m*C + c, not with the output's leading dimension;
    the kept set equals the host replica of dl3_uniform and the one dl3_grad_finish draws for the same (M, C, seed,
    step).  1/(1 - 0.5) = 2 and the inputs are ones: the kept values are exactly 2."""
    M, ldo, seed, stp = 70, C + 12, 4321, 3
    ones = np.ones((M, C), np.float32)
    out, gout = dev(OO.guard_buffer(M, ldo)), dev(OO.guard_buffer(M, ldo))
    step = _step(stp)
    call("dl3_affine_add", ptr(dev(ones)), C, None, None, 0, None, 0, None, None, 0, ptr(out, 4), ldo, M, C, 0.5, seed,
         step.data_ptr())
    call("dl3_grad_finish", ptr(dev(ones)), C, 1, 1.0, ptr(gout, 4), ldo, None, 0, None, 0, None, None, 0, None, None,
         None, M, C, 0.5, seed, step.data_ptr())
    idx = OO.region_index(M, ldo, 4, C)
    h, hg = host(out), host(gout)
    OO.assert_guard(h, idx)
    OO.assert_guard(hg, idx)
    keep = OO.keep_mask(seed, M * C, 0.5, stp).reshape(M, C)
    assert np.array_equal(h[idx], np.where(keep, np.float32(2), np.float32(0)))
    assert np.array_equal(hg[idx], h[idx])
    assert not np.array_equal(keep, OO.keep_mask(seed, M * ldo, 0.5, stp).reshape(M, ldo)[:, :C])  # the shape can tell


# ====================================================================================================== grad_finish
def _grad_finish(L, rng, M, C, div=1, rate=0.0, alias=None):
    ldgin, ldgout, ldadd, ldx = C + 3, C + 5, C + 7, C + 9      # all padded, all different
    cg, cgo, cad, cx = 1, 2, 3, 4
    G = (M - 1) // div + 1
    if alias == "gin":
        ldgout, cgo = ldgin, cg
    if alias == "add":
        ldgout, cgo = ldadd, cad
    gin, add, x = _filled(rng, G, ldgin), _filled(rng, M, ldadd), _filled(rng, M, ldx, sd=3.0)
    s, t = _pars(rng, C)
    OO.put(x, OO.unambiguous_mask_input(OO.view(x, M, ldx, cx, C), s, t, 2), M, ldx, cx, C)
    mean, invstd = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    P = L.dl3_rows_partials(M)
    assert P == min(max(M // 64, 1), 512)
    gscale = 1.0 / div if div > 1 else 0.75
    seed, stp = 99, 2
    gd, ad = dev(gin), dev(add)
    if alias == "gin":       # the region holds gin, everything else the sentinel
        gd = dev(OO.put(OO.guard_buffer(M, ldgin), OO.view(gin, M, ldgin, cg, C), M, ldgin, cg, C))
    if alias == "add":
        ad = dev(OO.put(OO.guard_buffer(M, ldadd), OO.view(add, M, ldadd, cad, C), M, ldadd, cad, C))
    out = gd if alias == "gin" else ad if alias == "add" else dev(OO.guard_buffer(M, ldgout))
    step = _step(stp)
    part = dev(OO.guard_buffer(P, 2 * C))
    call("dl3_grad_finish", ptr(gd, cg), ldgin, div, gscale, ptr(out, cgo), ldgout, ptr(ad, cad), ldadd,
         ptr(dev(x), cx), ldx, ptr(dev(s)), ptr(dev(t)), 2, ptr(dev(mean)), ptr(dev(invstd)), ptr(part), M, C, rate,
         seed, step.data_ptr() if rate > 0 else None)
    h, hp = host(out), host(part)
    idx = OO.region_index(M, ldgout, cgo, C)
    OO.assert_guard(h, idx)
    OO.assert_guard(hp, np.arange(P * 2 * C))
    ref, mag, (s1, a1, s2, a2) = OO.grad_finish(gin, ldgin, cg, div, gscale, add, ldadd, cad, x, ldx, cx, s, t, 2, mean,
                                                invstd, M, C, rate, seed, stp)
    # gout: gin_scale * g (1), [* keep_scale (1), keep_scale = 1/(1 - rate) itself (2)], the mask is an exact 0/1,
    # + add (1): 2 roundings without dropout, 5 with
    r = 5 if rate > 0 else 2
    OO.assert_elementwise(h[idx], ref, mag, r, "grad_finish")
    # dstat: a lane (blockIdx.y, row lane) adds rows by*8 + rl + j * 8P, j = 0 .. ceil(M / 8P) - 1, the 8 row lanes
    # of a workgroup are folded in LDS (8 adds), the P partials are folded here in float64.  One term carries the
    # roundings of gout (r) and, for the second sum, x - mean (1), * invstd (1), * gout (1).
    chain = math.ceil(M / (8 * P)) + 8 + r + 3
    pp = hp[:P * 2 * C].astype(np.float64).reshape(P, C, 2)
    OO.assert_reduction(pp[:, :, 0].sum(0), s1, a1, chain, "grad_finish dstat")
    OO.assert_reduction(pp[:, :, 1].sum(0), s2, a2, chain, "grad_finish dstat")


@pytest.mark.parametrize("C", [1, 33])
@pytest.mark.parametrize("M", [1, 7, 63, 65, 203, 33001])
def test_grad_finish_ragged_rows(L, M, C):
    """grad_finish_kernel steps 4 x 8P rows per trip and clamps the rows past M to M-1 and the columns past C to C-1
    (loads only): M < 64 gives P = 1 (M = 1, 7, 63: every trip ragged), 65 and 203 are no multiple of the 32 / 96-row
    step, 33001 > 32768 caps P at 512 (4096 lanes x 4 rows = 16384 rows per trip: three trips, the last one ragged).
    C = 1 and 33 leave 31 clamped column lanes in a workgroup.  relu6 mask with scale / shift, an `add` operand, all
    leading dimensions padded and different, dstat partials per channel."""
    _grad_finish(L, np.random.default_rng(910 + C), M, C)


def test_grad_finish_broadcast_dropout_mask_add(L):
    """gin_div = HW = 29 with gin_scale = 1/HW (backward of the global average pool), Dropout at 0.5, relu6 mask and
    `add` in one launch: M = 7 x 29 = 203 rows read gin row m / 29"""
    _grad_finish(L, np.random.default_rng(920), 203, 33, div=29, rate=0.5)


@pytest.mark.parametrize("alias", ["gin", "add"])
def test_grad_finish_in_place(L, alias):
    """gout == gin (gin_div = 1) and gout == add at the ragged M = 203: every element is read before it is written"""
    _grad_finish(L, np.random.default_rng(921), 203, 33, alias=alias)


# ========================================================================================================== gap_fwd
@pytest.mark.parametrize("N,HW", [(2, 1), (2, 5), (2, 515), (256, 3), (256, 131)])
def test_gap_forms_and_tails(L, N, HW):
    """gap_kernel<32> (1024 threads: N = 2, C = 33 -> 2 x 2 = 4 pairs < 512) walks 16 x 32 = 512 rows per unrolled trip:
    HW = 1 and 5 leave most row lanes without a row, 515 = one unrolled trip + a 3-row tail.  gap_kernel<8> (N = 256:
    2 x 256 = 512 pairs) walks 128 rows per trip: HW = 3, and 131 = one trip + 3.  Reads a column slice (offset 5) of a
    row of C + 11 floats."""
    rng = np.random.default_rng(930)
    C, ldx, cx = 33, 44, 5
    x = _filled(rng, N * HW, ldx, sd=2.0)
    s, t = _pars(rng, C)
    for affine in (True, False):
        out = dev(OO.guard_buffer(N, C))
        call("dl3_gap_fwd", ptr(dev(x), cx), ldx, ptr(dev(s)) if affine else None, ptr(dev(t)) if affine else None, 1,
             ptr(out), N, HW, C, 1.0 / HW)
        h = host(out)
        idx = OO.region_index(N, C, 0, C)
        OO.assert_guard(h, idx)
        ref, mag = OO.gap(x, ldx, cx, s if affine else None, t if affine else None, 1, N, HW, C, 1.0 / HW)
        # the sum runs in double and is rounded to fp32 once: without an affine transform the terms relu(x) are exact
        # and non-negative (magnitude == value), so the result is the float64 one rounded once (2 * 0.5 * 2**-24);
        # with it every term carries s*x (1) and + t (1) before the final rounding (1)
        OO.assert_elementwise(h[idx], ref, mag if affine else np.abs(ref), 3 if affine else 0.5, "gap_fwd")


# ======================================================================================================== subsample
@pytest.mark.parametrize("H,W,stride", [(8, 10, 2), (9, 10, 2), (7, 7, 3), (5, 6, 1), (4, 17, 2)])
def test_subsample_strides_and_slices(L, H, W, stride):
    """y = T(x)[:, ::s, ::s] from a column slice (offset 4 of ld 52) at C = 40: even and odd H at stride 2, stride 3,
    stride 1 (a copy), and W = 17 -> Wo = 9: Wo*C = 360 > 256, an output row spans two workgroups (so does every
    backward row: W*C >= 240, > 256 but for (5, 6, 1)).  The backward is a scatter: bit-exact, 0.0 at every
    non-sampled position including the rows / columns past (Ho-1)*s."""
    rng = np.random.default_rng(940)
    N, C, ldx, cx = 2, 40, 52, 4
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = _filled(rng, N * H * W, ldx, sd=2.0)
    s, t = _pars(rng, C)
    n_out = N * Ho * Wo
    for form in ("none", "act", "affine+act"):
        sc, sh = (s, t) if "affine" in form else (None, None)
        a = 1 if "act" in form else 0
        y = dev(OO.guard_buffer(n_out, C))
        call("dl3_subsample_fwd", ptr(dev(x), cx), ldx, None if sc is None else ptr(dev(sc)),
             None if sh is None else ptr(dev(sh)), a, ptr(y), N, H, W, C, stride, Ho, Wo)
        h = host(y)
        OO.assert_guard(h, np.arange(n_out * C))
        ref, mag = OO.subsample_fwd(x, ldx, cx, sc, sh, a, N, H, W, C, stride, Ho, Wo)
        got = h[:n_out * C].reshape(N, Ho, Wo, C)
        if sc is None:
            assert np.array_equal(got, ref.astype(np.float32))      # a copy (and a clamp)
        else:
            OO.assert_elementwise(got, ref, mag, 2, "subsample")   # s*x (1) + t (1)
    g = rng.normal(0, 1, (N, Ho, Wo, C)).astype(np.float32)
    dx = dev(OO.guard_buffer(N * H * W, C))
    call("dl3_subsample_bwd", ptr(dev(g)), ptr(dx), N, H, W, C, stride, Ho, Wo)
    h = host(dx)
    OO.assert_guard(h, np.arange(N * H * W * C))
    got = h[:N * H * W * C].reshape(N, H, W, C)
    assert np.array_equal(got, OO.subsample_bwd(g, N, H, W, C, stride, Ho, Wo))
    keep = np.zeros((H, W), bool)
    keep[::stride, ::stride] = True
    assert np.all(got[:, ~keep] == 0.0) and not np.signbit(got[:, ~keep]).any()


# ======================================================================================================== conv_taps
@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("same", [True, False], ids=["same", "valid"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_conv_taps(L, k, same, C):
    """dl3_conv_taps_fwd / _bwd (no other test file names them): k x k taps of T(x) side by side, SAME
    (pad = (k-1)//2: k = 2 pads only below / right) and VALID, x read with ldx = C + 5 at column offset 2.  Padding is
    exactly 0.0 whatever the transform (affine with a non-zero shift, with and without relu6); forms without scale /
    shift are gathers: bit-exact.  The backward adds at most k*k terms in a fixed order."""
    rng = np.random.default_rng(950)
    N, H, W, ldx, cx = 2, 5, 7, C + 5, 2
    pad = (k - 1) // 2 if same else 0
    Ho, Wo = (H, W) if same else (H - k + 1, W - k + 1)
    x = _filled(rng, N * H * W, ldx, sd=2.0)
    s, t = _pars(rng, C)
    t = (np.abs(t) + 0.5).astype(np.float32)       # act(shift) != 0: a transformed padding would show
    rows, width = N * Ho * Wo, k * k * C
    cols_none = None
    for sc, sh, a in ((None, None, 0), (s, t, 0), (s, t, 2)):
        cols = dev(OO.guard_buffer(rows, width))
        call("dl3_conv_taps_fwd", ptr(dev(x), cx), ldx, None if sc is None else ptr(dev(sc)),
             None if sh is None else ptr(dev(sh)), a, ptr(cols), N, H, W, C, k, pad, pad, Ho, Wo)
        h = host(cols)
        OO.assert_guard(h, np.arange(rows * width))
        got = h[:rows * width].reshape(rows, width)
        ref, mag = OO.conv_taps_fwd(x, ldx, cx, sc, sh, a, N, H, W, C, k, pad, pad, Ho, Wo)
        outside = mag == 0            # (|s*x| + |t| > 0 everywhere inside the image: t != 0)
        if sc is None:
            outside = OO.conv_taps_fwd(x, ldx, cx, s, t, 0, N, H, W, C, k, pad, pad, Ho, Wo)[1] == 0
            assert np.array_equal(got, ref.astype(np.float32))
            cols_none = got
        else:
            OO.assert_elementwise(got, ref, mag, 2, "conv_taps")   # s*x (1) + t (1)
        assert outside.any() == same          # SAME pads (k = 2: below / right only), VALID does not
        assert np.all(got[outside] == 0.0)
    d = rng.normal(0, 1, (rows, width)).astype(np.float32)
    dx = dev(OO.guard_buffer(N * H * W, C))
    call("dl3_conv_taps_bwd", ptr(dev(d)), ptr(dx), N, H, W, C, k, pad, pad, Ho, Wo)
    h = host(dx)
    OO.assert_guard(h, np.arange(N * H * W * C))
    got = h[:N * H * W * C].reshape(N, H, W, C)
    ref, ab = OO.conv_taps_bwd(d, N, H, W, C, k, pad, pad, Ho, Wo)
    OO.assert_reduction(got, ref, ab, k * k, "conv_taps")          # s += dcols[...] over the k*k taps
    # <cols(x), d> == <x, bwd(d)>, both sides in float64 from the device outputs (cols of the plain form is exact)
    xs = OO.view(x, N * H * W, ldx, cx, C).astype(np.float64).reshape(N, H, W, C)
    lhs = np.sum(cols_none.astype(np.float64) * d)
    rhs = np.sum(xs * got)
    OO.assert_reduction(np.array([rhs]), np.array([lhs]), np.array([np.sum(np.abs(xs) * ab)]), k * k, "conv_taps")


# ================================================================================================== resize_bilinear
# fp32 source coordinates: fl(o * fl(in/out)) floors to the integer BELOW the exact o*in/out at
#   (2, 9, 11, 4, 5, 6): none;  (1, 4, 12, 9, 5, 3): none;  (1, 3, 5, 7, 11, 4): none;
#   (1, 2, 33, 3, 130, 128): none;  (1, 2, 130, 3, 131, 128): none
# (tests/test_ops_oracle_host.py::test_resize_fp32_source_index asserts this list); the oracle takes index and weight
# from the fp32 product either way.
RESIZE_DIMS = [(2, 9, 11, 4, 5, 6), (1, 4, 12, 9, 5, 3), (1, 3, 5, 7, 11, 4)]
RESIZE_FWD_DIMS = RESIZE_DIMS + [(1, 2, 33, 3, 130, 128)]
RESIZE_BWD_DIMS = RESIZE_DIMS + [(1, 2, 130, 3, 131, 128)]


@pytest.mark.parametrize("dims", RESIZE_FWD_DIMS)
def test_resize_fwd_transform_padded_slices(L, dims):
    """resize_fwd_kernel down (9x11 -> 4x5), mixed (4x12 -> 9x5) and by a non-integer factor up (3x5 -> 7x11), with
    affine + relu on load, from columns 3.. of ldx = C + 7 into columns 2.. of ldy = C + 5.  (1, 2, 33, 3, 130, 128):
    Wo*C = 16 640 > 64 workgroups x 256 = 16 384: grid.x is clamped to 64 and the row loop runs a second time."""
    N, Hi, Wi, Ho, Wo, C = dims
    rng = np.random.default_rng(960)
    ldx, cx, ldy, cy = C + 7, 3, C + 5, 2
    x = _filled(rng, N * Hi * Wi, ldx, sd=2.0)
    s, t = _pars(rng, C)
    rows = N * Ho * Wo
    for affine in (True, False):
        y = dev(OO.guard_buffer(rows, ldy))
        call("dl3_resize_bilinear_fwd", ptr(dev(x), cx), ldx, ptr(dev(s)) if affine else None,
             ptr(dev(t)) if affine else None, 1 if affine else 0, ptr(y, cy), ldy, N, Hi, Wi, Ho, Wo, C)
        h = host(y)
        idx = OO.region_index(rows, ldy, cy, C)
        OO.assert_guard(h, idx)
        ref, mag = OO.resize_fwd(x, ldx, cx, s if affine else None, t if affine else None, 1 if affine else 0, N, Hi, Wi,
                                 Ho, Wo, C)
        # s*x (1), + t (2), tr - tl (3), the weight (4), * w (5), + tl (6), bot - top (7), * w (8), + top (9).  The
        # weight: w = f - floor(f) is exact given the fp32 product f = fl(o * scale), which the oracle rounds as TF does;
        # the kernel's compiler contracts o * scale - floor into one FMA (no rounding of f): up to 2**-24 * f apart, an
        # error of the size of the COORDINATE (33 here) — it is in the magnitude (ops_oracle.lerp_slack)
        OO.assert_elementwise(h[idx].reshape(ref.shape), ref, mag, 9 if affine else 7, "resize_fwd")


@pytest.mark.parametrize("dims", RESIZE_BWD_DIMS)
def test_resize_bwd_three_forms(L, dims):
    """resize_bwd_kernel (2-D gather), resize_bwd_x_kernel + resize_bwd_y_kernel (separable, with a workspace) and
    dl3_resize_bilinear_bwd_rows (the y half alone), lddy = C + 6 / lddx = C + 4 at column offsets, accumulate 0 and 1.
    Hi > Ho / Wi > Wo (9x11 <- 4x5, 12 <- 5): the candidate range floor((i-1)/s)-1 .. ceil((i+1)/s)+1 with s > 1 —
    input rows no output row reads must come out 0.  (1, 2, 130, 3, 131, 128): Wi*C = 16 640 > 16 384: the clamped
    grid.x = 64 loops in all three kernels."""
    N, Hi, Wi, Ho, Wo, C = dims
    rng = np.random.default_rng(961)
    lddy, cy, lddx, cxo = C + 6, 1, C + 4, 3
    dy = _filled(rng, N * Ho * Wo, lddy)
    base = rng.normal(0, 1, (N * Hi * Wi, C)).astype(np.float32)
    ref, ab = OO.resize_bwd(dy, lddy, cy, N, Hi, Wi, Ho, Wo, C)
    cx_, cy_ = OO.taps_per_input(Wo, Wi), OO.taps_per_input(Ho, Hi)
    # a weight is the product behind w (1: see test_resize_fwd_transform_padded_slices, its size is in abs_sum), (1 - w)
    # (2), possibly + w (3); wx * dy (4), the inner sum adds cx_ non-zero terms (zeros are exact), wy (3 more),
    # wy * racc (1), cy_ adds: cx_ + cy_ + 8; the separable form rounds the same operations
    chain = cx_ + cy_ + 8
    nb = L.dl3_resize_bilinear_bwd_workspace(N, Hi, Wi, Ho, Wo, C)
    assert nb == N * Ho * Wi * C * 4
    idx = OO.region_index(N * Hi * Wi, lddx, cxo, C)
    got = {}
    for form in ("gather", "separable"):
        for accumulate in (0, 1):
            buf = OO.guard_buffer(N * Hi * Wi, lddx)
            if accumulate:
                OO.put(buf, base, N * Hi * Wi, lddx, cxo, C)
            dx, ws = dev(buf), dev(OO.guard_buffer(nb // 4, 1))
            call("dl3_resize_bilinear_bwd", ptr(dev(dy), cy), lddy, ptr(dx, cxo), lddx, N, Hi, Wi, Ho, Wo, C, accumulate,
                 ptr(ws) if form == "separable" else None, nb if form == "separable" else 0)
            h = host(dx)
            OO.assert_guard(h, idx)
            OO.assert_guard(host(ws), np.arange(nb // 4))
            r = ref + base.reshape(ref.shape) if accumulate else ref
            a = ab + np.abs(base.reshape(ref.shape)) if accumulate else ab
            OO.assert_reduction(h[idx].reshape(ref.shape), r, a, chain + accumulate, "resize_bwd")
            got[form, accumulate] = h[idx].reshape(ref.shape)
    # both within `chain` of the exact value: within 2 * chain of each other
    OO.assert_reduction(got["separable", 0], got["gather", 0].astype(np.float64), ab, 2 * chain, "resize_bwd forms")
    # the y half alone, from an x-folded tensor [N,Ho,Wi,C]
    xf = rng.normal(0, 1, (N, Ho, Wi, C)).astype(np.float32)
    rref, rab = OO.resize_bwd_rows(xf, Hi, Ho)
    for accumulate in (0, 1):
        buf = OO.guard_buffer(N * Hi * Wi, lddx)
        if accumulate:
            OO.put(buf, base, N * Hi * Wi, lddx, cxo, C)
        dx = dev(buf)
        call("dl3_resize_bilinear_bwd_rows", ptr(dev(xf)), ptr(dx, cxo), lddx, N, Hi, Wi, Ho, C, accumulate)
        h = host(dx)
        OO.assert_guard(h, idx)
        r = rref + base.reshape(rref.shape) if accumulate else rref
        a = rab + np.abs(base.reshape(rref.shape)) if accumulate else rab
        OO.assert_reduction(h[idx].reshape(rref.shape), r, a, cy_ + 4 + accumulate, "resize_bwd")   # wy (3), * (1), adds


# =========================================================================== softmax / argmax / count / softmax_xent
@pytest.mark.parametrize("C", [1, 2, 21, 40])
def test_argmax_ties_first_maximum_wins(L, C):
    """argmax_kernel on ties (continuous random data never has one): constant rows, the maximum duplicated at (first,
    last), (middle, last) and everywhere, +0.0 against -0.0 (equal: the first wins) — against np.argmax"""
    rng = np.random.default_rng(970)
    rows = []
    base = rng.normal(0, 1, C).astype(np.float32)
    top = np.float32(base.max() + 1)
    rows.append(np.full(C, 1.5, np.float32))
    rows.append(np.zeros(C, np.float32))
    for pos in ((0, C - 1), (C // 2, C - 1), tuple(range(C))):
        r = base.copy()
        r[list(pos)] = top
        rows.append(r)
    for first in (0.0, -0.0):
        r = np.full(C, -1.0, np.float32)
        r[C - 1] = -first
        r[C // 2] = first
        rows.append(r)
    r = np.full(C, -0.0, np.float32)
    r[C - 1] = 0.0
    rows.append(r)
    x = np.stack(rows)
    M = x.shape[0]
    out = torch.full((M + 8,), -77, dtype=torch.int32, device="cuda")
    call("dl3_argmax", ptr(dev(x)), out.data_ptr(), M, C)
    h = host(out)
    assert np.array_equal(h[:M], OO.argmax_first(x)) and np.all(h[M:] == -77)
    if C > 1:
        assert not np.array_equal(OO.argmax_first(x), OO.argmax_first(x, bug="last_max"))


@pytest.mark.parametrize("M", [1048576 + 300, 2097152 + 300])
def test_softmax_argmax_grid_stride_loop(L, M):
    """softmax_kernel / argmax_kernel, one row per thread behind ew_blocks.  The element-wise launches of csrc/bn.hip
    cap at 4096 workgroups: M = 1 048 876 rows > 4096 x 256 would loop there; csrc/misc.hip's own ew_blocks caps at
    8192, so here it takes M = 2 097 452 rows > 8192 x 256 = 2 097 152: second loop iteration for the last 300 rows
    (the first M runs 4098 workgroups, past the 4096 of the other file).  C = 2; every 7th row is a tie."""
    rng = np.random.default_rng(971)
    C = 2
    x = rng.normal(0, 3, (M, C)).astype(np.float32)
    x[::7, 1] = x[::7, 0]
    p = dev(OO.guard_buffer(M, C))
    xd = dev(x)
    call("dl3_softmax_fwd", ptr(xd), ptr(p), M, C)
    h = host(p)
    OO.assert_guard(h, np.arange(M * C))
    ref, mag, _ = OO.softmax_rows(x)
    # x - max (1, scaled by |x - max|: in the magnitude), expf (2: 1 ulp), the sum of C terms (C, each term carrying
    # the 3 above), 1 / s (1), * inv (1): C + 8
    OO.assert_elementwise(h[:M * C].reshape(M, C), ref, mag, C + 8, "softmax")
    am = torch.full((M + 8,), -77, dtype=torch.int32, device="cuda")
    call("dl3_argmax", ptr(xd), am.data_ptr(), M, C)
    ha = host(am)
    assert np.array_equal(ha[:M], OO.argmax_first(x)) and np.all(ha[M:] == -77)


def _loss_chain(M, P, C):
    """a thread adds ceil(M / 256P) row losses, 6 butterfly adds fold a wave, 3 adds fold the 4 waves; the P partials
    are folded in float64 here.  One term: the probability q = p_t / sum p (C + 8 for p_t, C more for the sum of the C
    probabilities, 1 for the division), logf (2), * w (1), * inv_nnz (1), inv_nnz = 1 / nnz (1): 2C + 14"""
    return math.ceil(M / (256 * P)) + 6 + 3 + 2 * C + 14


@pytest.mark.parametrize("variant", ["all", "no_weights", "no_probs", "no_dlogits"])
@pytest.mark.parametrize("M,C", [(33007, 1), (33007, 2), (33007, 32), (33007, 33), (131072 + 77, 2)])
def test_softmax_xent_kernel_switch_and_capped_partials(L, M, C, variant):
    """dl3_softmax_xent: C = 32 is the last width of row_kernel, C = 33 the first of softmax_xent_kernel, C = 1 and 2
    the narrowest rows of the LDS transpose.  M = 33 007 > 32 768 caps dl3_rows_partials at P = 512 (515 without the
    cap; the last workgroup's tile is ragged: 33007 = 128 x 256 + 239); M = 131 149 > 512 x 256 = 131 072 makes the
    row loop of both kernels run a second time.  weights == NULL (every valid row weighs 1), probs == NULL with
    dlogits and the reverse.  Rows 0..19 leave Keras' clip interval on either side (no gradient, constant loss)."""
    rng = np.random.default_rng(972)
    x, labels, w = OO.xent_inputs(rng, M, C, void_w=True)
    if variant == "no_weights":
        w = None
    nnz_v = float(M if w is None else (w != 0).sum())
    P = L.dl3_rows_partials(M)
    assert P == 512
    nnz = dev(np.array([nnz_v], np.float32))
    probs = dev(OO.guard_buffer(M, C)) if variant != "no_probs" else None
    dl = dev(OO.guard_buffer(M, C)) if variant != "no_dlogits" else None
    lp = dev(OO.guard_buffer(P, 1))
    call("dl3_softmax_xent", ptr(dev(x)), ptr(dev(labels)), None if w is None else ptr(dev(w)), ptr(nnz), ptr(probs),
         ptr(dl), ptr(lp), M, C)
    r = OO.softmax_xent(x, labels, w, nnz_v)
    if probs is not None:
        h = host(probs)
        OO.assert_guard(h, np.arange(M * C))
        OO.assert_elementwise(h[:M * C].reshape(M, C), r["p"], r["pmag"], C + 8, "softmax_xent")   # as softmax_kernel
    if dl is not None:
        h = host(dl)
        OO.assert_guard(h, np.arange(M * C))
        got = h[:M * C].reshape(M, C)
        # p (C + 8), p - onehot (1), gs = w * inv_nnz (1), inv_nnz = 1 / nnz (1), * gs (1): C + 12
        OO.assert_elementwise(got, r["dl"], r["dlmag"], C + 12, "softmax_xent")
        assert np.all(got[:20] == 0) and np.all(r["dl"][:20] == 0)
        assert np.all(got[labels.astype(np.int64) >= C] == 0)          # void rows, whatever their weight
    h = host(lp)
    OO.assert_guard(h, np.arange(P))
    OO.assert_reduction(np.array([h[:P].astype(np.float64).sum()]), np.array([r["l"].sum()]),
                        np.array([r["lmag"].sum()]), _loss_chain(M, P, C), "loss")


@pytest.mark.parametrize("C", [2, 33])
def test_softmax_xent_all_void_batch(L, C):
    """every label void, every weight 0, nnz = 0: 1 / max(nnz, DL3_NNZ_FLOOR) = 1e20 meets w = 0 — loss partials and
    gradient are exactly 0.0 and nothing is inf or nan (both kernels)"""
    rng = np.random.default_rng(973)
    M = 1000
    x = rng.normal(0, 3, (M, C)).astype(np.float32)
    labels, w = np.full(M, C, np.float32), np.zeros(M, np.float32)
    P = L.dl3_rows_partials(M)
    probs, dl, lp = dev(OO.guard_buffer(M, C)), dev(OO.guard_buffer(M, C)), dev(OO.guard_buffer(P, 1))
    call("dl3_softmax_xent", ptr(dev(x)), ptr(dev(labels)), ptr(dev(w)), ptr(dev(np.zeros(1, np.float32))), ptr(probs),
         ptr(dl), ptr(lp), M, C)
    hp, hd, hl = host(probs), host(dl), host(lp)
    for h, n in ((hp, M * C), (hd, M * C), (hl, P)):
        OO.assert_guard(h, np.arange(n))
        assert np.isfinite(h[:n]).all()
    assert np.all(hd[:M * C] == 0.0) and np.all(hl[:P] == 0.0)
    r = OO.softmax_xent(x, labels, w, 0.0)
    OO.assert_elementwise(hp[:M * C].reshape(M, C), r["p"], r["pmag"], C + 8, "softmax_xent")


def test_count_nonzero_signed_zero_denormal_single(L):
    """count_nz_kernel: -0.0 is zero, a denormal weight is not; M = 1; a count past one workgroup's share"""
    w = np.array([0.0, -0.0, 1e-42, -1e-45, 2.0, 0.0, -3.0], np.float32)
    assert (w != 0).sum() == 4
    for arr in (w, np.array([1e-42], np.float32), np.array([-0.0], np.float32), np.tile(w, 70000)):
        out = dev(OO.guard_buffer(1, 1))
        call("dl3_count_nonzero", ptr(dev(arr)), arr.size, ptr(out))
        h = host(out)
        OO.assert_guard(h, np.arange(1))
        assert h[0] == float((arr != 0).sum())


# ================================================================================== upsample_softmax_xent / _fold
def _upsample_case(rng, dims):
    N, Hi, Wi, Ho, Wo, C = dims
    M = N * Ho * Wo
    lo = rng.normal(0, 2, (N, Hi, Wi, C)).astype(np.float32)
    labels = rng.integers(0, C + 1, M).astype(np.float32)
    up, zmag = OO.resize_fwd(lo, C, 0, None, None, 0, N, Hi, Wi, Ho, Wo, C)
    amb = OO.clip_ambiguous_rows(up.reshape(M, C), labels)
    labels[amb] = C
    w = rng.uniform(0.5, 2, M).astype(np.float32)
    return lo, labels, w, up.reshape(M, C), zmag.reshape(M, C)


def test_upsample_softmax_xent_capped_partials(L):
    """row_kernel<XentTerm, UPSAMPLE> at (3, 3, 5, 110, 101, 4): M = 33 330 output pixels > 32 768: P = 512 (capped), the last
    workgroup's tile ragged (33330 = 130 x 256 + 50); a non-integer factor both ways"""
    dims = (3, 3, 5, 110, 101, 4)
    N, Hi, Wi, Ho, Wo, C = dims
    rng = np.random.default_rng(980)
    lo, labels, w, up, zmag = _upsample_case(rng, dims)
    M = N * Ho * Wo
    P = L.dl3_rows_partials(M)
    assert P == 512
    nnz_v = float((w != 0).sum())
    probs, dl, lp = dev(OO.guard_buffer(M, C)), dev(OO.guard_buffer(M, C)), dev(OO.guard_buffer(P, 1))
    call("dl3_upsample_softmax_xent", ptr(dev(lo)), ptr(dev(labels)), ptr(dev(w)), ptr(dev(np.array([nnz_v], np.float32))),
         ptr(probs), ptr(dl), ptr(lp), N, Hi, Wi, Ho, Wo, C)
    # the interpolated logit carries 6 roundings of its magnitude (resize_fwd without transform): an absolute error in
    # the exponent, i.e. a relative one in the probability — it enters the magnitude, the counts stay those of
    # dl3_softmax_xent
    r = OO.softmax_xent(up, labels, w, nnz_v, zmag=6 * zmag)
    for buf, key, rd in ((probs, "p", C + 8), (dl, "dl", C + 12)):
        h = host(buf)
        OO.assert_guard(h, np.arange(M * C))
        OO.assert_elementwise(h[:M * C].reshape(M, C), r[key], r[key + "mag"], rd, "upsample_xent")
    h = host(lp)
    OO.assert_guard(h, np.arange(P))
    OO.assert_reduction(np.array([h[:P].astype(np.float64).sum()]), np.array([r["l"].sum()]),
                        np.array([r["lmag"].sum()]), _loss_chain(M, P, C), "loss")


@pytest.mark.parametrize("dims", [(70, 2, 2, 60, 4, 3), (3, 3, 5, 110, 101, 4)])
def test_upsample_softmax_xent_fold_capped_rows(L, dims):
    """fold_kernel<XentTerm, ..>: one workgroup per output row behind dl3_xent_fold_partials' cap of 4096.  (70, 2, 2, 60, 4,
    3): N*Ho = 4200 rows > 4096: rows 4096..4199 are second trips of workgroups 0..103.  (3, 3, 5, 110, 101, 4): 330
    rows, one each.  The first takes the form without prefetch (Wi*C = 6 is no multiple of 4), the second the
    prefetching one (Wi*C = 20, Wo*C = 404: whole float4s; 101 pixels: one per thread, the second slot idle)."""
    N, Hi, Wi, Ho, Wo, C = dims
    rng = np.random.default_rng(981)
    lo, labels, w, up, zmag = _upsample_case(rng, dims)
    M = N * Ho * Wo
    P = L.dl3_xent_fold_partials(N, Ho)
    assert P == min(N * Ho, 4096)
    nnz_v = float((w != 0).sum())
    xfold, lp = dev(OO.guard_buffer(N * Ho * Wi, C)), dev(OO.guard_buffer(P, 1))
    call("dl3_upsample_softmax_xent_fold", ptr(dev(lo)), ptr(dev(labels)), ptr(dev(w)),
         ptr(dev(np.array([nnz_v], np.float32))), ptr(xfold), ptr(lp), N, Hi, Wi, Ho, Wo, C)
    # magnitudes as in test_upsample_softmax_xent_capped_partials, doubled: this kernel's __expf = exp2(x * log2 e) rounds
    # the product once more in proportion to |x - max| (1 + 2D <= 2 (1 + D))
    r = OO.softmax_xent(up, labels, w, nnz_v, zmag=6 * zmag)
    A2 = 2.0
    ref, _ = OO.resize_bwd_cols(r["dl"].reshape(N, Ho, Wo, C), Wi, Wo)
    _, ab = OO.resize_bwd_cols(A2 * r["dlmag"].reshape(N, Ho, Wo, C), Wi, Wo)
    h = host(xfold)
    OO.assert_guard(h, np.arange(N * Ho * Wi * C))
    # one term: dlogits (C + 12), the weight (3: see test_resize_bwd_three_forms), * (1); the fold adds taps_per_input terms
    OO.assert_reduction(h[:N * Ho * Wi * C].reshape(ref.shape), ref, ab, C + 16 + OO.taps_per_input(Wo, Wi), "xent_fold")
    h = host(lp)
    OO.assert_guard(h, np.arange(P))
    # a workgroup's thread adds ceil(Wo / 256) pixels per row and ceil(N*Ho / P) rows
    chain = math.ceil(Wo / 256) * math.ceil(N * Ho / P) + 6 + 3 + 2 * C + 14
    OO.assert_reduction(np.array([h[:P].astype(np.float64).sum()]), np.array([r["l"].sum()]),
                        np.array([A2 * r["lmag"].sum()]), chain, "loss")


# ============================================================================================ adam / fill / scale
ADAM = dict(lr_t=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _adam_call(name, n, p, g, m, v, gs, denom=None):
    bufs = []
    for a in (p, m, v):
        b = OO.guard_buffer(n, 1)
        b[:n] = a
        bufs.append(dev(b))
    args = [ptr(bufs[0]), ptr(dev(g)), ptr(bufs[1]), ptr(bufs[2]), n, ADAM["lr_t"], ADAM["b1"], ADAM["b2"], ADAM["eps"], gs]
    if denom is not None:
        args.append(ptr(dev(np.array([denom], np.float32))))
    call(name, *args)
    outs = []
    for b in bufs:
        h = host(b)
        OO.assert_guard(h, np.arange(n))
        outs.append(h[:n])
    return outs


def _adam_inputs(n, zero_g=False):
    rng = np.random.default_rng(990)
    p, g = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    m, v = rng.normal(0, 0.1, n).astype(np.float32), rng.uniform(0, 0.1, n).astype(np.float32)
    return p, (np.zeros(n, np.float32) if zero_g else g), m, v


@pytest.mark.parametrize("n", [1, 1048576 + 777])
def test_adam_step_grid_stride_loop(L, n):
    """adam_kernel at n = 1 (one live lane) and n = 1 049 353 > 4096 x 256 = 1 048 576: the last 777 elements are second
    loop iterations; guard band after element n on p, m and v"""
    p, g, m, v = _adam_inputs(n)
    got = _adam_call("dl3_adam_step", n, p, g, m, v, 0.5)
    ref, mag = OO.adam(p, g, m, v, gs=0.5, **ADAM)
    # m: g*gs (1), 1 - b1 (1), * (1), + b1*m (1): 4.  v: gi twice (2), 1 - b2 (1), two products (2), + (1): 6.
    # p: m (4), the denominator (v 6 halved by the root: 3, sqrtf 1, + eps 1), lr * m (1), / (1), p - u (1): 12
    for o, r_, mg, rd in zip(got, ref, mag, (12, 4, 6)):
        OO.assert_elementwise(o, r_, mg, rd, "adam")


@pytest.mark.parametrize("n", [1, 1048576 + 777])
@pytest.mark.parametrize("denom", [1234.0, 0.5, 0.0])
def test_adam_step_norm_denominator_and_floor(L, n, denom):
    """adam_norm_kernel (named by no other test): the gradient scale gs / max(denom[0], 1e-20) finished on the device;
    denom = 0 takes the floor (scale 5e19; g = 0 keeps the step finite).  Against float64 Adam and against dl3_adam_step
    handed the same scale precomputed in fp32; n as in test_adam_step_grid_stride_loop"""
    p, g, m, v = _adam_inputs(n, zero_g=denom == 0.0)
    gs = 0.5
    got = _adam_call("dl3_adam_step_norm", n, p, g, m, v, gs, denom)
    ref, mag = OO.adam(p, g, m, v, gs=gs, denom=denom, **ADAM)
    sc32 = float(np.float32(gs) / np.maximum(np.float32(denom), np.float32(1e-20)))
    plain = _adam_call("dl3_adam_step", n, p, g, m, v, sc32)
    # the scale is one more rounding on every use of the gradient: m 5, v 8, p 5 + (4 + 2) + 2 + 1 = 14
    for o, pl, r_, mg, rd in zip(got, plain, ref, mag, (14, 5, 8)):
        assert np.isfinite(o).all()
        OO.assert_elementwise(o, r_, mg, rd, "adam")
        OO.assert_elementwise(o, pl.astype(np.float64), mg, rd, "adam")


@pytest.mark.parametrize("n", [1, 1048576 + 777])
def test_fill_scale_grid_stride_loop(L, n):
    """fill_kernel and scale_kernel (dl3_scale is named by no other test) at n = 1 and n = 1 049 353 > 4096 x 256:
    bit-exact (a store; a single multiply), guard band after element n"""
    rng = np.random.default_rng(991)
    buf = dev(OO.guard_buffer(n, 1))
    call("dl3_fill", ptr(buf), 2.5, n)
    h = host(buf)
    OO.assert_guard(h, np.arange(n))
    assert np.all(h[:n] == np.float32(2.5))
    x = rng.normal(0, 1, n).astype(np.float32)
    b = OO.guard_buffer(n, 1)
    b[:n] = x
    buf = dev(b)
    call("dl3_scale", ptr(buf), 0.3, n)
    h = host(buf)
    OO.assert_guard(h, np.arange(n))
    assert np.array_equal(h[:n], x * np.float32(0.3))


# ================================================================================== bn_finalize / bn_bwd_finalize
@pytest.mark.parametrize("P", [1, 33])
def test_bn_finalize_ragged_channel_block_and_variance_clamp(L, P):
    """bn_finalize_kernel / bn_bwd_finalize_kernel fold 8 channels per workgroup: C = 21 leaves 3 lanes of the third
    workgroup without a channel (cok == false: clamped loads, no store); partial rows of ldc = 40 read from channel
    c0 = 8; P = 1 (31 of 32 row lanes idle) and 33 (the second unrolled slot of row lane 0's first trip: a trip covers
    8 x 32 rows, test_bn_finalize_folds_every_partial_row has the second trip).  Channel 5 holds the fp32 sums of a
    constant tensor whose s2/n - mean^2 is negative in float64: the clamp gives invstd = 1/sqrt(eps), finite scale /
    shift, and moving_var moves toward 0."""
    rng = np.random.default_rng(995)
    ldc, C, c0 = 40, 21, 8
    s1n, s2n, n = OO.negative_variance_sums()
    count = float(n)
    assert s2n / count - (s1n / count) ** 2 < 0
    part = rng.normal(0, 1, (P, ldc, 2)).astype(np.float32)
    part[:, :, 1] = np.abs(part[:, :, 1]) * 40 + 30
    part[:, c0 + 5] = 0
    part[0, c0 + 5] = (s1n, s2n)
    gamma, beta = _pars(rng, C)
    mm, mv = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    eps, mom = 1e-3, 0.99
    unb = count / (count - 1) * count / (count - (1 + eps))
    names = ("scale", "shift", "mean", "invstd", "mmean", "mvar")
    bufs = [OO.guard_buffer(C, 1) for _ in names]
    bufs[4][:C], bufs[5][:C] = mm, mv
    d = [dev(b) for b in bufs]
    call("dl3_bn_finalize", ptr(dev(part), 2 * c0), P, ldc, C, count, ptr(dev(gamma)), ptr(dev(beta)), eps, mom, unb,
         *[ptr(b) for b in d])
    ref = OO.bn_finalize(part, P, ldc, c0, C, count, gamma, beta, eps, mom, unb, mm, mv)
    got = {}
    for name, b in zip(names, d):
        h = host(b)
        OO.assert_guard(h, np.arange(C))
        got[name] = h[:C]
        # the kernel folds and finishes in double: ONE fp32 rounding of the float64 value (relative, per channel)
        OO.assert_elementwise(h[:C], ref[name], np.abs(ref[name]), 1, "bn_finalize")
    assert abs(got["invstd"][5] - 1 / math.sqrt(float(np.float32(eps)))) <= OO.U * 2 / math.sqrt(eps)
    assert np.isfinite(got["scale"]).all() and np.isfinite(got["shift"]).all()
    assert abs(got["mvar"][5]) < abs(mv[5]) and abs(got["mvar"][5] - float(np.float32(mom)) * mv[5]) <= 2 * OO.U * mv[5]
    # backward finaliser on the same geometry, both modes
    dpart = rng.normal(0, 1, (P, ldc, 2)).astype(np.float32)
    mean, invstd = got["mean"], got["invstd"]
    for mode in (1, 0):
        co = [dev(OO.guard_buffer(C, 1)) for _ in range(5)]
        call("dl3_bn_bwd_finalize", ptr(dev(dpart), 2 * c0), P, ldc, C, count, ptr(dev(gamma)), ptr(dev(mean)),
             ptr(dev(invstd)), mode, *[ptr(o) for o in co])
        rb = OO.bn_bwd_finalize(dpart, P, ldc, c0, C, count, gamma, mean, invstd, mode)
        for name, o in zip(("cA", "cB", "cC", "dgamma", "dbeta"), co):
            h = host(o)
            OO.assert_guard(h, np.arange(C))
            OO.assert_elementwise(h[:C], rb[name], np.abs(rb[name]), 1, "bn_bwd_finalize")   # one rounding, as above


@pytest.mark.parametrize("P", [256, 257, 1250])
def test_bn_finalize_folds_every_partial_row(L, P):
    """fold2 adds FOLD_U x 32 = 256 partial rows per trip: P = 256 fills the first trip exactly, 257 starts the second with one
    row (row lane 0 alone), 1 250 is the largest count dl3_pwconv_partials returns (32 -> 172 at 40 000 rows: five trips, the
    last one ragged in every unrolled slot).  The partial rows are integers, so their float64 fold is exact in any order and
    the outputs are ONE fp32 rounding of the float64 expression; a row added twice or left out moves every sum by percent."""
    rng = np.random.default_rng(996 + P)
    C, count = 21, 40000.0
    if P == 1250:
        assert L.dl3_pwconv_partials(40000, 32, 172) == 1250
    part = np.empty((P, C, 2), np.float32)
    part[:, :, 0] = rng.integers(-9, 10, (P, C)) + np.arange(P)[:, None] % 7     # every row differs from its neighbours
    part[:, :, 1] = rng.integers(40, 120, (P, C)) + np.arange(P)[:, None] % 5
    gamma, beta = _pars(rng, C)
    mm, mv = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    eps, mom = 1e-3, 0.99
    unb = count / (count - 1) * count / (count - (1 + eps))
    names = ("scale", "shift", "mean", "invstd", "mmean", "mvar")
    bufs = [OO.guard_buffer(C, 1) for _ in names]
    bufs[4][:C], bufs[5][:C] = mm, mv
    d = [dev(b) for b in bufs]
    call("dl3_bn_finalize", ptr(dev(part)), P, C, C, count, ptr(dev(gamma)), ptr(dev(beta)), eps, mom, unb, *[ptr(b) for b in d])
    ref = OO.bn_finalize(part, P, C, 0, C, count, gamma, beta, eps, mom, unb, mm, mv)
    assert (part[:, :, 1].astype(np.float64).sum(0) / count - ref["mean"] ** 2 > 0.01).all()   # (far from the variance clamp)
    scale64 = ref["scale"]
    mags = dict(scale=np.abs(scale64), shift=np.abs(beta.astype(np.float64)) + np.abs(ref["mean"] * scale64), mean=np.abs(ref["mean"]),
                invstd=np.abs(ref["invstd"]), mmean=np.abs(ref["mmean"]), mvar=np.abs(ref["mvar"]))
    for name, b in zip(names, d):
        h = host(b)
        OO.assert_guard(h, np.arange(C))
        OO.assert_elementwise(h[:C], ref[name], mags[name], 1, "bn_finalize")
    dpart = np.empty((P, C, 2), np.float32)
    dpart[:, :, 0] = rng.integers(-9, 10, (P, C)) + np.arange(P)[:, None] % 7
    dpart[:, :, 1] = rng.integers(-20, 21, (P, C)) + np.arange(P)[:, None] % 3
    mean, invstd = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    for mode in (1, 0):
        co = [dev(OO.guard_buffer(C, 1)) for _ in range(5)]
        call("dl3_bn_bwd_finalize", ptr(dev(dpart)), P, C, C, count, ptr(dev(gamma)), ptr(dev(mean)), ptr(dev(invstd)), mode,
             *[ptr(o) for o in co])
        rb = OO.bn_bwd_finalize(dpart, P, C, 0, C, count, gamma, mean, invstd, mode)
        mag = {k: np.abs(v) for k, v in rb.items()}
        # cC = -a * s1 / n - b * mean: two terms that may cancel
        mag["cC"] = np.abs(rb["cA"] * rb["dbeta"] / count) + np.abs(rb["cB"] * mean.astype(np.float64))
        for name, o in zip(("cA", "cB", "cC", "dgamma", "dbeta"), co):
            h = host(o)
            OO.assert_guard(h, np.arange(C))
            OO.assert_elementwise(h[:C], rb[name], mag[name], 1, "bn_bwd_finalize")
        # the folded sums themselves are integers: exact
        assert np.array_equal(host(co[3])[:C], dpart[:, :, 1].astype(np.float64).sum(0))
        assert np.array_equal(host(co[4])[:C], dpart[:, :, 0].astype(np.float64).sum(0))


@pytest.mark.parametrize("with_stats", [True, False], ids=["mean-invstd", "null-mean-invstd"])
@pytest.mark.parametrize("C", [21, 257])
def test_bn_frozen_centered(L, C, with_stats):
    """dl3_bn_frozen_centered, the frozen BatchNorm whose producer subtracts the mean: scale = gamma / sqrt(var + eps) and invstd
    at ONE fp32 rounding of the float64 value (the kernel evaluates them in double), shift = beta, neg_mean = -moving_mean and
    mean = 0 bit for bit; C = 21 (one ragged workgroup) and 257 (a second workgroup with one channel); mean / invstd NULL"""
    rng = np.random.default_rng(997 + C)
    gamma, beta = _pars(rng, C)
    mm = (rng.normal(0, 30, C)).astype(np.float32)        # |mean| >> sigma is what the centred form is for
    mm[0] = 0.0                                           # (-0.0 is the negation of 0.0)
    mv = rng.uniform(1e-4, 4, C).astype(np.float32)
    eps = 1e-3
    names = ("scale", "shift", "mean", "invstd", "neg_mean")
    d = {n: dev(OO.guard_buffer(C, 1)) for n in names}
    call("dl3_bn_frozen_centered", ptr(dev(gamma)), ptr(dev(beta)), ptr(dev(mm)), ptr(dev(mv)), eps, C, ptr(d["scale"]),
         ptr(d["shift"]), ptr(d["mean"]) if with_stats else None, ptr(d["invstd"]) if with_stats else None, ptr(d["neg_mean"]))
    inv64 = 1.0 / np.sqrt(mv.astype(np.float64) + float(np.float32(eps)))
    h = {n: host(b) for n, b in d.items()}
    for n in names:
        OO.assert_guard(h[n], np.arange(C) if (with_stats or n not in ("mean", "invstd")) else np.arange(0))
    OO.assert_elementwise(h["scale"][:C], gamma * inv64, np.abs(gamma * inv64), 1, "bn_frozen_centered")
    assert np.array_equal(h["shift"][:C].view(np.uint32), beta.view(np.uint32))
    assert np.array_equal(h["neg_mean"][:C].view(np.uint32), (-mm).view(np.uint32))
    if with_stats:
        OO.assert_elementwise(h["invstd"][:C], inv64, inv64, 1, "bn_frozen_centered")
        assert np.array_equal(h["mean"][:C].view(np.uint32), np.zeros(C, np.uint32))
