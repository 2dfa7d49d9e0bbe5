"""CPU: the bounds of tests/ops_oracle.py discriminate.  For each family of tests/test_gpu_ops_edges.py (same shapes,
same seeds) the comparison helper is handed a deliberately wrong oracle variant in place of device output and must
reject it, and — where the oracle can be evaluated in float32 — that host emulation of the kernel's arithmetic in place
of device output and must accept it."""
import math

import numpy as np
import pytest

from tests import ops_oracle as OO


def _pars(rng, C, lo=0.5, hi=1.5):
    return rng.uniform(lo, hi, C).astype(np.float32), rng.normal(0, 1, C).astype(np.float32)


def _filled(rng, rows, ld, lead=0, sd=1.0):
    return rng.normal(0, sd, lead + rows * ld + OO.GUARD_TAIL).astype(np.float32)


def _rejected(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_guard_band_catches_a_stray_write():
    buf = OO.guard_buffer(5, 8, lead=3)
    idx = OO.region_index(5, 8, 2, 4, lead=3)
    buf[idx] = 1.0
    OO.assert_guard(buf, idx)
    for stray in (0, 3 + 1, 3 + 8 + 6, buf.size - 1):     # lead, a padding column left and right, the tail
        b = buf.copy()
        b[stray] = 0.0
        _rejected(OO.assert_guard, b, idx)
    b = buf.copy()
    b[0] = -OO.SENTINEL        # bit for bit: another value, not merely another magnitude
    _rejected(OO.assert_guard, b, idx)


def test_keep_mask_is_the_replica_of_gpu_util():
    from tests.gpu_util import dropout_keep_mask
    for step in (0, 3):
        assert np.array_equal(OO.keep_mask(4321, 70 * 37, 0.5, step), dropout_keep_mask(4321, 70 * 37, 0.5, step) != 0)


@pytest.mark.parametrize("C", [37, 40])
def test_affine_add_bounds(C):
    """fp32 evaluation accepted; one element off by 8 roundings of its magnitude rejected; Dropout mask indexed with
    m*ld + c instead of m*C + c rejected (shapes of test_affine_add_scalar_kernel_padded_slices / _dropout_mask_...)"""
    rng = np.random.default_rng(901)
    M, lda, ca, ldb, cb = 70, C + 3, 3, C + 7, 5
    a, b = _filled(rng, M, lda, sd=3.0), _filled(rng, M, ldb, sd=3.0)
    (sa, ta), (sb, tb) = _pars(rng, C), _pars(rng, C)
    args = (a, lda, ca, sa, ta, 2, b, ldb, cb, sb, tb, 1, M, C)
    ref, mag = OO.affine_add(*args)
    emu, _ = OO.affine_add(*args, dt=np.float32)
    assert OO.assert_elementwise(emu, ref, mag, 3) <= 0.5      # no FMA on the host: half the bound
    wrong = emu.astype(np.float64)
    wrong[M // 2, C // 2] += 8 * OO.U * mag[M // 2, C // 2]
    _rejected(OO.assert_elementwise, wrong, ref, mag, 3)
    ones = np.ones((M, C), np.float32)
    kw = dict(rate=0.5, seed=4321, step=3)
    ref, mag = OO.affine_add(ones, C, 0, None, None, 0, None, 0, 0, None, None, 0, M, C, **kw)
    bad, _ = OO.affine_add(ones, C, 0, None, None, 0, None, 0, 0, None, None, 0, M, C, bug="mask_ld", ldo=C + 12, **kw)
    assert not np.array_equal(bad, ref)
    _rejected(OO.assert_elementwise, bad, ref, mag, 6)


@pytest.mark.parametrize("M,C", [(7, 1), (65, 33), (203, 33), (33001, 33)])
def test_grad_finish_bounds(M, C):
    """fp32 evaluation accepted; the last row dropped from the per-channel sums rejected; the Dropout mask indexed with
    the leading dimension rejected (inputs of test_grad_finish_ragged_rows)"""
    rng = np.random.default_rng(910 + C)
    ldgin, ldadd, ldx = C + 3, C + 7, C + 9
    gin, add, x = _filled(rng, M, ldgin), _filled(rng, M, ldadd), _filled(rng, M, ldx, sd=3.0)
    s, t = _pars(rng, C)
    OO.put(x, OO.unambiguous_mask_input(OO.view(x, M, ldx, 4, C), s, t, 2), M, ldx, 4, C)
    mean, invstd = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    args = (gin, ldgin, 1, 1, 0.75, add, ldadd, 3, x, ldx, 4, s, t, 2, mean, invstd, M, C)
    ref, mag, (s1, a1, s2, a2) = OO.grad_finish(*args)
    emu, _, _ = OO.grad_finish(*args, dt=np.float32)
    assert OO.assert_elementwise(emu, ref, mag, 2) <= 0.5
    P = min(max(M // 64, 1), 512)
    chain = math.ceil(M / (8 * P)) + 8 + 2 + 3
    e64 = emu.astype(np.float32)
    xs = OO.view(x, M, ldx, 4, C)
    t1 = e64.sum(0, dtype=np.float32)
    t2 = (e64 * ((xs - mean) * invstd)).sum(0, dtype=np.float32)
    if M <= 8 * P:           # a host fp32 sum is one chain of M adds, the kernel's is ceil(M / 8P) + 8
        OO.assert_reduction(t1, s1, a1, M + 2)
        OO.assert_reduction(t2, s2, a2, M + 5)
    _, _, (b1, _, b2, _) = OO.grad_finish(*args, bug="drop_last_row")
    if M > 1:
        _rejected(OO.assert_reduction, b1, s1, a1, chain)
        _rejected(OO.assert_reduction, b2, s2, a2, chain)
    kw = dict(rate=0.5, seed=99, step=2)
    ref, mag = OO.grad_finish(*args[:14], None, None, M, C, **kw)
    bad, _ = OO.grad_finish(*args[:14], None, None, M, C, bug="mask_ld", **kw)
    if M > 1:
        _rejected(OO.assert_elementwise, bad, ref, mag, 5)


@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_conv_taps_padding_transformed_is_rejected(k, C):
    """act(shift) instead of 0 at the padding positions (SAME cases of test_conv_taps), and the adjoint identity"""
    rng = np.random.default_rng(950)
    N, H, W, ldx, cx = 2, 5, 7, C + 5, 2
    pad = (k - 1) // 2
    x = _filled(rng, N * H * W, ldx, sd=2.0)
    s, t = _pars(rng, C)
    t = (np.abs(t) + 0.5).astype(np.float32)
    for a in (0, 2):
        ref, mag = OO.conv_taps_fwd(x, ldx, cx, s, t, a, N, H, W, C, k, pad, pad, H, W)
        bad, _ = OO.conv_taps_fwd(x, ldx, cx, s, t, a, N, H, W, C, k, pad, pad, H, W, bug="pad_transformed")
        assert (mag == 0).any() and np.all(ref[mag == 0] == 0)
        OO.assert_elementwise(ref, ref, mag, 2)
        _rejected(OO.assert_elementwise, bad, ref, mag, 2)
    cols, _ = OO.conv_taps_fwd(x, ldx, cx, None, None, 0, N, H, W, C, k, pad, pad, H, W)
    d = rng.normal(0, 1, cols.shape)
    dx, ab = OO.conv_taps_bwd(d, N, H, W, C, k, pad, pad, H, W)
    xs = OO.view(x, N * H * W, ldx, cx, C).astype(np.float64).reshape(N, H, W, C)
    assert abs(np.sum(cols * d) - np.sum(xs * dx)) <= 1e-12 * np.sum(np.abs(xs) * ab)
    dropped = dx.copy()
    dropped[0, 0, 0] -= d.reshape(N, H, W, k * k, C)[0, 0, 0, pad * k + pad]     # the centre tap left out
    _rejected(OO.assert_reduction, dropped, dx, ab, k * k)


RESIZE_DIMS = [(2, 9, 11, 4, 5, 6), (1, 4, 12, 9, 5, 3), (1, 3, 5, 7, 11, 4), (1, 2, 33, 3, 130, 128),
               (1, 2, 130, 3, 131, 128)]


def test_resize_fp32_source_index():
    """which of the listed shapes hold an output index whose fp32 source coordinate fl(o * fl(in/out)) floors to another
    integer than the exact o*in/out: NONE of them (every in/out pair below); the oracle takes the index from the fp32
    product regardless.  A pair that does differ, to show the check can tell: 5 -> 3 does not, 7 <- 3 does not, but
    e.g. out = 49 from in = 5 does (o = 10, 20, ...: fl(5/49) * o rounds below the integer)."""
    for N, Hi, Wi, Ho, Wo, C in RESIZE_DIMS:
        assert OO.fp32_index_differs(Ho, Hi).size == 0 and OO.fp32_index_differs(Wo, Wi).size == 0
    found = [(o, i) for o in range(2, 64) for i in range(1, 16) if OO.fp32_index_differs(o, i).size]
    assert found, "no (out, in) pair below 64 x 16 with an fp32 / exact index disagreement"


@pytest.mark.parametrize("dims", RESIZE_DIMS[:4])
def test_resize_bounds(dims):
    """fp32 evaluation of the forward accepted; `hi` not clamped to in-1 rejected wherever an output index reaches the
    last input row / column (every shape that does not shrink BOTH axes); a tap dropped from the backward rejected"""
    N, Hi, Wi, Ho, Wo, C = dims
    rng = np.random.default_rng(960)
    ldx, cx = C + 7, 3
    x = _filled(rng, N * Hi * Wi, ldx, sd=2.0)
    s, t = _pars(rng, C)
    ref, mag = OO.resize_fwd(x, ldx, cx, s, t, 1, N, Hi, Wi, Ho, Wo, C)
    emu, _ = OO.resize_fwd(x, ldx, cx, s, t, 1, N, Hi, Wi, Ho, Wo, C, dt=np.float32)
    assert OO.assert_elementwise(emu, ref, mag, 9) <= 0.5
    bad, _ = OO.resize_fwd(x, ldx, cx, s, t, 1, N, Hi, Wi, Ho, Wo, C, bug="hi_unclamped")
    if Ho >= Hi or Wo >= Wi:
        _rejected(OO.assert_elementwise, bad, ref, mag, 9)
    else:
        OO.assert_elementwise(bad, ref, mag, 9)        # 9x11 -> 4x5 never reaches the clamp: see the other shapes
    rng = np.random.default_rng(961)
    lddy = C + 6
    dy = _filled(rng, N * Ho * Wo, lddy)
    dref, ab = OO.resize_bwd(dy, lddy, 1, N, Hi, Wi, Ho, Wo, C)
    chain = OO.taps_per_input(Wo, Wi) + OO.taps_per_input(Ho, Hi) + 8
    cols, _ = OO.resize_bwd_cols(OO.view(dy, N * Ho * Wo, lddy, 1, C).reshape(N, Ho, Wo, C), Wi, Wo)
    rows, _ = OO.resize_bwd_rows(cols, Hi, Ho)
    OO.assert_reduction(rows, dref, ab, 1)             # the separable restatement is the same operator
    short = OO.view(dy, N * Ho * Wo, lddy, 1, C).reshape(N, Ho, Wo, C).astype(np.float64).copy()
    short[:, -1, -1] = 0                                # the last output pixel never collected
    bad, _ = OO.resize_bwd(short, C, 0, N, Hi, Wi, Ho, Wo, C)
    _rejected(OO.assert_reduction, bad, dref, ab, chain)


@pytest.mark.parametrize("C", [1, 2, 21, 40])
def test_argmax_last_maximum_is_rejected(C):
    x = np.zeros((3, C), np.float32)
    x[1] = 1.5
    x[2, C // 2:] = 2.0
    assert np.array_equal(OO.argmax_first(x), [0, 0, C // 2])
    if C > 1:
        assert not np.array_equal(OO.argmax_first(x, bug="last_max"), OO.argmax_first(x))
    z = np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32)
    assert np.array_equal(OO.argmax_first(z), [0, 0]) and np.array_equal(OO.argmax_first(z, bug="last_max"), [1, 1])


@pytest.mark.parametrize("C", [1, 2, 32, 33])
def test_softmax_xent_bounds(C):
    """fp32 evaluation accepted (probabilities, gradient, loss); a void row given non-zero gradient rejected; a
    loss sum that leaves rows out rejected"""
    M = 33007
    rng = np.random.default_rng(972)
    x, labels, w = OO.xent_inputs(rng, M, C, void_w=True)
    nnz = float((w != 0).sum())
    r = OO.softmax_xent(x, labels, w, nnz)
    e = OO.softmax_xent(x, labels, w, nnz, dt=np.float32)
    assert OO.assert_elementwise(e["p"], r["p"], r["pmag"], C + 8) <= 0.5
    assert OO.assert_elementwise(e["dl"], r["dl"], r["dlmag"], C + 12) <= 0.5
    assert np.all(r["dl"][:20] == 0) and np.all(r["dl"][labels >= C] == 0)
    P = 512
    chain = math.ceil(M / (256 * P)) + 6 + 3 + 2 * C + 14
    OO.assert_reduction(np.array([e["l"].astype(np.float64).sum()]), np.array([r["l"].sum()]), np.array([r["lmag"].sum()]),
                        chain)
    bad = OO.softmax_xent(x, labels, w, nnz, bug="void_gradient")
    assert (labels >= C).any()
    _rejected(OO.assert_elementwise, bad["dl"], r["dl"], r["dlmag"], C + 12)
    half = np.where(np.arange(M) % 2 == 0, r["l"], 0.0)          # every other row's loss never added
    if C > 1:                # (C = 1: p == 1, every row's loss is the constant -log(1 - 1e-7f), below the rounding of q)
        _rejected(OO.assert_reduction, np.array([half.sum()]), np.array([r["l"].sum()]), np.array([r["lmag"].sum()]), chain)
    # the loss oracle agrees with oracle/dl3_oracle.py wherever the two clip constants cannot matter
    from oracle import dl3_oracle as O
    loss, dl, p = O.loss_sparse_xent_ignoring_last_label(x.astype(np.float64)[None], labels[None], w.astype(np.float64)[None])
    assert np.allclose(p[0], r["p"], rtol=1e-12, atol=0) and np.allclose(dl[0], r["dl"], rtol=1e-12, atol=1e-300)
    if C > 1:
        assert abs(loss - r["l"].sum()) <= 3e-7 * abs(loss)


def test_adam_bounds():
    """fp32 evaluation accepted for adam_step and adam_step_norm; a missing bias-free second moment term rejected"""
    n = 4099
    rng = np.random.default_rng(990)
    p, g = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    m, v = rng.normal(0, 0.1, n).astype(np.float32), rng.uniform(0, 0.1, n).astype(np.float32)
    kw = dict(lr_t=1e-3, b1=0.9, b2=0.999, eps=1e-8, gs=0.5)
    for denom, rds in ((None, (12, 4, 6)), (1234.0, (14, 5, 8)), (0.5, (14, 5, 8))):
        ref, mag = OO.adam(p, g, m, v, denom=denom, **kw)
        emu, _ = OO.adam(p, g, m, v, denom=denom, dt=np.float32, **kw)
        for e, r, mg, rd in zip(emu, ref, mag, rds):
            assert OO.assert_elementwise(e, r, mg, rd) <= 0.5
        wrong, _ = OO.adam(p, g * np.float32(1 + 3e-5), m, v, denom=denom, **kw)   # a gradient scale off by 3e-5
        _rejected(OO.assert_elementwise, wrong[1], ref[1], mag[1], rds[1])
    ref, _ = OO.adam(p, np.zeros(n, np.float32), m, v, denom=0.0, **kw)
    assert all(np.isfinite(r).all() for r in ref)


@pytest.mark.parametrize("P", [1, 33])
def test_bn_finalize_variance_not_clamped_is_rejected(P):
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
    args = (part, P, ldc, c0, C, count, gamma, beta, 1e-3, 0.99, 1.0, mm, mv)
    ref, bad = OO.bn_finalize(*args), OO.bn_finalize(*args, bug="var_unclamped")
    assert abs(ref["invstd"][5] - 1 / math.sqrt(float(np.float32(1e-3)))) < 1e-12
    assert all(np.isfinite(v).all() for v in ref.values()) and (np.delete(ref["invstd"], 5) < 31).all()
    for name in ("invstd", "scale"):   # (moving_var moves by 0.01 * |var|: below one rounding, the GPU test checks its direction)
        OO.assert_elementwise(ref[name].astype(np.float32), ref[name], np.abs(ref[name]), 1)
        _rejected(OO.assert_elementwise, bad[name], ref[name], np.abs(ref[name]), 1)
