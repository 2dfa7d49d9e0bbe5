"""-m gpu parity tests of the depthwise 3x3 convolutions (csrc/dwconv.hip) on the paths tests/test_gpu_ops.py does not
reach: the straight-line row-loop bodies of the three march kernels (all four dw_march_bwd instantiations), several row
phases per workgroup in the two-pixel forward, rate 32, the optional operands of the backward kernels (no dx, no addend, no
statistics, a plain gradient), dw_gather_bwd at strides 2 and 3, the second grid-stride iteration of the gather kernels and
of dw_s2_bwd, dw_s2_bwd on mixed and absent padding, asymmetric padding at stride 1, and the argument checks.

Every reference is the float64 oracle (oracle/dl3_oracle.py) on the same seeded inputs; the case table, the Python mirror
of the planner and their host-side checks live in tests/dwconv_cases.py / tests/test_dwconv_cases_host.py.  Tensors are
compared at TOL (max|a-b| <= TOL * max|b|).  Every folded sum (the BatchNorm partials of the forward and of the backward,
the nine weight-gradient taps) is compared per channel: |s_c - ref_c| <= SUM_TOL * sum|terms_c|, the float64 sum of the
absolute values of what the kernel adds up for that channel, so a channel cannot hide behind a larger one.  Every device
output lies between two sentinel bands that the launch must leave bit-for-bit untouched and is NaN before the launch; the
partial buffers have the dl3_dwconv3x3_partials row count, so a NaN left in one is a row nobody wrote or zeroed."""
import zlib

import numpy as np
import pytest
import torch

from oracle import dl3_oracle as O
from tests import dwconv_cases as D
from tests.gpu_util import Guarded, assert_bands, assert_untouched, call, dev, host, np_act, np_mask, ptr, relerr, stream

pytestmark = pytest.mark.gpu
TOL = 2e-4
SUM_TOL = 1e-3
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    return capi.lib()


def _ppb_env(monkeypatch, ppb):
    if ppb is None:
        monkeypatch.delenv("DL3_DW_PPB", raising=False)
    else:
        monkeypatch.setenv("DL3_DW_PPB", str(ppb))


def _filled(gd, what):
    assert not bool(torch.isnan(gd.t).any()), "%s: %s holds an element no launch wrote" % (what, gd.name)


def _channel_sums(name, got, ref, terms):
    """|got_c - ref_c| <= SUM_TOL * terms_c for every channel (and tap); prints the worst ratio to the bound"""
    got, ref, terms = (np.asarray(a, np.float64) for a in (got, ref, terms))
    err = np.abs(got - ref)
    print(" %s %.1e" % (name, float((err / (SUM_TOL * terms + 1e-300)).max())), end="")
    bad = np.argwhere(err > SUM_TOL * terms)
    assert bad.size == 0, "%s: %d channel sums off, first at %s: got %r ref %r sum|terms| %r" % (
        name, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])], terms[tuple(bad[0])])


def _fold(part, P, C):
    p = host(part.t).reshape(P, C, 2).astype(np.float64)
    return p[:, :, 0].sum(0), p[:, :, 1].sum(0)


def _drive(L, case):
    """one case of the table through dl3_dwconv3x3_fwd and then dl3_dwconv3x3_bwd or, for an sx case, _bwd_sx (and _bwd on the
    same inputs: dx, dw and sum(dx) must be bit-identical between the two)"""
    geom, impl = case.geom, case.impl
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = geom
    P = D.plan_of(case).Pmax
    assert L.dl3_dwconv3x3_partials(N, H, W, C, stride, rate, Ho, Wo, impl) == P
    pool = []
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 1)
    x, s, t, act, _ = D.draw_view(case)
    w = rng.normal(0, 0.3, (3, 3, C)).astype(np.float32)
    z = D.preact(x, s, t)
    xin = np_act(z, act)
    wv = w.astype(np.float64)
    tape = O.Tape()
    ref = O.depthwise3x3(xin, wv, stride, rate, pt, pl, Ho, Wo, tape=tape)
    xd, wd = dev(x), dev(w)
    view = (ptr(dev(s)), ptr(dev(t)), act) if s is not None else (None, None, act)
    print("   %-34s" % case.id, end="")

    y = Guarded(pool, "y", N, Ho, Wo, C)
    part = Guarded(pool, "stat_partial", P, C, 2) if case.stats else None
    call("dl3_dwconv3x3_fwd", ptr(xd), *view, ptr(wd), y.p, *geom, part.p if part else None, impl)
    _filled(y, "forward")
    e = relerr(host(y.t), ref)
    print(" y %.2e" % e, end="")
    assert e < TOL
    if part:
        _filled(part, "forward")
        s1, s2 = _fold(part, P, C)
        _channel_sums("sum", s1, ref.sum((0, 1, 2)), np.abs(ref).sum((0, 1, 2)))
        _channel_sums("sumsq", s2, (ref ** 2).sum((0, 1, 2)), (ref ** 2).sum((0, 1, 2)))

    # the gradient operand: BatchNorm-backward affine of two tensors (cA*g + cB*yraw + cC), or g itself
    g = rng.normal(0, 1, ref.shape).astype(np.float32)
    if case.grad == "bn":
        yraw = rng.normal(0, 1, ref.shape).astype(np.float32)
        cA, cB, cC = [rng.normal(0, 1, C).astype(np.float32) for _ in range(3)]
        dY = cA * g.astype(np.float64) + cB * yraw.astype(np.float64) + cC
        operand = (ptr(dev(yraw)), ptr(dev(cA)), ptr(dev(cB)), ptr(dev(cC)))
    else:
        dY = g.astype(np.float64)
        operand = (None, None, None, None)
    grads = tape.backward(ref, dY)
    dw_ref, dw_terms = grads[id(wv)], D.dw_abs_terms(xin, dY, geom)
    add = rng.normal(0, 1, x.shape).astype(np.float32) if case.add else None
    mean = rng.normal(0, 1, C).astype(np.float32)
    invstd = rng.uniform(0.5, 2, C).astype(np.float32)
    other = rng.normal(0, 1, x.shape).astype(np.float32) if case.sx else None
    head = (ptr(dev(g)), *operand, ptr(xd), *view, ptr(wd))
    addp, meanp, invp = ptr(dev(add)) if case.add else None, ptr(dev(mean)), ptr(dev(invstd))

    def launch(sx):
        dx = Guarded(pool, "dx", N, H, W, C)
        dpart = Guarded(pool, "dstat_partial", P, C, 2) if case.stats else None
        wpart = Guarded(pool, "dw_partial", P, 9, C)
        stat = (meanp, invp, dpart.p) if dpart else (None, None, None)
        mid = (dx.p if case.dx else None, addp) + ((ptr(dev(other)),) if sx else ())
        call("dl3_dwconv3x3_bwd_sx" if sx else "dl3_dwconv3x3_bwd", *head, *mid, *stat, wpart.p, *geom, impl)
        return dx, dpart, wpart

    dx, dpart, wpart = launch(case.sx)
    _filled(wpart, "backward")
    _channel_sums("dw", host(wpart.t).astype(np.float64).sum(0).reshape(3, 3, C), dw_ref, dw_terms)
    if not case.dx:
        torch.cuda.synchronize()
        assert dx.unwritten(), "a weight-gradient-only launch wrote dx"
    else:
        _filled(dx, "backward")
        dx_ref = grads[id(xin)] * np_mask(z, act)
        if case.add:
            dx_ref = dx_ref + add
        dxg = host(dx.t)
        e = relerr(dxg, dx_ref)
        print(" dx %.2e" % e, end="")
        assert e < TOL
        # input rows and columns under no tap: the gradient there is the addend itself
        dead_y, dead_x = (Ho - 1) * stride - pt + 2 * rate + 1, (Wo - 1) * stride - pl + 2 * rate + 1
        if case.add and (dead_y < H or dead_x < W):
            assert np.array_equal(dxg[:, dead_y:].view(np.int32), add[:, dead_y:].view(np.int32))
            assert np.array_equal(dxg[:, :, dead_x:].view(np.int32), add[:, :, dead_x:].view(np.int32))
        if dpart:
            _filled(dpart, "backward")
            d1, d2 = _fold(dpart, P, C)
            xhat = ((other if case.sx else x).astype(np.float64) - mean) * invstd
            _channel_sums("dsum", d1, dx_ref.sum((0, 1, 2)), np.abs(dx_ref).sum((0, 1, 2)))
            _channel_sums("dsum_xhat", d2, (dx_ref * xhat).sum((0, 1, 2)), np.abs(dx_ref * xhat).sum((0, 1, 2)))
    if case.sx:
        dx0, dpart0, wpart0 = launch(False)
        assert np.array_equal(host(dx0.t).view(np.int32), host(dx.t).view(np.int32))
        assert np.array_equal(host(wpart0.t).view(np.int32), host(wpart.t).view(np.int32))
        d0, d1 = host(dpart0.t).view(np.int32), host(dpart.t).view(np.int32)
        assert np.array_equal(d0[:, :, 0], d1[:, :, 0])                      # sum(dx): the same
        assert not np.array_equal(d0[:, :, 1], d1[:, :, 1])                  # the second sum is against another tensor
        print(" sx==bwd", end="")
    print()
    assert_bands(pool)


@pytest.mark.parametrize("case", D.MARCH_CASES, ids=lambda c: c.id)
def test_dwconv_march(L, case, monkeypatch):
    """dw_march_fwd / dw_march2_fwd and the four dw_march_bwd instantiations"""
    _ppb_env(monkeypatch, case.ppb)
    assert D.bwd_kernel(case) == "dw_march_bwd"
    _drive(L, case)


@pytest.mark.parametrize("case", D.GATHER_CASES, ids=lambda c: c.id)
def test_dwconv_gather(L, case, monkeypatch):
    """dw_gather_fwd and dw_gather_bwd"""
    _ppb_env(monkeypatch, None)
    assert (D.fwd_kernel(case), D.bwd_kernel(case)) == ("dw_gather_fwd", "dw_gather_bwd")
    _drive(L, case)


@pytest.mark.parametrize("case", D.S2_CASES, ids=lambda c: c.id)
def test_dwconv_stride2_backward(L, case, monkeypatch):
    """dw_gather_fwd and dw_s2_bwd"""
    _ppb_env(monkeypatch, None)
    assert (D.fwd_kernel(case), D.bwd_kernel(case)) == ("dw_gather_fwd", "dw_s2_bwd")
    _drive(L, case)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.id)
def test_partials_equal_the_mirror(L, case, monkeypatch):
    """dl3_dwconv3x3_partials against the Python planner, for every impl a launch of the geometry can be sized with"""
    _ppb_env(monkeypatch, case.ppb)
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = case.geom
    for impl in (D.AUTO, D.GATHER, D.MARCH):
        if impl == D.MARCH and not D.march_ok(case.geom):
            continue
        assert L.dl3_dwconv3x3_partials(N, H, W, C, stride, rate, Ho, Wo, impl) == D.partials(case.geom, impl, case.ppb), impl


# ---- refusals: a status, and nothing written ------------------------------------------------------------------------------------
class _Args:
    """the operands of a launch on `geom`, every output guarded; keyword overrides replace single arguments"""

    def __init__(self, geom):
        N, H, W, C, stride, rate, pt, pl, Ho, Wo = geom
        n_in, n_out, C = max(N * H * W, 1), max(N * Ho * Wo, 1), max(C, 4)
        self.geom, self.pool = geom, []
        self.x, self.g, self.w, self.c = dev(np.ones((n_in, C))), dev(np.ones((n_out, C))), dev(np.ones((9, C))), dev(np.ones(C))
        self.y, self.dx = Guarded(self.pool, "y", n_out, C), Guarded(self.pool, "dx", n_in, C)
        self.part, self.dpart = Guarded(self.pool, "stat_partial", 16, C, 2), Guarded(self.pool, "dstat_partial", 16, C, 2)
        self.wpart = Guarded(self.pool, "dw_partial", 16, 9, C)

    def fwd(self, L, impl, **o):
        a = dict(x=ptr(self.x), sc=None, sh=None, act=0, w=ptr(self.w), y=self.y.p, part=self.part.p, geom=self.geom)
        a.update(o)
        return L.dl3_dwconv3x3_fwd(a["x"], a["sc"], a["sh"], a["act"], a["w"], a["y"], *a["geom"], a["part"], impl, stream())

    def bwd(self, L, impl, sx=False, **o):
        c = ptr(self.c)
        a = dict(g=ptr(self.g), yraw=ptr(self.g), cA=c, cB=c, cC=c, x=ptr(self.x), sc=None, sh=None, act=0, w=ptr(self.w),
                 dx=self.dx.p, add=None, stat_x=ptr(self.x), mean=c, invstd=c, dpart=self.dpart.p, wpart=self.wpart.p,
                 geom=self.geom)
        a.update(o)
        head = (a["g"], a["yraw"], a["cA"], a["cB"], a["cC"], a["x"], a["sc"], a["sh"], a["act"], a["w"], a["dx"], a["add"])
        tail = (a["mean"], a["invstd"], a["dpart"], a["wpart"], *a["geom"], impl, stream())
        if sx:
            return L.dl3_dwconv3x3_bwd_sx(*head, a["stat_x"], *tail)
        return L.dl3_dwconv3x3_bwd(*head, *tail)


SAME8 = D.same(1, 8, 8, 32, 1, 1)


def _with(geom, **kw):
    names = "N H W C stride rate pad_t pad_l Ho Wo".split()
    return tuple(kw.get(n, v) for n, v in zip(names, geom))


@pytest.mark.parametrize("geom,rc,word", [(_with(SAME8, C=6), EUNSUPPORTED, b"multiple of 4"),
                                          (_with(SAME8, C=34), EUNSUPPORTED, b"multiple of 4"),
                                          (_with(SAME8, H=0), EINVAL, b"non-positive"), (_with(SAME8, N=-1), EINVAL, b"non-positive"),
                                          (_with(SAME8, Wo=0), EINVAL, b"non-positive"), (_with(SAME8, C=0), EINVAL, b"non-positive"),
                                          (_with(SAME8, rate=0), EINVAL, b"rate"), (_with(SAME8, stride=0), EINVAL, b"stride")],
                         ids=["c6", "c34", "h0", "n-1", "wo0", "c0", "rate0", "stride0"])
def test_dw_check_refuses(L, geom, rc, word):
    """dw_check: the forward and both backward entry points return the same status and write nothing"""
    a = _Args(geom)
    for status in (a.fwd(L, D.AUTO), a.bwd(L, D.AUTO), a.bwd(L, D.AUTO, sx=True)):
        assert status == rc and word in L.dl3_last_error()
    assert_untouched(a.pool)


def test_operand_combinations_are_argument_errors(L):
    """DL3_EINVAL, nothing written: scale without shift, cA without yraw, dstat_partial without dx or x_mean, stat_x without
    dstat_partial, dl3_dwconv3x3_bwd_sx without stat_x, a NULL required pointer"""
    a = _Args(SAME8)
    c = ptr(a.c)
    assert a.fwd(L, D.AUTO, sc=c) == EINVAL and b"scale/shift" in L.dl3_last_error()
    assert a.fwd(L, D.AUTO, sh=c) == EINVAL
    assert a.fwd(L, D.AUTO, y=None) == EINVAL and b"null" in L.dl3_last_error()
    for sx in (False, True):
        assert a.bwd(L, D.AUTO, sx, sc=c) == EINVAL and b"scale/shift" in L.dl3_last_error()
        assert a.bwd(L, D.AUTO, sx, yraw=None) == EINVAL and b"yraw" in L.dl3_last_error()
        assert a.bwd(L, D.AUTO, sx, cB=None) == EINVAL
        assert a.bwd(L, D.AUTO, sx, dx=None) == EINVAL and b"dstat" in L.dl3_last_error()
        assert a.bwd(L, D.AUTO, sx, mean=None) == EINVAL and b"dstat" in L.dl3_last_error()
        assert a.bwd(L, D.AUTO, sx, invstd=None) == EINVAL
        assert a.bwd(L, D.AUTO, sx, wpart=None) == EINVAL and b"null" in L.dl3_last_error()
    assert a.bwd(L, D.AUTO, True, dpart=None) == EINVAL and b"stat_x without dstat_partial" in L.dl3_last_error()
    assert a.bwd(L, D.AUTO, True, stat_x=None) == EINVAL and b"stat_x is NULL" in L.dl3_last_error()
    assert_untouched(a.pool)


@pytest.mark.parametrize("geom", [D.same(1, 8, 8, 32, 2, 1), D.padded(1, 8, 8, 32, 1, 1, 0, 0), (1, 8, 8, 32, 1, 2, 1, 1, 8, 8),
                                  (1, 8, 8, 32, 1, 1, 1, 0, 8, 8)], ids=["stride2", "valid", "pad1-rate2", "pad_l0"])
def test_march_is_refused_off_its_geometry(L, geom):
    """impl = DL3_IMPL_MARCH at stride 2, and at stride 1 with pads that are not the rate: DL3_EUNSUPPORTED"""
    assert D.resolve_impl(D.MARCH, geom) == -1
    a = _Args(geom)
    for status in (a.fwd(L, D.MARCH), a.bwd(L, D.MARCH), a.bwd(L, D.MARCH, sx=True)):
        assert status == EUNSUPPORTED and b"march impl needs" in L.dl3_last_error()
    assert_untouched(a.pool)


@pytest.mark.parametrize("geom,impl", [(SAME8, D.GATHER), (D.same(1, 8, 8, 32, 2, 1), D.AUTO), (D.AUTO_REFUSED[0], D.GATHER)],
                         ids=["gather-asked", "stride2", "asym-pad"])
def test_sums_against_another_tensor_need_the_march_kernel(L, geom, impl):
    assert D.resolve_impl(impl, geom) == D.GATHER
    a = _Args(geom)
    assert a.bwd(L, impl, sx=True) == EUNSUPPORTED and b"need the march kernel" in L.dl3_last_error()
    assert_untouched(a.pool)


@pytest.mark.parametrize("geom", D.AUTO_REFUSED, ids=lambda g: "x".join(map(str, g)))
def test_auto_is_refused_where_its_partials_count_march_rows_for_a_gather_launch(L, geom):
    """stride 1, Ho == H, Wo == W, pads that are not the rate: dl3_dwconv3x3_partials(DL3_IMPL_AUTO) is the march count, the
    launch would run the gather kernels over more rows.  DL3_EUNSUPPORTED from the forward and the backward, the message
    names DL3_IMPL_GATHER (tests/dwconv_cases.py GATHER_CASES runs such geometries under it)"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = geom
    assert D.auto_mismatch(D.AUTO, geom)
    assert L.dl3_dwconv3x3_partials(N, H, W, C, stride, rate, Ho, Wo, D.AUTO) == D.partials(geom, D.AUTO)
    assert L.dl3_dwconv3x3_partials(N, H, W, C, stride, rate, Ho, Wo, D.GATHER) == D.partials(geom, D.GATHER)
    a = _Args(geom)
    for status in (a.fwd(L, D.AUTO), a.bwd(L, D.AUTO)):
        assert status == EUNSUPPORTED and b"DL3_IMPL_GATHER" in L.dl3_last_error()
    assert_untouched(a.pool)


@pytest.mark.parametrize("geom", D.AUTO_TAKEN, ids=lambda g: "x".join(map(str, g)))
def test_auto_is_taken_where_its_rules_agree(L, geom):
    """the refusal stops at its condition: SAME, VALID, stride 2 and over-padded geometries launch under DL3_IMPL_AUTO into
    buffers of dl3_dwconv3x3_partials(DL3_IMPL_AUTO) rows"""
    N, H, W, C, stride, rate, pt, pl, Ho, Wo = geom
    assert not D.auto_mismatch(D.AUTO, geom)
    P = L.dl3_dwconv3x3_partials(N, H, W, C, stride, rate, Ho, Wo, D.AUTO)
    assert P == D.partials(geom, D.AUTO) <= 16
    a = _Args(geom)
    for gd in (a.part, a.dpart, a.wpart):      # P rows of the 16-row buffers are the launch's
        gd.t[P:].fill_(0.0)
    assert a.fwd(L, D.AUTO) == 0 and a.bwd(L, D.AUTO) == 0
    assert_bands(a.pool)
    assert not any(bool(torch.isnan(gd.t).any()) for gd in a.pool)
    for gd in (a.part, a.dpart, a.wpart):
        assert not bool(gd.t[P:].any()), gd.name
