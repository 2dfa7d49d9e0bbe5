"""-m gpu tests of the 1x1-convolution GEMMs (csrc/pwstream.hip, pwlds.hip, pwws.hip, pwsmall.hip, pwwgrad.hip, pwfused.hip
behind csrc/pwplan.h) over the case table tests/pwconv_cases.py: every kernel instantiation the launchers can name, whole and
ragged tiles, and the shapes above the planner's row thresholds that the benchmarked networks do not have.

Exact cases: integer operands chosen so that every partial sum is an integer below 2**24 (conditions in the case module, checked
on the host by tests/test_pwconv_cases_host.py) — outputs, dY, dW after the slab fold, dbias and every statistic partial after a
float64 fold of its rows are compared with ==.  A duplicated, dropped or unzeroed element cannot hide in a tolerance.
Real-valued cases: ops_oracle.assert_reduction on outputs (abs-sum sum|a||b| + |bias| + |addend|, chain K + 4; split math: the
project's own 6e-7 * sum|a||b|), sums and weight gradients per channel at 1e-3 of the sum of the absolute terms.

Every device output lies between sentinel bands over a NaN payload (tests/gpu_util.Guarded); statistic partial buffers have
the dl3_pwconv_partials row count, workspaces the queried size; the columns of a wider buffer beside a written slice stay NaN."""
import numpy as np
import pytest
import torch

from tests import ops_oracle as R
from tests import pwconv_cases as C
from tests.gpu_util import BAND, Guarded, assert_bands, assert_untouched, dev, host, ptr, release, stream

pytestmark = pytest.mark.gpu
KNOBS = ("DL3_GEMM_CFG", "DL3_WGRAD_CFG", "DL3_GEMM_PRE", "DL3_GEMM_PY", "DL3_GEMM_MATH", "DL3_FUSED_V", "DL3_FUSED_OCC")
ROUTE_OF = {"stream": 0, "lds": 0, "wgrad": 0, "ws": 1, "ws2": 2, "ksplit": 3, "wgrad_row": 4, "flat": 5, "narrowk": 5, "wgrad_narrow": 5}
SUM_TOL = 1e-3
SPLIT_BOUND = 6e-7   # tests/test_gpu_ops.py test_split_math_error: |err| / sum|a||b| of the 3 x bf16 split


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    yield capi.lib()
    print("\n   worst error / bound of the real-valued cases: " +
          ", ".join("%s %.3f" % kv for kv in sorted(R.RATIOS.items()) if kv[0].startswith("pwconv")))


@pytest.fixture
def knobs(monkeypatch):
    def set_(case):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in case.knobs:
            monkeypatch.setenv(k, v)
    return set_


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
class _In:
    """an [M, C] operand at column `off` of a [M, off + C + extra] device buffer whose other columns hold a large finite value (a
    kernel that uses them gets a wrong result), one float off its 16-byte boundary when `mis`"""

    def __init__(self, a, off=0, extra=0, mis=False):
        M, Cw = a.shape
        lead = 1 if mis else 0
        self.ld = off + Cw + extra
        full = np.full(lead + M * self.ld, 1e4, np.float32)
        full[lead:].reshape(M, self.ld)[:, off:off + Cw] = a
        self.t = dev(full)
        self.p = ptr(self.t, lead + off)


def _vec(a):
    return ptr(dev(a)) if a is not None else None


class _Out:
    """an [M, C] output at column `off` of a guarded [M, off + C + extra] NaN buffer"""

    def __init__(self, pool, name, M, Cw, off=0, extra=0, mis=False):
        self.M, self.C, self.off, self.ld, self.mis = M, Cw, off, off + Cw + extra, int(mis)
        self.g = Guarded(pool, name, M * self.ld + self.mis)
        self.p = ptr(self.g.full, BAND + self.mis + off)

    def read(self):
        """the written slice; everything beside it must still be NaN"""
        flat = host(self.g.t)
        full = flat[self.mis:].reshape(self.M, self.ld)
        beside = np.ones(self.ld, bool)
        beside[self.off:self.off + self.C] = False
        assert np.isnan(full[:, beside]).all() and np.isnan(flat[:self.mis]).all(), "%s: written outside its slice" % self.g.name
        return full[:, self.off:self.off + self.C]


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = ~(got == want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ from the exact reference, first at %s: device %r, reference %r" % (
            name, int(bad.sum()), bad.size, i, got[i], want[i]))


def _fold(part, P, Cw):
    p = host(part.t).reshape(P, Cw, 2).astype(np.float64)
    return p[:, :, 0].sum(0), p[:, :, 1].sum(0)


def _check_output(case, name, got, r, chain):
    if case.exact:
        _same(case.id + " " + name, got, r["out"])
    elif C.runs_split_math(case):
        got = np.asarray(got, np.float64)
        err = np.abs(got - r["out"])
        ratio = R.worst_ratio(err, SPLIT_BOUND * r["out_abs"])
        R._note("pwconv-split", ratio)
        assert np.isfinite(got).all() and ratio <= 1.0, (case.id, name, ratio)
    else:
        R.assert_reduction(got, r["out"], r["out_abs"], chain, "pwconv-" + case.entry)


def _check_sums(case, part, P, Cw, r):
    s1, s2 = _fold(part, P, Cw)
    if case.exact:
        _same(case.id + " first statistic sum", s1, r["s1"])
        _same(case.id + " second statistic sum", s2, r["s2"])
    else:
        for got, want, ab in ((s1, r["s1"], r["a1"]), (s2, r["s2"], r["a2"])):
            assert np.isfinite(got).all()
            ratio = R.worst_ratio(np.abs(got - want), SUM_TOL * ab)
            R._note("pwconv-sums", ratio)
            assert ratio <= 1.0, (case.id, ratio)


def _check_dw(case, name, got, want, ab):
    if case.exact:
        _same(case.id + " " + name, got, want)
    else:
        got = np.asarray(got, np.float64)
        assert np.isfinite(got).all()
        ratio = R.worst_ratio(np.abs(got - want), SUM_TOL * np.asarray(ab, np.float64))
        R._note("pwconv-dw", ratio)
        assert ratio <= 1.0, (case.id, name, ratio)


def _assert_route(L, case):
    kernel = C.PLANS[case.id].split()[0]
    if C.misaligned(case) or case.knobs or case.entry == "fused":
        return
    d = None
    if case.entry == "fwd" and not case.add:
        d = 0
    elif case.entry == "bwd_data" and not case.two and not case.add:
        d = 1 if (case.stats and case.act) else (3 if not case.stats and not case.act else None)
    elif case.entry == "bwd_weight":
        d = 2 if case.two else (None if case.slabs else 4)
    if d is not None:
        want = ROUTE_OF[kernel] if (d != 3 or ROUTE_OF[kernel] == 5) else 0
        assert L.dl3_pwconv_route(d, case.M, case.K, case.N) == want, case.id


DEVICE_ERROR = []   # set by the first launch that leaves a device error: the tests after it launch nothing more


def _call(L, name, *args):
    rc = getattr(L, name)(*args, stream())
    if rc == -2:   # DL3_EHIP
        DEVICE_ERROR.append(name)
    assert rc == 0, "%s returned %d: %s" % (name, rc, L.dl3_last_error().decode())


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------------
def _fwd(L, c, d, r):
    M, K, N = c.M, c.K, c.N
    mis = C.misaligned(c)
    pool = []
    x = _In(d["x"], *C.layout(c, "x"), mis=mis)
    w = _In(d["w"], mis=mis)
    y = _Out(pool, "y", M, N, *C.layout(c, "y"), mis=mis)
    P = L.dl3_pwconv_partials(M, K, N)
    part = Guarded(pool, "stat_partial", P, N, 2) if c.stats else None
    args = (x.p, x.ld, _vec(d["s"]), _vec(d["t"]), c.act, w.p, _vec(d["bias"]), y.p, y.ld, M, K, N, part.p if part else None)
    if c.add:
        add = _In(d["add"], mis=mis)
        _call(L, "dl3_pwconv_fwd_add", *args, add.p, add.ld, C.ADD_DIV if c.add == 2 else 1)
    else:
        _call(L, "dl3_pwconv_fwd", *args)
    _check_output(c, "y", y.read(), r, K + 4)
    if part:
        _check_sums(c, part, P, N, r)
    assert_bands(pool)


def _wT(d, mis):
    return _In(np.ascontiguousarray(d["w"].T), mis=mis)


def _bwd_data(L, c, d, r):
    M, K, N = c.M, c.K, c.N
    mis = C.misaligned(c)
    pool = []
    g = _In(d["g"], *C.layout(c, "g"), mis=mis)
    yraw = _In(d["yraw"], *C.layout(c, "g"), mis=mis) if c.two else None
    wT = _wT(d, mis)
    need_x = bool(c.act) or c.stats
    x = _In(d["x"], *C.layout(c, "x"), mis=mis) if need_x else None
    dx = _Out(pool, "dx", M, K, *C.layout(c, "dx"), mis=mis)
    P = L.dl3_pwconv_partials(M, N, K)
    part = Guarded(pool, "dstat_partial", P, K, 2) if c.stats else None
    addp, ldadd, div = None, K, 1
    if c.add == 1:
        add = _In(d["add"], *C.layout(c, "dx"), mis=mis)
        addp, ldadd = add.p, add.ld
    elif c.add == 2:
        add = _In(d["add"], mis=mis)
        addp, ldadd, div = add.p, add.ld, C.ADD_DIV
    _call(L, "dl3_pwconv_bwd_data", g.p, g.ld, yraw.p if c.two else None, g.ld, _vec(d["cA"]), _vec(d["cB"]), _vec(d["cC"]), wT.p,
          dx.p, dx.ld, x.p if need_x else None, x.ld if need_x else K, _vec(d["s"]), _vec(d["t"]), c.act, addp, ldadd, div,
          C.ADD_SCALE, _vec(d["mean"]) if c.stats else None, _vec(d["invstd"]) if c.stats else None, part.p if part else None,
          M, K, N)
    _check_output(c, "dx", dx.read(), r, N + 4)
    if part:
        _check_sums(c, part, P, K, r)
    assert_bands(pool)


def _bwd_weight(L, c, d, r):
    M, K, N = c.M, c.K, c.N
    mis = C.misaligned(c)
    pool = []
    x = _In(d["x"], *C.layout(c, "x"), mis=mis)
    g = _In(d["g"], *C.layout(c, "g"), mis=mis)
    yraw = _In(d["yraw"], *C.layout(c, "g"), mis=mis) if c.two else None
    nbytes = L.dl3_pwconv_bwd_weight_workspace(M, K, N)
    assert nbytes % 4 == 0
    operands = (x.p, x.ld, _vec(d["s"]), _vec(d["t"]), c.act, g.p, g.ld, yraw.p if c.two else None, g.ld, _vec(d["cA"]),
                _vec(d["cB"]), _vec(d["cC"]))

    def launch(tag, with_dy):
        ws = Guarded(pool, "workspace" + tag, nbytes // 4)
        dw = None if c.slabs else Guarded(pool, "dw" + tag, K, N)
        db = Guarded(pool, "dbias" + tag, N) if c.dbias else None
        tail = (dw.p if dw else None, db.p if db else None, M, K, N, ws.p, nbytes)
        dy = None
        if with_dy:
            dy = _Out(pool, "dy_out", M, N, *C.layout(c, "dy"))
            _call(L, "dl3_pwconv_bwd_weight_dy", *operands, *tail, dy.p, dy.ld)
        else:
            _call(L, "dl3_pwconv_bwd_weight", *operands, *tail)
        if c.slabs:   # the slabs stay at the head of the workspace: the caller folds them
            S = L.dl3_pwconv_bwd_weight_splits(M, K, N, int(c.two))
            dw = Guarded(pool, "dw" + tag, K, N)
            _call(L, "dl3_reduce_partials", ws.p, S, K * N, dw.p)
        return host(dw.t).copy(), (host(db.t).copy() if db else None), dy

    dw, db, dy = launch("", c.dy_out)
    _check_dw(c, "dw", dw, r["dw"], r["dw_abs"])
    if c.dbias:
        _check_dw(c, "dbias", db, r["dbias"], r["dbias_abs"])
    if c.dy_out:
        got = dy.read()
        if c.exact:
            _same(c.id + " dy_out", got, r["dy"])
        else:   # one fp32 expression of three terms: cA*g + cB*yraw + cC
            mag = (np.abs(d["cA"] * d["g"].astype(np.float64)) + np.abs(d["cB"] * d["yraw"].astype(np.float64)) + np.abs(d["cC"])
                   if c.two else np.abs(d["g"]).astype(np.float64))
            R.assert_elementwise(got, r["dy"], mag, 3, "pwconv-dy")
        # the launch that also stores dY computes the gradient of dl3_pwconv_bwd_weight bit for bit
        dw0, _, _ = launch("-plain", False)
        assert np.array_equal(dw0.view(np.uint32), dw.view(np.uint32)), c.id
    assert_bands(pool)


def _fused(L, c, d, r):
    M, K, N = c.M, c.K, c.N
    pool = []
    assert L.dl3_pwconv_bwd_fused_supported(M, K, N) == (2 if K <= 64 else 1)
    S = L.dl3_pwconv_bwd_fused_splits(M, K, N)
    nbytes = L.dl3_pwconv_bwd_fused_workspace(M, K, N)
    assert nbytes == 4 * S * K * N
    x, g, wT = _In(d["x"]), _In(d["g"]), _wT(d, False)
    yraw = _In(d["yraw"]) if c.two else None
    add = _In(d["add"]) if c.add else None
    sx = x if c.stats == 1 else (_In(d["other"]) if c.stats == 2 else None)   # sums against x: the SAME device tensor

    def launch(tag, fold):
        ws = Guarded(pool, "workspace" + tag, S, K, N)
        dw = Guarded(pool, "dw" + tag, K, N)
        dx = Guarded(pool, "dx" + tag, M, K)
        part = Guarded(pool, "dstat_partial" + tag, S, K, 2) if c.stats else None
        _call(L, "dl3_pwconv_bwd_fused", x.p, x.ld, _vec(d["s"]), _vec(d["t"]), c.act, g.p, g.ld, yraw.p if c.two else None, N,
              _vec(d["cA"]), _vec(d["cB"]), _vec(d["cC"]), wT.p, dw.p if fold else None, dx.p, K, add.p if add else None, K,
              sx.p if sx else None, K, _vec(d["mean"]) if c.stats else None, _vec(d["invstd"]) if c.stats else None,
              part.p if part else None, M, K, N, ws.p, nbytes)
        if not fold:
            _call(L, "dl3_reduce_partials", ws.p, S, K * N, dw.p)
        return host(dw.t).copy(), host(dx.t).copy(), part

    dw, dx, part = launch("", not c.slabs)
    _check_output(c, "dx", dx, r, N + 4)
    _check_dw(c, "dw", dw, r["dw"], r["dw_abs"])
    if part:
        _check_sums(c, part, S, K, r)
    # folded by the op or by the caller: the same gradient, bit for bit
    dw2, dx2, _ = launch("-other-fold", c.slabs)
    assert np.array_equal(dw2.view(np.uint32), dw.view(np.uint32)) and np.array_equal(dx2.view(np.uint32), dx.view(np.uint32)), c.id
    assert_bands(pool)


DRIVER = {"fwd": _fwd, "bwd_data": _bwd_data, "bwd_weight": _bwd_weight, "fused": _fused}


def _run(L, case, knobs):
    assert not DEVICE_ERROR, "an earlier launch (%s) left a device error: nothing more is launched" % DEVICE_ERROR[0]
    knobs(case)
    _assert_route(L, case)
    d = C.draw(case)
    r = C.reference(case, d)
    try:
        try:
            DRIVER[case.entry](L, case, d, r)
        finally:
            if not DEVICE_ERROR:
                release()
    except RuntimeError as e:   # (torch reports a device error of an earlier launch at its next synchronisation)
        DEVICE_ERROR.append(str(e).splitlines()[0])
        raise


@pytest.mark.parametrize("case", C.GEMM_CASES, ids=lambda c: c.id)
def test_pwconv_gemm(L, case, knobs):
    """dl3_pwconv_fwd / _fwd_add / _bwd_data on the stream, LDS-staged, K-split and weight-stationary kernels"""
    _run(L, case, knobs)


@pytest.mark.parametrize("case", C.WGRAD_CASES, ids=lambda c: c.id)
def test_pwconv_weight_gradient(L, case, knobs):
    """dl3_pwconv_bwd_weight / _bwd_weight_dy on the tiled, one-tile-row and narrow kernels"""
    _run(L, case, knobs)


@pytest.mark.parametrize("case", C.FUSED_CASES, ids=lambda c: c.id)
def test_pwconv_fused(L, case, knobs):
    """dl3_pwconv_bwd_fused, round-5 and round-4 kernel"""
    _run(L, case, knobs)


@pytest.mark.parametrize("case", C.REAL + C.OLD, ids=lambda c: c.id)
def test_pwconv_real_valued(L, case, knobs):
    """normal operands at derived bounds: the off-benchmark shapes, the split-math forms, and every case list of the older 1x1 tests"""
    _run(L, case, knobs)


# ---- refusals: the status, the word of the message, and nothing written ---------------------------------------------------------------
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4


class _Refusal:
    """valid arguments of every entry point over one small layer (M = 40, K = 32, N = 64), by name; a refusal case replaces some"""

    def __init__(self, L):
        self.L, self.pool = L, []
        M, K, N = 40, 32, 64
        ones = lambda *s: ptr(dev(np.ones(s, np.float32)))
        self.out = {n: Guarded(self.pool, n, *s) for n, s in dict(y=(M, N), dx=(M, K), dw=(K, N), dbias=(N,), dy_out=(M, N),
                                                                    part=(64, N, 2), ws=(1 << 16,)).items()}
        o = {n: g.p for n, g in self.out.items()}
        vK, vN = ones(K), ones(N)
        self.base = {
            "dl3_pwconv_fwd": dict(x=ones(M, K), ldx=K, in_scale=vK, in_shift=vK, in_act=1, w=ones(K, N), bias=vN, y=o["y"], ldy=N,
                                   M=M, K=K, N=N, stat_partial=o["part"]),
            "dl3_pwconv_bwd_data": dict(g=ones(M, N), ldg=N, yraw=ones(M, N), ldyraw=N, cA=vN, cB=vN, cC=vN, wT=ones(N, K), dx=o["dx"],
                                        lddx=K, x=ones(M, K), ldx=K, in_scale=vK, in_shift=vK, in_act=1, dx_add=None, ldadd=K,
                                        add_div=1, add_scale=1.0, x_mean=vK, x_invstd=vK, dstat_partial=o["part"], M=M, K=K, N=N),
            "dl3_pwconv_bwd_weight": dict(x=ones(M, K), ldx=K, in_scale=vK, in_shift=vK, in_act=1, g=ones(M, N), ldg=N,
                                          yraw=ones(M, N), ldyraw=N, cA=vN, cB=vN, cC=vN, dw=o["dw"], dbias=None, M=M, K=K, N=N,
                                          workspace=o["ws"], workspace_bytes=4 << 16),
        }
        b = self.base
        b["dl3_pwconv_fwd_add"] = dict(b["dl3_pwconv_fwd"], add=ones(M, N), ldadd=N, add_div=1)
        b["dl3_pwconv_fwd_rows"] = dict({k: v for k, v in b["dl3_pwconv_fwd"].items() if k != "stat_partial"}, add=None, ldadd=N,
                                        add_div=1)
        b["dl3_pwconv_bwd_weight_dy"] = dict(b["dl3_pwconv_bwd_weight"], dy_out=o["dy_out"], lddy=N)
        bd = b["dl3_pwconv_bwd_data"]
        b["dl3_pwconv_bwd_fused"] = dict(
            x=bd["x"], ldx=K, in_scale=vK, in_shift=vK, in_act=1, g=bd["g"], ldg=N, yraw=bd["yraw"], ldyraw=N, cA=vN, cB=vN, cC=vN,
            wT=bd["wT"], dw=o["dw"], dx=o["dx"], lddx=K, dx_add=None, ldadd=K, stat_x=bd["x"], ldstatx=K, x_mean=vK, x_invstd=vK,
            dstat_partial=o["part"], M=M, K=K, N=N, workspace=o["ws"], workspace_bytes=4 << 16)
        self.other = ones(M, K)

    def call(self, entry, changes):
        from dl3_amd import capi
        kw = dict(self.base[entry])
        for k, v in changes.items():
            kw[k] = self.other if isinstance(v, str) and v == "other" else (kw[k] + v[1] if isinstance(v, tuple) else v)
        names = [a for _, a in capi.protos()[entry][1]]
        assert names[-1] == "stream" and set(names[:-1]) == set(kw), (entry, names, sorted(kw))
        return getattr(self.L, entry)(*[kw[a] for a in names[:-1]], stream())


REFUSALS = [
    # entry point, changed arguments (("+", n): the base pointer moved by n bytes), status, a word of the message
    ("dl3_pwconv_fwd", dict(M=0), EINVAL, "non-positive"),
    ("dl3_pwconv_fwd", dict(w=None), EINVAL, "null pointer"),
    ("dl3_pwconv_fwd", dict(ldy=60), EINVAL, "leading dimension"),
    ("dl3_pwconv_fwd", dict(in_shift=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_fwd_add", dict(N=-1), EINVAL, "non-positive"),
    ("dl3_pwconv_fwd_add", dict(add=None), EINVAL, "null pointer"),
    ("dl3_pwconv_fwd_add", dict(add_div=0), EINVAL, "add_div"),
    ("dl3_pwconv_fwd_add", dict(in_scale=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_fwd_rows", dict(K=0), EINVAL, "non-positive"),
    ("dl3_pwconv_fwd_rows", dict(x=None), EINVAL, "null pointer"),
    ("dl3_pwconv_fwd_rows", dict(ldx=8), EINVAL, "leading dimension"),
    ("dl3_pwconv_fwd_rows", dict(in_shift=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_fwd_rows", dict(M=65536), EUNSUPPORTED, "few rows"),
    ("dl3_pwconv_bwd_data", dict(M=0), EINVAL, "non-positive"),
    ("dl3_pwconv_bwd_data", dict(wT=None), EINVAL, "null pointer"),
    ("dl3_pwconv_bwd_data", dict(yraw=None), EINVAL, "cA needs"),
    ("dl3_pwconv_bwd_data", dict(x=None, dstat_partial=None), EINVAL, "mask needs x"),
    ("dl3_pwconv_bwd_data", dict(x_mean=None), EINVAL, "dstat needs"),
    ("dl3_pwconv_bwd_data", dict(in_scale=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_bwd_weight", dict(N=0), EINVAL, "non-positive"),
    ("dl3_pwconv_bwd_weight", dict(g=None), EINVAL, "null pointer"),
    ("dl3_pwconv_bwd_weight", dict(dw=None, dbias="other", cA=None), EINVAL, "dbias without dw"),
    ("dl3_pwconv_bwd_weight", dict(cB=None), EINVAL, "cA needs"),
    ("dl3_pwconv_bwd_weight", dict(in_shift=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_bwd_weight", dict(dbias="other"), EUNSUPPORTED, "dbias with"),
    ("dl3_pwconv_bwd_weight", dict(workspace_bytes=64), EWORKSPACE, "workspace"),
    ("dl3_pwconv_bwd_weight_dy", dict(dy_out=None), EINVAL, "dy_out is NULL"),
    ("dl3_pwconv_bwd_weight_dy", dict(lddy=66), EINVAL, "dy_out must be"),
    ("dl3_pwconv_bwd_weight_dy", dict(dy_out=("+", 4)), EINVAL, "dy_out must be"),
    ("dl3_pwconv_bwd_weight_dy", dict(workspace_bytes=64), EWORKSPACE, "workspace"),
    ("dl3_pwconv_bwd_fused", dict(M=0), EINVAL, "non-positive"),
    ("dl3_pwconv_bwd_fused", dict(K=30), EUNSUPPORTED, "multiples of 4"),
    ("dl3_pwconv_bwd_fused", dict(K=192, N=64), EUNSUPPORTED, "<= 6"),
    ("dl3_pwconv_bwd_fused", dict(wT=None), EINVAL, "null pointer"),
    ("dl3_pwconv_bwd_fused", dict(cC=None), EINVAL, "cA needs"),
    ("dl3_pwconv_bwd_fused", dict(in_scale=None), EINVAL, "scale/shift"),
    ("dl3_pwconv_bwd_fused", dict(x_invstd=None), EINVAL, "dstat needs"),
    ("dl3_pwconv_bwd_fused", dict(ldg=66), EINVAL, "16-byte aligned"),
    ("dl3_pwconv_bwd_fused", dict(x=("+", 4)), EINVAL, "16-byte aligned"),
    ("dl3_pwconv_bwd_fused", dict(workspace_bytes=64), EWORKSPACE, "workspace"),
    ("dl3_pwconv_bwd_fused", dict(K=96, N=32, ldx=96, lddx=96, dx_add="other"), EUNSUPPORTED, "K <= 64"),
    ("dl3_pwconv_bwd_fused", dict(dx_add="other", ldadd=34), EINVAL, "dx_add / stat_x"),
]


@pytest.fixture(scope="module")
def refusal(L):
    return _Refusal(L)


@pytest.mark.parametrize("entry,changes,status,word", REFUSALS,
                         ids=["%s-%s" % (e[4:], w.replace(" ", "_").replace("/", "_")) for e, _, _, w in REFUSALS])
def test_pwconv_refusals(L, refusal, entry, changes, status, word):
    """every DL3_CHECK_ARG / DL3_UNSUPPORTED / workspace check of the 1x1 entry points: its status, its message, no output touched"""
    assert not DEVICE_ERROR, "an earlier launch (%s) left a device error: nothing more is launched" % DEVICE_ERROR[0]
    assert refusal.call(entry, changes) == status
    assert word.encode() in L.dl3_last_error(), L.dl3_last_error()
    assert_untouched(refusal.pool)
    assert refusal.call(entry, {}) == 0   # ... and the unchanged arguments are a valid launch
    torch.cuda.synchronize()
    for g in refusal.pool:
        g.t.fill_(float("nan"))
    assert_untouched(refusal.pool)
