"""-m gpu parity tests of the dense 3x3 convolutions (csrc/conv3x3.hip) on the paths tests/test_gpu_ops.py does not reach:
the matrix-pipe stem kernels on ragged-only / whole-tile / one- and two-channel / VALID / activated inputs, the route
boundary inside dl3_conv3x3_fwd, the direct vector-ALU kernels at every supported width and in their grid-stride loops,
backward-data at stride 2, and the tap-gather MFMA kernels on an even stride-2 map and in their second outer step.

Every reference is the float64 oracle (oracle/dl3_oracle.py) on the same seeded inputs; the case table and its host-side
checks live in tests/conv3x3_cases.py / tests/test_conv3x3_cases_host.py.  Tolerances are the library's own: TOL on
tensors (max|a-b| <= TOL * max|b|), 1e-3 on folded partial sums and on weight gradients.  Every device output lies inside
a larger buffer with a sentinel band on either side that the launch must leave bit-for-bit untouched, and is NaN before
the launch, so an unwritten element or partial row poisons what is compared."""
import zlib

import numpy as np
import pytest

from oracle import dl3_oracle as O
from tests import conv3x3_cases as C
from tests.gpu_util import Guarded as _Guarded, assert_bands as _assert_bands, assert_untouched as _assert_untouched
from tests.gpu_util import call, dev, host, np_act, np_mask, ptr, relerr, stream

pytestmark = pytest.mark.gpu
TOL = 2e-4
SUM_TOL = 1e-3


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    return capi.lib()


def _sums(part, P, C_):
    p = host(part.t).reshape(P, C_, 2).astype(np.float64)
    return p[:, :, 0].sum(0), p[:, :, 1].sum(0)


def _drive(L, case):
    """forward + both BatchNorm partial sums, weight gradient, backward-data + both BatchNorm-backward partial sums of one
    case of the table, through the direct (dl3_conv3x3_*) or the tap-gather (dl3_conv3x3_mfma_*) entry points"""
    geom = case.geom
    N, H, W, Cin, Cout, stride, pt, pl, Ho, Wo = geom
    tap = case.api == "tap"
    if tap:
        assert L.dl3_conv3x3_mfma_supported(Cin, Cout) == 1
    pool = []
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 1)
    x, s, t, act, _ = C.draw_view(case)
    w = rng.normal(0, 0.2, (3, 3, Cin, Cout)).astype(np.float32)
    z = C.preact(x, s, t)
    xin = np_act(z, act)
    wv = w.astype(np.float64)
    tape = O.Tape()
    ref = O.conv2d(xin, wv, stride, pt, pl, Ho, Wo, tape=tape)
    xd, wd = dev(x), dev(w)
    sd, td = (dev(s), dev(t)) if s is not None else (None, None)
    print("   %-36s" % case.id, end="")

    if "f" in case.ops:
        P = L.dl3_conv3x3_mfma_partials(N, Ho, Wo) if tap else L.dl3_conv3x3_partials(N, Ho, Wo, Cout)
        y = _Guarded(pool, "y", N, Ho, Wo, Cout)
        part = _Guarded(pool, "stat_partial", P, Cout, 2) if case.stats else None
        call("dl3_conv3x3_mfma_fwd" if tap else "dl3_conv3x3_fwd", ptr(xd), ptr(sd), ptr(td), act, ptr(wd), y.p, *geom,
             part.p if part else None)
        e = relerr(host(y.t), ref)
        print(" y %.2e" % e, end="")
        assert e < TOL
        if part:
            s1, s2 = _sums(part, P, Cout)
            e1, e2 = relerr(s1, ref.sum((0, 1, 2))), relerr(s2, (ref ** 2).sum((0, 1, 2)))
            print(" sum %.2e sumsq %.2e" % (e1, e2), end="")
            assert e1 < SUM_TOL and e2 < SUM_TOL

    # the gradient operand: BatchNorm-backward affine of two tensors (cA*g + cB*yraw + cC), or g itself
    g = rng.normal(0, 1, ref.shape).astype(np.float32)
    gd = dev(g)
    if case.grad == "bn":
        yraw = rng.normal(0, 1, ref.shape).astype(np.float32)
        cA, cB, cC = [rng.normal(0, 1, Cout).astype(np.float32) for _ in range(3)]
        dY = cA * g.astype(np.float64) + cB * yraw.astype(np.float64) + cC
        operand = (ptr(dev(yraw)), ptr(dev(cA)), ptr(dev(cB)), ptr(dev(cC)))
    else:
        dY = g.astype(np.float64)
        operand = (None, None, None, None)
    grads = tape.backward(ref, dY)

    if "w" in case.ops:
        if tap:
            wsb = L.dl3_conv3x3_mfma_bwd_weight_workspace(N, H, W, Cin, Cout, stride, Ho, Wo)
            assert wsb % 4 == 0
            ws = _Guarded(pool, "workspace", wsb // 4)
            dw = _Guarded(pool, "dw", 3, 3, Cin, Cout)
            call("dl3_conv3x3_mfma_bwd_weight", ptr(xd), ptr(sd), ptr(td), act, ptr(gd), *operand, dw.p, *geom, ws.p, wsb)
            dwg = host(dw.t)
        else:
            Pw = L.dl3_conv3x3_partials(N, Ho, Wo, Cout)
            wpart = _Guarded(pool, "dw_partial", Pw, 9 * Cin * Cout)
            call("dl3_conv3x3_bwd_weight", ptr(xd), ptr(sd), ptr(td), act, ptr(gd), *operand, wpart.p, *geom)
            dwg = host(wpart.t).astype(np.float64).sum(0).reshape(3, 3, Cin, Cout)
        e = relerr(dwg, grads[id(wv)])
        print(" dw %.2e" % e, end="")
        assert e < SUM_TOL

    if "d" in case.ops:
        if tap:
            wk = dev(np.ascontiguousarray(w.reshape(9 * Cin, Cout).T))   # wT [Cout][9*Cin]
            P2 = L.dl3_conv3x3_mfma_partials(N, H, W)
        else:
            wk = wd
            P2 = L.dl3_conv3x3_partials(N, H, W, Cin)
        dx = _Guarded(pool, "dx", N, H, W, Cin)
        dpart = _Guarded(pool, "dstat_partial", P2, Cin, 2) if case.stats else None
        add = rng.normal(0, 1, (N, H, W, Cin)).astype(np.float32) if case.add else None
        mean = rng.normal(0, 1, Cin).astype(np.float32)
        invstd = rng.uniform(0.5, 2, Cin).astype(np.float32)
        stat_args = (ptr(dev(mean)), ptr(dev(invstd)), dpart.p) if dpart else (None, None, None)
        view = (None, None, None, 0) if case.xnull else (ptr(xd), ptr(sd), ptr(td), act)
        call("dl3_conv3x3_mfma_bwd_data" if tap else "dl3_conv3x3_bwd_data", ptr(gd), operand[0], *operand[1:], ptr(wk), dx.p,
             *view, ptr(dev(add)) if case.add else None, *stat_args, *geom)
        dx_ref = grads[id(xin)] * (1.0 if case.xnull else np_mask(z, act))
        if case.add:
            dx_ref = dx_ref + add
        e = relerr(host(dx.t), dx_ref)
        print(" dx %.2e" % e, end="")
        assert e < TOL
        if dpart:
            d1, d2 = _sums(dpart, P2, Cin)
            e1 = relerr(d1, dx_ref.sum((0, 1, 2)))
            e2 = relerr(d2, (dx_ref * (x.astype(np.float64) - mean) * invstd).sum((0, 1, 2)))
            print(" dsum %.2e dsum_xhat %.2e" % (e1, e2), end="")
            assert e1 < SUM_TOL and e2 < SUM_TOL
    print()
    _assert_bands(pool)


@pytest.mark.parametrize("case", C.DIRECT_CASES, ids=lambda c: c.id)
def test_conv3x3_direct_and_stem(L, case):
    """dl3_conv3x3_fwd / _bwd_weight / _bwd_data: the stem kernels on the matrix pipe where the route takes them, the
    direct vector-ALU kernels everywhere else"""
    _drive(L, case)


@pytest.mark.parametrize("case", C.TAP_CASES, ids=lambda c: c.id)
def test_conv3x3_tap_mfma(L, case):
    """dl3_conv3x3_mfma_fwd / _bwd_weight / _bwd_data, the tap-gather kernels"""
    _drive(L, case)


# ---- refusals: a status, and nothing written ------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -4


def _refusal_buffers(Cin, Cout, geom):
    N, H, W = geom[:3]
    Ho, Wo = geom[-2:]
    pool = []
    ins = dict(x=dev(np.ones((N, H, W, Cin))), w=dev(np.ones((3, 3, Cin, Cout))), g=dev(np.ones((N, Ho, Wo, Cout))),
               c=dev(np.ones(max(Cin, Cout))))
    outs = dict(y=_Guarded(pool, "y", N, Ho, Wo, Cout), part=_Guarded(pool, "partial", 4, max(Cin, Cout), 2),
                dw=_Guarded(pool, "dw", 4, 9 * Cin * Cout), dx=_Guarded(pool, "dx", N, H, W, Cin),
                ws=_Guarded(pool, "workspace", 9 * Cin * Cout))
    return ins, outs, pool


@pytest.mark.parametrize("Cout", [24, 40, 48])
def test_direct_refuses_unsupported_output_widths(L, Cout):
    """MobileNetV2 stems of alpha 0.75, 1.3, 1.4: DL3_EUNSUPPORTED from the forward and the weight gradient"""
    assert not C.direct_supported(Cout)
    geom = C.same(1, 8, 8, 3, Cout, 2)
    i, o, pool = _refusal_buffers(3, Cout, geom)
    assert L.dl3_conv3x3_fwd(ptr(i["x"]), None, None, 0, ptr(i["w"]), o["y"].p, *geom, o["part"].p, stream()) == EUNSUPPORTED
    assert b"Cout" in L.dl3_last_error()
    assert L.dl3_conv3x3_bwd_weight(ptr(i["x"]), None, None, 0, ptr(i["g"]), None, None, None, None, o["dw"].p, *geom,
                                    stream()) == EUNSUPPORTED
    _assert_untouched(pool)


@pytest.mark.parametrize("Cin", [6, 12])
def test_direct_bwd_data_refuses_unsupported_input_widths(L, Cin):
    assert not C.direct_supported(Cin)
    geom = C.same(1, 8, 8, Cin, 8, 1)
    i, o, pool = _refusal_buffers(Cin, 8, geom)
    assert L.dl3_conv3x3_bwd_data(ptr(i["g"]), None, None, None, None, ptr(i["w"]), o["dx"].p, None, None, None, 0, None, None,
                                  None, None, *geom, stream()) == EUNSUPPORTED
    _assert_untouched(pool)


@pytest.mark.parametrize("Cin,Cout", [(48, 32), (32, 48), (48, 48), (64, 48)])
def test_tap_refuses_unsupported_channel_pairs(L, Cin, Cout):
    assert L.dl3_conv3x3_mfma_supported(Cin, Cout) == 0
    geom = C.same(1, 8, 8, Cin, Cout, 1)
    i, o, pool = _refusal_buffers(Cin, Cout, geom)
    assert L.dl3_conv3x3_mfma_fwd(ptr(i["x"]), None, None, 0, ptr(i["w"]), o["y"].p, *geom, o["part"].p, stream()) == EUNSUPPORTED
    assert L.dl3_conv3x3_mfma_bwd_data(ptr(i["g"]), None, None, None, None, ptr(i["w"]), o["dx"].p, None, None, None, 0, None,
                                       None, None, None, *geom, stream()) == EUNSUPPORTED
    assert L.dl3_conv3x3_mfma_bwd_weight(ptr(i["x"]), None, None, 0, ptr(i["g"]), None, None, None, None, o["dw"].p, *geom,
                                         o["ws"].p, 4 * o["ws"].n, stream()) == EUNSUPPORTED
    _assert_untouched(pool)


def test_gradient_operand_without_yraw_is_an_argument_error(L):
    """cA given, yraw NULL: DL3_EINVAL from every launch that takes the two-tensor gradient operand"""
    geom = C.same(1, 8, 8, 32, 32, 1)
    i, o, pool = _refusal_buffers(32, 32, geom)
    c = ptr(i["c"])
    assert L.dl3_conv3x3_bwd_weight(ptr(i["x"]), None, None, 0, ptr(i["g"]), None, c, c, c, o["dw"].p, *geom, stream()) == EINVAL
    assert b"yraw" in L.dl3_last_error()
    assert L.dl3_conv3x3_bwd_data(ptr(i["g"]), None, c, c, c, ptr(i["w"]), o["dx"].p, None, None, None, 0, None, None, None,
                                  None, *geom, stream()) == EINVAL
    assert L.dl3_conv3x3_mfma_bwd_data(ptr(i["g"]), None, c, c, c, ptr(i["w"]), o["dx"].p, None, None, None, 0, None, None,
                                       None, None, *geom, stream()) == EINVAL
    assert L.dl3_conv3x3_mfma_bwd_weight(ptr(i["x"]), None, None, 0, ptr(i["g"]), None, c, c, c, o["dw"].p, *geom, o["ws"].p,
                                         4 * o["ws"].n, stream()) == EINVAL
    _assert_untouched(pool)
