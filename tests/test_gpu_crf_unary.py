"""-m gpu: the softmax unary of the dense CRF (csrc/crfunary.hip), crf.dense_crf_softmax and
Model.predict_mask(crf=True, crf_unary="softmax").

Bounds (none of them tuned to the device's output):
  * dl3_crf_unary_* — max-abs distance from the float64 oracle (tests/crf_unary_oracle.py) over max|U|, at most twice the
    same distance of the oracle's OWN float32 run (the rule of tests/test_gpu_crf.py and tests/test_gpu_eval.py).  Where
    that yardstick is exactly 0 the device must equal the float32 oracle.  Positions where the float32 oracle is +inf
    (clip = None and a probability that underflows) must be +inf on the device and are left out of the distance.
  * bilinear, no scale, no clip: the arg-min of U is dl3_resize_bilinear_fwd + dl3_argmax on every pixel whose two
    largest device logits differ.
  * dense_crf_softmax — the MAP equals the float64 mean-field (tests/crf_oracle.py) on the float64 unary except where
    the oracle itself cannot tell: float64 top-two gap of Q under tau = max(1e-5, 10 x |Q_float32 - Q_float64|_max), both
    from the oracle; at most 0.5 % of the pixels may be excused.  The seeds below were kept after the float32 oracle
    itself passed that rule against the float64 one on the CPU.  Q: distance <= 2 x the float32 oracle's.
  * model level — the fused forms read what the final resize / phase shift would have spread: the device unary of the
    plan must equal dl3_crf_unary_plain on the engine's materialised full-resolution logits BIT FOR BIT, and so must
    the masks (stricter than the excuse rule above, which it therefore satisfies).

Measured on the MI355X, worst device distance / float32-oracle distance per form: see DESIGN.md §9.
"""
import numpy as np
import pytest

from tests import crf_oracle as CO
from tests import crf_unary_oracle as UO

pytestmark = pytest.mark.gpu

EXCUSE_CAP = 0.005
SCALES = (0.0, 0.5)
CLIPS = (0.0, 1e-5)


# ---------------------------------------------------------------------------------------------------------- operator
def _device_unary(form, x, dims, B, C, scale, clip, is_prob=0):
    """one call through the C ABI -> U [B,C,N] host array.  dims: bilinear (Hi, Wi, Ho, Wo); shuffle (H, W, r); plain (N,)"""
    from tests import gpu_util as GU
    dx = GU.dev(x)
    if form == "bilinear":
        N = dims[2] * dims[3]
        U = GU.empty(B, C, N)
        GU.call("dl3_crf_unary_bilinear", GU.ptr(dx), GU.ptr(U), B, dims[0], dims[1], dims[2], dims[3], C, scale, clip)
    elif form == "shuffle":
        N = dims[0] * dims[2] * dims[1] * dims[2]
        U = GU.empty(B, C, N)
        GU.call("dl3_crf_unary_shuffle", GU.ptr(dx), GU.ptr(U), B, dims[0], dims[1], C, dims[2], scale, clip)
    else:
        N = dims[0]
        U = GU.empty(B, C, N)
        GU.call("dl3_crf_unary_plain", GU.ptr(dx), int(is_prob), GU.ptr(U), B, N, C, scale, clip)
    return GU.host(U)


def _shape_of(form, dims):
    return (dims[2], dims[3]) if form == "bilinear" else dims[2] if form == "shuffle" else None


def _input_shape(form, dims, B, C):
    if form == "bilinear":
        return (B, dims[0], dims[1], C)
    if form == "shuffle":
        return (B, dims[0], dims[1], C * dims[2] * dims[2])
    return (B, dims[0], C)


def _logits(kind, form, dims, B, C, rng):
    shp = _input_shape(form, dims, B, C)
    if kind == "equal":
        return np.full(shp, 0.75, np.float32)
    x = (4.0 * rng.standard_normal(shp)).astype(np.float32)   # N(0, 4^2): some probabilities fall under the clip
    if kind == "underflow":
        # class 0 at -100 and class 1 at >= 12: exp(-112) is 0 in float32 beyond doubt (its smallest subnormal is
        # exp(-103.3)), and far from 0 in float64
        v = x.reshape(shp[:-1] + ((C, -1) if form == "shuffle" else (C,)))
        if form == "shuffle":
            v[..., 0, :] = -100.0
            v[..., 1, :] = 12.0 + np.abs(v[..., 1, :])
        else:
            v[..., 0] = -100.0
            v[..., 1] = 12.0 + np.abs(v[..., 1])
    return x


def _compare(what, got, U64, U32):
    """-> (ratio, mine, yard); asserts the rule of the module docstring"""
    assert got.shape == U64.shape and got.dtype == np.float32
    inf32 = np.isinf(U32)
    assert np.array_equal(np.isinf(got), inf32) and np.array_equal(got[inf32], U32[inf32]), what
    fin = ~inf32 & np.isfinite(U64)
    assert not np.isnan(got).any(), what
    top = float(np.abs(U64[fin]).max()) if fin.any() else 0.0
    if top == 0.0:
        assert np.array_equal(got, U32), what
        return 0.0, 0.0, 0.0
    yard = float(np.abs(U32[fin].astype(np.float64) - U64[fin]).max()) / top
    mine = float(np.abs(got[fin].astype(np.float64) - U64[fin]).max()) / top
    if yard == 0.0:
        assert np.array_equal(got, U32), what
        return 0.0, mine, yard
    assert mine <= 2.0 * yard, (what, mine, yard)
    return mine / yard, mine, yard


def _run_cases(form, dims, C, kinds=("normal",), probs=(0,)):
    worst = (0.0, 0.0, 0.0, "")
    n = 0
    for kind in kinds:
        if kind == "underflow" and C < 2:
            continue
        for B in ((1, 3) if kind == "normal" else (1,)):
            rng = np.random.default_rng(1000 * C + 10 * B + sum(dims))
            z = _logits(kind, form, dims, B, C, rng)
            for is_prob in probs:
                x = UO.softmax(z, np.float32) if is_prob else z     # probabilities arrive as float32, as predict's do
                for scale in SCALES:
                    for clip in CLIPS:
                        kw = dict(is_prob=bool(is_prob), scale=scale or None, clip=clip or None)
                        U64 = UO.unary(form, x, _shape_of(form, dims), dtype=np.float64, **kw)
                        U32 = UO.unary(form, x, _shape_of(form, dims), dtype=np.float32, **kw)
                        if kind == "underflow" and not clip and not scale and not is_prob:
                            assert np.isinf(U32).any() and not np.isinf(U64).any()   # the case is what it claims to be
                        got = _device_unary(form, x, dims, B, C, scale, clip, is_prob)
                        what = "%s %r C=%d B=%d %s is_prob=%d scale=%g clip=%g" % (form, dims, C, B, kind, is_prob, scale, clip)
                        r = _compare(what, got, U64, U32)
                        worst = max(worst, r + (what,))
                        n += 1
    print("crf_unary_%s %r C=%d: %d cases, worst device %.3e against oracle-fp32 yardstick (1x) %.3e (ratio %.2f) at %s"
          % (form, dims, C, n, worst[1], worst[2], worst[0], worst[3]))


KINDS = ("normal", "underflow", "equal")


@pytest.mark.parametrize("C", [1, 2, 21, 32])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4099])
def test_unary_plain_against_float64(N, C):
    _run_cases("plain", (N,), C, KINDS, probs=(0, 1))


@pytest.mark.parametrize("C", [2, 21])
@pytest.mark.parametrize("dims", [(1, 1, 5, 7), (3, 5, 17, 33), (9, 9, 65, 65), (8, 8, 64, 64)])
def test_unary_bilinear_against_float64(dims, C):
    _run_cases("bilinear", dims, C, KINDS)


@pytest.mark.parametrize("C", [2, 21])
@pytest.mark.parametrize("dims", [(4, 4, 4), (2, 3, 8), (5, 3, 4)])
def test_unary_shuffle_against_float64(dims, C):
    _run_cases("shuffle", dims, C, KINDS)


def test_more_than_32_classes_is_unsupported():
    from dl3_amd import capi
    from tests import gpu_util as GU
    L = capi.lib()
    x, U = GU.dev(np.zeros(4 * 4 * 33 * 16)), GU.empty(33 * 256)
    assert L.dl3_crf_unary_plain(GU.ptr(x), 0, GU.ptr(U), 1, 16, 33, 0.0, 1e-5, GU.stream()) == -4
    assert b"classes" in L.dl3_last_error()
    assert L.dl3_crf_unary_bilinear(GU.ptr(x), GU.ptr(U), 1, 4, 4, 16, 16, 33, 0.0, 1e-5, GU.stream()) == -4
    assert L.dl3_crf_unary_shuffle(GU.ptr(x), GU.ptr(U), 1, 4, 4, 33, 4, 0.0, 1e-5, GU.stream()) == -4
    assert L.dl3_crf_unary_plain(None, 0, GU.ptr(U), 1, 16, 3, 0.0, 1e-5, GU.stream()) == -1
    assert L.dl3_crf_unary_plain(GU.ptr(x), 2, GU.ptr(U), 1, 16, 3, 0.0, 1e-5, GU.stream()) == -1
    assert np.isnan(GU.host(U)).all()   # nothing was launched


@pytest.mark.parametrize("C", [2, 21])
@pytest.mark.parametrize("dims", [(1, 1, 5, 7), (3, 5, 17, 33), (9, 9, 65, 65), (8, 8, 64, 64)])
def test_bilinear_argmin_is_the_resize_kernels_argmax(dims, C):
    import torch
    from tests import gpu_util as GU
    Hi, Wi, Ho, Wo = dims
    B = 3
    x = (4.0 * np.random.default_rng(7 + C + Ho).standard_normal((B, Hi, Wi, C))).astype(np.float32)
    got = _device_unary("bilinear", x, dims, B, C, 0.0, 0.0)
    dx, full = GU.dev(x), GU.empty(B * Ho * Wo * C)
    GU.call("dl3_resize_bilinear_fwd", GU.ptr(dx), C, None, None, 0, GU.ptr(full), C, B, Hi, Wi, Ho, Wo, C)
    am = torch.full((B * Ho * Wo,), -1, dtype=torch.int32, device="cuda")
    GU._KEEP.append(am)
    GU.call("dl3_argmax", GU.ptr(full), am.data_ptr(), B * Ho * Wo, C)
    z = GU.host(full).reshape(B, Ho * Wo, C)
    am = am.cpu().numpy().reshape(B, Ho * Wo)
    top2 = np.sort(z, -1)[..., -2:]
    decided = top2[..., 1] != top2[..., 0]
    assert decided.mean() > 0.9
    assert np.array_equal(got.argmin(1)[decided], am[decided])


@pytest.mark.parametrize("C", [2, 21])
@pytest.mark.parametrize("dims", [(3, 5, 17, 33), (9, 9, 65, 65), (5, 7, 33, 19)])
def test_bilinear_is_plain_on_the_resize_kernels_output(dims, C):
    """inexact scale factors, where a different contraction of the interpolation would show: the bilinear form's U is
    the plain form's on dl3_resize_bilinear_fwd's output, bit for bit"""
    from tests import gpu_util as GU
    Hi, Wi, Ho, Wo = dims
    B = 2
    x = (4.0 * np.random.default_rng(11 + C + Wo).standard_normal((B, Hi, Wi, C))).astype(np.float32)
    dx, full = GU.dev(x), GU.empty(B * Ho * Wo * C)
    GU.call("dl3_resize_bilinear_fwd", GU.ptr(dx), C, None, None, 0, GU.ptr(full), C, B, Hi, Wi, Ho, Wo, C)
    z = GU.host(full).reshape(B, Ho * Wo, C)
    for scale, clip in ((0.0, 0.0), (0.5, 1e-5)):
        fused = _device_unary("bilinear", x, dims, B, C, scale, clip)
        plain = _device_unary("plain", z, (Ho * Wo,), B, C, scale, clip)
        assert np.array_equal(fused.view(np.int32), plain.view(np.int32)), (dims, C, scale, clip)


def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(9)
    for form, dims, C in (("plain", (4099,), 21), ("bilinear", (9, 9, 65, 65), 21), ("shuffle", (5, 3, 4), 21),
                          ("plain", (256,), 32)):
        x = _logits("normal", form, dims, 3, C, rng)
        a = _device_unary(form, x, dims, 3, C, 0.5, 1e-5)
        b = _device_unary(form, x, dims, 3, C, 0.5, 1e-5)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), form


# ------------------------------------------------------------------------------------------------ dense_crf_softmax
# (H, W), C, seeds of the two images: kept after the CPU check described in the module docstring
E2E_CASES = [((24, 40), 3, (1, 2)), ((24, 40), 21, (1, 2)), ((31, 17), 3, (1, 2)), ((31, 17), 21, (1, 2))]

_ORACLE = {}


def _oracle(hw, C, seed):
    """computed once per input and shared; nothing writes to it"""
    key = (hw, C, seed)
    if key not in _ORACLE:
        im, logits = UO.softmax_case(hw[0], hw[1], C, seed)
        U64 = UO.unary("plain", logits.reshape(1, -1, C), None, dtype=np.float64)[0]
        U32 = UO.unary("plain", logits.reshape(1, -1, C), None, dtype=np.float32)[0]
        Q64, _, M64 = CO.inference(im, U64, dtype=np.float64)
        Q32, _, M32 = CO.inference(im, U32, dtype=np.float32)
        exc, tau, dist = UO.excusable(Q64, Q32)
        assert exc.mean() <= EXCUSE_CAP and not ((M32 != M64) & ~exc).any(), "the INPUT is too close to ties"
        _ORACLE[key] = dict(im=im, logits=logits, Q64=Q64, M64=M64, exc=exc, tau=tau, dist=dist)
    return _ORACLE[key]


@pytest.mark.parametrize("hw,C,seeds", E2E_CASES)
def test_dense_crf_softmax_against_float64(hw, C, seeds):
    from dl3_amd import crf
    H, W = hw
    cases = [_oracle(hw, C, s) for s in seeds]
    ims = np.stack([c["im"] for c in cases])
    logits = np.stack([c["logits"] for c in cases])
    got, Q = crf.dense_crf_softmax(ims, logits=logits, return_q=True)
    assert got.shape == (2, H, W) and got.dtype == np.int64 and Q.shape == (2, C, H * W)
    probs = UO.softmax(logits, np.float32)
    from_probs = crf.dense_crf_softmax(ims, probs=probs.reshape(2, H * W, C))
    for b, c in enumerate(cases):
        flips = got[b].reshape(-1) != c["M64"]
        mine = float(np.abs(Q[b].astype(np.float64) - c["Q64"]).max())
        print("dense_crf_softmax %dx%d C=%d seed %d: %d flips, %d excusable pixels of %d (tau %.2e); Q max-abs device %.3e, "
              "oracle-fp32 yardstick (1x) %.3e" % (H, W, C, seeds[b], int(flips.sum()), int(c["exc"].sum()), H * W, c["tau"],
                                                   mine, c["dist"]))
        assert c["exc"].mean() <= EXCUSE_CAP
        assert not (flips & ~c["exc"]).any(), "MAP differs on %d pixels the oracle resolves" % int((flips & ~c["exc"]).sum())
        assert mine <= 2.0 * c["dist"], (mine, c["dist"])
        assert not ((from_probs[b].reshape(-1) != got[b].reshape(-1)) & ~c["exc"]).any()
        # the CRF has to matter: its MAP is not the plain arg-max of the logits
        assert (c["M64"] != c["logits"].reshape(-1, C).argmax(-1)).mean() >= 0.02


def test_dense_crf_softmax_surface():
    import torch
    from dl3_amd import capi, crf
    from dl3_amd import utils as U
    c = _oracle((24, 40), 3, 1)
    im, logits = c["im"], c["logits"]
    one = crf.dense_crf_softmax(im[None], logits=logits[None])
    # device tensors in, a device tensor out; [B,H*W,C] is [B,H,W,C]
    dm = crf.dense_crf_softmax(torch.from_numpy(im[None]).cuda(), logits=torch.from_numpy(logits.reshape(1, -1, 3)).cuda())
    assert dm.is_cuda and dm.dtype == torch.int64 and np.array_equal(dm.cpu().numpy(), one)
    probs = UO.softmax(logits, np.float32)
    assert np.array_equal(U.do_crf_softmax(im, probs), crf.dense_crf_softmax(im[None], probs=probs[None])[0])
    # one class: nothing to infer; more than 32: refused
    z, Q = crf.dense_crf_softmax(im[None], logits=logits[None, :, :, :1], return_q=True)
    assert z.shape == (1, 24, 40) and not z.any() and Q.shape == (1, 1, 960) and (Q == 1).all()
    with pytest.raises(capi.DL3Error):
        crf.dense_crf_softmax(im[None], logits=np.zeros((1, 24, 40, 33), np.float32))
    with pytest.raises(ValueError):
        crf.dense_crf_softmax(im[None], logits=logits[None, :20])


# ------------------------------------------------------------------------------------------------------- model level
MODELS = [("mobilenetv2", "original", "dl3_crf_unary_bilinear", "dl3_resize_bilinear_fwd"),
          ("mobilenetv2", "subpixel", "dl3_crf_unary_shuffle", "dl3_phase_shift"),
          ("mobilenetv2", "deeplab", "dl3_crf_unary_bilinear", "dl3_resize_bilinear_fwd"),
          ("xception", "subpixel", "dl3_crf_unary_shuffle", "dl3_phase_shift")]


@pytest.mark.parametrize("backbone,head,op,gone", MODELS)
def test_predict_mask_softmax_unary(backbone, head, op, gone):
    import torch
    from dl3_amd import crf
    from tests.test_gpu_eval import _model
    C, B = 5, 2
    model = _model(backbone, head, classes=C)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:64, :64]
    x = rng.integers(0, 256, (B, 64, 64, 3)).astype(np.float32)
    x[..., 0] = (xx * 3 + yy) % 256
    # the parent's paths, before anything new has run
    plain0 = model.predict_mask(x, batch_size=B)
    crf0 = model.predict_mask(x, batch_size=B, crf=True)
    assert np.array_equal(crf0, crf.dense_crf(x, plain0))

    eng = model._engine(B, False)
    names = eng.crf_unary_op_names()
    fwd = [r[0] for r in eng.ops_fwd]
    assert names[-1] == op and "dl3_softmax_fwd" not in names
    assert fwd[-1] == gone and names[:-1] == fwd[:-1]
    if backbone == "xception":
        assert eng.units[-1].r == 4

    got = model.predict_mask(x, batch_size=B, crf=True, crf_unary="softmax")
    assert got.shape == (B, 64, 64) and got.dtype == np.int32
    # the reference route: the engine's materialised full-resolution logits through dense_crf_softmax
    eng.set_input(x)
    eng.forward()
    z = eng.logits()
    assert z.shape == (B, 64, 64, C)
    want = crf.dense_crf_softmax(x, logits=z)
    Uplan = eng.crf_unary()
    Uplain = crf.unary_plain(torch.from_numpy(z.reshape(B, -1, C)).cuda(), False)
    torch.cuda.synchronize()
    assert torch.equal(Uplan.view(torch.int32), Uplain.view(torch.int32))
    # the engine's plain route (a head that ends in neither a resize nor a phase shift), forced on this model: the whole
    # forward plan, then dl3_crf_unary_plain on the head's logits, and the same U
    names = eng.crf_unary_op_names(form="plain")
    assert names[-1] == "dl3_crf_unary_plain" and names[:-1] == fwd
    Uforced = eng.crf_unary(form="plain")
    torch.cuda.synchronize()
    assert torch.equal(Uforced.view(torch.int32), Uplan.view(torch.int32))
    assert eng.crf_unary_op_names()[-1] == op
    print("%s/%s: %s, %d of %d pixels differ from the arg-max mask" % (backbone, head, op, int((got != plain0).sum()), got.size))
    assert np.array_equal(got, want)
    # a second call with the same batch is bit-identical
    assert np.array_equal(model.predict_mask(x, batch_size=B, crf=True, crf_unary="softmax"), got)
    # the parent's paths afterwards: untouched, and "labels" is the default
    assert np.array_equal(model.predict_mask(x, batch_size=B), plain0)
    assert np.array_equal(model.predict_mask(x, batch_size=B, crf=True), crf0)
    assert np.array_equal(model.predict_mask(x, batch_size=B, crf=True, crf_unary="labels"), crf0)
    assert np.array_equal(model.predict_mask(x, batch_size=B, crf_unary="nonsense"), plain0)   # ignored without crf
    with pytest.raises(ValueError):
        model.predict_mask(x, crf=True, crf_unary="bogus")
