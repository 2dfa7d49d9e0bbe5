"""-m gpu: the dense-CRF kernels (csrc/crf.hip) through the C ABI against the float64 run of the numpy oracle
(tests/crf_oracle.py).  No tolerance is a constant: the yardstick of every comparison is the distance of the oracle's OWN
float32 run from its float64 run on the same inputs, and the device has to stay within twice that (the margin
tests/test_gpu_fullsize.py gives a second fp32 summation order).  Both numbers are printed.

MAP labels must equal the float64 MAP except on pixels whose float64 top-two margin is below twice that distance; at
most 0.5 % of the pixels may be excused that way, and the float32 oracle itself has to stay under the cap (asserted, so
that a failure points at the device and not at the input)."""
import numpy as np
import pytest
import torch

import dl3_amd  # noqa: F401
from dl3_amd import capi
from dl3_amd import crf as C
from dl3_amd import utils as U
from tests import crf_oracle as O
from tests.gpu_util import dev, empty, host, ptr, stream

pytestmark = pytest.mark.gpu

EXCUSE_CAP = 0.005


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def _ws(B, N, Lb):
    n = int(capi.lib().dl3_crf_workspace_bytes(B, 1, N, Lb))
    t = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    return t


def _features(kind, D, B, N, rng):
    """feature scales of the real model: positions x/80, y/80 of a (roughly square) raster, colours c/13 of a uint8 image —
    white noise (K nearly diagonal) or a smooth image (K far from diagonal)"""
    W = max(int(np.sqrt(N)), 1)
    i = np.arange(N)
    pos = np.stack([(i % W) / 80.0, (i // W) / 80.0], 1)
    f = np.empty((B, N, D))
    for b in range(B):
        if kind == "noise":
            col = rng.integers(0, 256, (N, 3)).astype(np.float64)
        else:
            col = 128 + 90 * np.stack([np.sin(pos[:, 0] * (3 + b)), np.cos(pos[:, 1] * 2.5), np.sin(pos.sum(1) * 2)], 1)
            col = np.rint(col + rng.integers(-2, 3, (N, 3)))
        full = np.concatenate([pos, col / 13.0], 1)
        f[b] = full[:, :D] if D == 2 else full[:, :D]
    return f.astype(np.float32)


def _message(feat, Q):
    B, N, D = feat.shape
    Lb = Q.shape[2]
    ws = _ws(B, N, Lb)
    out = empty(B, N, Lb)
    fd, qd = dev(feat), dev(Q)
    capi.call("dl3_crf_message", ptr(fd), D, ptr(qd), B, N, Lb, ptr(out), ws.data_ptr(), ws.numel(), stream())
    return host(out)


LABEL_COUNTS = (1, 2, 5, 21, 32)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2240, 9999])
@pytest.mark.parametrize("D", [2, 5])
def test_message_against_float64(D, N, B, kind):
    """every label count of LABEL_COUNTS on the same features: the message is linear in Q and its columns are
    independent, so the oracle's two runs are made once on 32 columns and the launch with L labels takes the first L"""
    rng = np.random.default_rng(1000 * D + N + B)
    feat = _features(kind, D, B, N, rng)
    Q = rng.random((B, N, 32)).astype(np.float32)
    ref = [O.message(feat[b].astype(np.float64), Q[b], np.float64) for b in range(B)]
    f32 = [O.message(feat[b], Q[b], np.float32) for b in range(B)]
    worst = (0.0, 0.0, 0.0)
    for Lb in LABEL_COUNTS:
        got = _message(feat, np.ascontiguousarray(Q[:, :, :Lb]))
        for b in range(B):
            r = ref[b][:, :Lb]
            scale = np.abs(r).max()
            yard = np.abs(f32[b][:, :Lb] - r).max() / scale
            mine = np.abs(got[b] - r).max() / scale
            worst = max(worst, (mine / max(yard, 1e-300), mine, yard))
            assert mine <= 2.0 * yard, (Lb, b, mine, yard)
    print("crf_message D=%d N=%d B=%d %s: worst device %.3e against oracle-fp32 yardstick (1x) %.3e (ratio %.2f)" % (
        D, N, B, kind, worst[1], worst[2], worst[0]))


def test_message_full_size_sampled():
    """512 x 512, 21 labels, a smooth image: every row computed on the device, 512 seeded rows compared with float64 sums
    over all 262 144 columns"""
    H = W = 512
    N, Lb = H * W, 21
    rng = np.random.default_rng(7)
    y, x = np.mgrid[:H, :W]
    im = np.stack([128 + 100 * np.sin(x / 70.0) * np.cos(y / 90.0), 128 + 100 * np.cos((x + y) / 110.0),
                   128 + 60 * np.sin(y / 40.0) + 40 * np.sin(x / 25.0)], -1)
    im = np.clip(np.rint(im + rng.integers(-2, 3, im.shape)), 0, 255).astype(np.uint8)
    feat = O.bilateral_features(im, 80, 13, np.float32)
    Q = rng.random((N, Lb)).astype(np.float32)
    got = _message(feat[None], Q[None])[0]
    rows = np.sort(rng.choice(N, 512, replace=False))
    ref = O.message_rows(feat.astype(np.float64), Q, rows, np.float64, block=32)
    f32 = O.message_rows(feat, Q, rows, np.float32, block=32)
    scale = np.abs(ref).max()
    yard, mine = np.abs(f32 - ref).max() / scale, np.abs(got[rows] - ref).max() / scale
    print("crf_message 512x512 L=21, 512 sampled rows: device %.3e, oracle-fp32 yardstick (1x) %.3e" % (mine, yard))
    assert mine <= 2.0 * yard, (mine, yard)


def _inference(im, Uh, iters=5):
    """im uint8 [B,H,W,3], Uh float32 [B,L,N] -> (Q, energy, map) host arrays"""
    B, H, W = im.shape[:3]
    Lb = Uh.shape[1]
    imd = torch.from_numpy(np.ascontiguousarray(im)).cuda()
    MAP, Q, E = C.inference(imd, dev(Uh), iters, want_q=True, want_energy=True)
    torch.cuda.synchronize()
    return Q.cpu().numpy(), E.cpu().numpy(), MAP.cpu().numpy()


def _map_parity(what, got_map, E64, E32, dist):
    """the excuse rule of the module docstring; returns the share of excused pixels"""
    want = E64.argmax(0)
    srt = np.sort(E64, 0)
    excusable = (srt[-1] - srt[-2]) < 2.0 * dist
    o32_flips = E32.argmax(0) != want
    flips = got_map != want
    print("%s: MAP flips device %d / oracle-fp32 %d of %d pixels; excusable pixels %d (oracle-fp32 flips among them %d)" % (
        what, int(flips.sum()), int(o32_flips.sum()), want.size, int(excusable.sum()), int((o32_flips & excusable).sum())))
    assert (o32_flips & ~excusable).sum() == 0 and excusable.mean() < EXCUSE_CAP, "the INPUT is too close to ties"
    assert not (flips & ~excusable).any(), "MAP differs on %d pixels float32 can resolve" % int((flips & ~excusable).sum())
    assert excusable.mean() <= EXCUSE_CAP
    return float(excusable.mean())


E2E_CASES = [(hw, Lb, zu) for hw in ((40, 56), (61, 47)) for Lb in (2, 4, 7) for zu in (False, True)]


@pytest.mark.parametrize("hw,Lb,zu", E2E_CASES)
def test_inference_end_to_end_against_float64(hw, Lb, zu):
    H, W = hw
    im, mask, _ = O.structured_case(H, W, Lb, seed=100 * Lb + H)
    colors, labels = np.unique(mask, return_inverse=True)
    labels = labels.reshape(-1)
    assert len(colors) == Lb
    U32 = C.unary_from_labels(labels, Lb, U.CRF_PARAMS["gt_prob"], zu)
    Q64, E64, M64 = O.inference(im, O.unary_from_labels(labels, Lb, 0.7, zu, np.float32).astype(np.float64))
    Q32, E32, M32 = O.inference(im, O.unary_from_labels(labels, Lb, 0.7, zu, np.float32), dtype=np.float32)
    # the appearance kernel has to matter: the result is not the input
    given = (labels - 1) % Lb if zu else labels
    assert (M64 != given).mean() >= 0.05
    Q, E, MAP = _inference(im[None], U32[None])
    dist = float(np.abs(E32.astype(np.float64) - E64).max())
    mine = float(np.abs(E[0] - E64).max())
    print("crf_inference %dx%d L=%d zero_unsure=%s: energy max-abs device %.3e, oracle-fp32 yardstick (1x) %.3e "
          "(max|energy| %.2f)" % (H, W, Lb, zu, mine, dist, float(np.abs(E64).max())))
    assert mine <= 2.0 * dist, (mine, dist)
    _map_parity("crf_inference %dx%d L=%d" % (H, W, Lb), MAP[0], E64, E32, dist)
    assert np.abs(Q[0].sum(0) - 1).max() < 1e-5
    assert np.array_equal(MAP[0], E[0].argmax(0))


@pytest.mark.parametrize("values", [(0, 1, 2), (0, 2, 15)])
@pytest.mark.parametrize("zu", [False, True])
def test_do_crf_device_backend_equals_the_oracle(values, zu):
    H, W = 40, 56
    im, mask, _ = O.structured_case(H, W, 3, seed=11)
    mask = np.array(values)[mask]
    got = U.do_crf(im, mask, zero_unsure=zu, backend="device")
    want, Q64, E64, M64, colors = O.do_crf(im, mask, zu, np.float64)
    _, _, E32, _, _ = O.do_crf(im, mask, zu, np.float32)
    assert got.shape == want.shape == (H, W) and got.dtype == want.dtype
    dist = float(np.abs(E32.astype(np.float64) - E64).max())
    srt = np.sort(E64, 0)
    excusable = ((srt[-1] - srt[-2]) < 2.0 * dist).reshape(H, W)
    print("do_crf device %r zero_unsure=%s: %d pixels differ, %d excusable" % (values, zu, int((got != want).sum()),
                                                                              int(excusable.sum())))
    assert excusable.mean() < EXCUSE_CAP
    assert not ((got != want) & ~excusable).any()


def test_batch_equals_single_calls_and_predict_mask():
    cases = [O.structured_case(40, 56, Lb, seed=20 + Lb) for Lb in (2, 5, 3)]
    ims = np.stack([c[0] for c in cases])
    masks = np.stack([c[1] for c in cases])
    for zu in (True, False):
        batch, Qb = C.dense_crf(ims, masks, zero_unsure=zu, return_q=True)
        for b in range(3):
            one, Q1 = C.dense_crf(ims[b:b + 1], masks[b:b + 1], zero_unsure=zu, return_q=True)
            assert np.array_equal(batch[b], one[0])
            assert np.array_equal(Qb[b, :Q1.shape[1]], Q1[0]) and not Qb[b, Q1.shape[1]:].any()
            assert np.array_equal(U.do_crf(ims[b], masks[b], zero_unsure=zu, backend="device"), one[0])
    # device tensors in, device tensors out
    dm = C.dense_crf(torch.from_numpy(ims).cuda(), torch.from_numpy(masks).cuda())
    assert dm.is_cuda and np.array_equal(dm.cpu().numpy(), C.dense_crf(ims, masks))
    # a single-valued mask comes back unchanged, alone and inside a batch
    flat = np.full((40, 56), 9, np.int32)
    assert np.array_equal(U.do_crf(ims[0], flat, backend="device"), flat)
    mixed = C.dense_crf(ims[:2], np.stack([flat, masks[1]]))
    assert np.array_equal(mixed[0], flat) and np.array_equal(mixed[1], C.dense_crf(ims[1:2], masks[1:2])[0])


def test_predict_mask_with_crf():
    from tests.test_gpu_model import _build, _load
    model, params = _build(input_shape=(64, 64, 3), classes=3)
    _load(model, params)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:64, :64]
    x = rng.integers(0, 256, (3, 64, 64, 3)).astype(np.float32)
    x[..., 0] = (xx * 3 + yy) % 256
    plain = model.predict_mask(x, batch_size=2)
    got = model.predict_mask(x, batch_size=2, crf=True)
    assert got.shape == plain.shape and got.dtype == np.int32
    assert np.array_equal(got, C.dense_crf(x, plain))
    assert np.array_equal(model.predict_mask(x, batch_size=2, crf=False), plain)


def test_inference_is_deterministic():
    im, mask, _ = O.structured_case(61, 47, 4, seed=31)
    U32 = C.unary_from_labels(mask.reshape(-1), 4, 0.7, False)
    imd = torch.from_numpy(np.stack([im, im[::-1].copy()])).cuda()
    Ud = dev(np.stack([U32, U32]))
    runs = [C.inference(imd, Ud, 5, want_q=True)[1] for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])


def test_error_reporting(L):
    """bad arguments come back as a status + message, not a crash"""
    N = 64
    f, q, o = dev(np.zeros((N, 8))), dev(np.zeros((N, 40))), empty(N, 40)
    ws = _ws(1, N, 32)
    args = lambda D, Lb, w, wb: (ptr(f), D, ptr(q), 1, N, Lb, ptr(o), w, wb, stream())  # noqa: E731
    assert L.dl3_crf_message(*args(5, 33, ws.data_ptr(), ws.numel())) == -4 and b"labels" in L.dl3_last_error()
    assert L.dl3_crf_message(*args(7, 5, ws.data_ptr(), ws.numel())) == -4 and b"feature" in L.dl3_last_error()
    assert L.dl3_crf_message(*args(5, 5, ws.data_ptr(), 16)) == -3 and b"workspace" in L.dl3_last_error()
    assert L.dl3_crf_message(*args(5, 5, None, 0)) == -3
    assert L.dl3_crf_message(None, 5, ptr(q), 1, N, 5, ptr(o), ws.data_ptr(), ws.numel(), stream()) == -1
    assert b"null" in L.dl3_last_error()
    assert L.dl3_crf_workspace_bytes(1, 8, 8, 33) == 0
    par = torch.from_numpy(C.kernel_params())
    im = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    inf = lambda i, u, Lb, p, wb: L.dl3_crf_inference(i, u, 1, 8, 8, Lb, p, 5, None, None, None, ws.data_ptr(), wb,  # noqa: E731
                                                      stream())
    assert inf(im.data_ptr(), ptr(q), 33, par.data_ptr(), ws.numel()) == -4
    assert inf(None, ptr(q), 4, par.data_ptr(), ws.numel()) == -1 and b"null" in L.dl3_last_error()
    assert inf(im.data_ptr(), ptr(q), 4, None, ws.numel()) == -1
    assert inf(im.data_ptr(), ptr(q), 4, par.data_ptr(), 64) == -3 and b"workspace" in L.dl3_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ feature dimensions, stage boundaries, 0 / 1 iterations
def _features_d(kind, D, B, N, rng):
    """_features at any D in 1..6: the first D of (x, y, r, g, b), and for D = 6 a sixth column of the same scale — the
    green channel in reversed pixel order"""
    f = _features(kind, 5, B, N, rng)
    if D <= 5:
        return np.ascontiguousarray(f[:, :, :D])
    return np.ascontiguousarray(np.concatenate([f, f[:, ::-1, 3:4]], 2))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("D", [1, 3, 4, 6])
def test_message_feature_dimensions_and_stage_boundaries(D, kind):
    """dl3_crf_message dispatches crf_pair_kernel<1|2|3> on ceil(D / 2): D = 3, 4 launch <2> (nothing else does), D = 1, 3
    take the odd-D zero fill (2 * k + 1 < D) in <1> and <2>, D = 6 fills <3>.  N sits on, one below and one above the
    128-column LDS stage, the 256-column compensated flush and the 256-row workgroup (127..257), and on a stage boundary
    past the first flush (385 = 3 * 128 + 1).  L in {1, 21, 32} on the same features, as test_message_against_float64:
    the yardstick is the oracle's float32 run, the factor 2."""
    B = 2
    for N in (127, 128, 129, 255, 256, 257, 385):
        rng = np.random.default_rng(1000 * D + N + B)
        feat = _features_d(kind, D, B, N, rng)
        assert feat.shape == (B, N, D)
        Q = rng.random((B, N, 32)).astype(np.float32)
        ref = [O.message(feat[b].astype(np.float64), Q[b], np.float64) for b in range(B)]
        f32 = [O.message(feat[b], Q[b], np.float32) for b in range(B)]
        worst = (0.0, 0.0, 0.0)
        for Lb in (1, 21, 32):
            got = _message(feat, np.ascontiguousarray(Q[:, :, :Lb]))
            again = _message(feat, np.ascontiguousarray(Q[:, :, :Lb]))
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), (N, Lb, "two runs differ")
            for b in range(B):
                r = ref[b][:, :Lb]
                scale = np.abs(r).max()
                yard = np.abs(f32[b][:, :Lb] - r).max() / scale
                mine = np.abs(got[b] - r).max() / scale
                worst = max(worst, (mine / max(yard, 1e-300), mine, yard))
                assert mine <= 2.0 * yard, (N, Lb, b, mine, yard)
        print("crf_message D=%d N=%d B=%d %s: worst device %.3e against oracle-fp32 yardstick (1x) %.3e (ratio %.2f)" % (
            D, N, B, kind, worst[1], worst[2], worst[0]))


@pytest.mark.parametrize("iters", [0, 1])
def test_inference_zero_and_one_iteration(iters):
    """dl3_crf_inference with iters = 0 (the first update writes Q, the energy and the MAP itself: Q = softmax(-U)) and
    iters = 1, on one 40 x 56 case against crf_oracle.inference(..., iters=): the energy and MAP rules of
    test_inference_end_to_end_against_float64, Q under the same yardstick; where the oracle's float32 run IS its float64
    run (iters = 0: the energy is -U) the device has to equal it bit for bit"""
    H, W, Lb, zu = 40, 56, 4, False
    im, mask, _ = O.structured_case(H, W, Lb, seed=100 * Lb + H)
    colors, labels = np.unique(mask, return_inverse=True)
    labels = labels.reshape(-1)
    assert len(colors) == Lb
    U32 = C.unary_from_labels(labels, Lb, U.CRF_PARAMS["gt_prob"], zu)
    Uo = O.unary_from_labels(labels, Lb, 0.7, zu, np.float32)
    Q64, E64, M64 = O.inference(im, Uo.astype(np.float64), iters=iters)
    Q32, E32, M32 = O.inference(im, Uo, dtype=np.float32, iters=iters)
    if iters == 0:
        assert np.array_equal(E64, -Uo.astype(np.float64)) and np.array_equal(Q64, O.softmax0(-Uo.astype(np.float64)))
    Q, E, MAP = _inference(im[None], U32[None], iters=iters)
    for name, got, r64, r32 in (("energy", E[0], E64, E32), ("Q", Q[0], Q64, Q32)):
        dist = float(np.abs(r32.astype(np.float64) - r64).max())
        mine = float(np.abs(got - r64).max())
        print("crf_inference %dx%d L=%d iters=%d: %s max-abs device %.3e, oracle-fp32 yardstick (1x) %.3e" % (
            H, W, Lb, iters, name, mine, dist))
        if dist == 0.0:
            assert np.array_equal(got, r32), name
        else:
            assert mine <= 2.0 * dist, (name, mine, dist)
    _map_parity("crf_inference %dx%d L=%d iters=%d" % (H, W, Lb, iters), MAP[0], E64, E32,
                float(np.abs(E32.astype(np.float64) - E64).max()))
    assert np.abs(Q[0].sum(0) - 1).max() < 1e-5
    assert np.array_equal(MAP[0], E[0].argmax(0))
