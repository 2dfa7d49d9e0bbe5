"""-m gpu: the trimap kernels (dl3_trimap_rings, dl3_trimap_confusion), trimap.py, Model.confusion_matrix_trimap and
utils.trimap_iou / trimap_iou_from_masks against the numpy oracle tests/trimap_oracle.py.

Everything is integer-exact: every comparison is bit for bit, no tolerance is chosen anywhere.

The images of a case (B, H, W, C): B = 1 is the "corner" image (a 3x3 block of class 1 in a corner on background: every
ring value the image has room for occurs), B = 2 a blobby map (arg-max of smoothed noise, about 1 % void) and the corner
image, B = 3 a blobby map, a constant image (no seeds: "beyond" everywhere) and the corner image; the (2, 5, 130, 4) case has
an all-void image in place of the blobby one.  (A batch of two has room for two kinds: the constant image rides in the
B = 3 case, which is also the one run at wmax = 254, where nothing else could fill the last bin.)  That every bin of every
case is non-empty is asserted on the oracle before the device is looked at."""
import ctypes
import functools

import numpy as np
import pytest

from tests import trimap_oracle as TO

pytestmark = pytest.mark.gpu

CASES = [(3, 37, 53, 21), (2, 5, 130, 4), (2, 64, 64, 33), (1, 1, 40, 3), (1, 40, 1, 3), (2, 96, 72, 21)]
RUNS = [(i, w) for i in range(len(CASES)) for w in (1, 4, 32)] + [(0, 254)]   # 254: larger than the image
METRIC_ID = {TO.CHEBYSHEV: 0, TO.EUCLIDEAN: 1}
GUARD = 64            # sentinel elements in front of and behind every guarded output
FILL = 0xA5


def _ids(v):
    return str(v).replace(" ", "")


@functools.lru_cache(maxsize=None)
def _labels(i):
    B, H, W, C = CASES[i]
    rng = np.random.default_rng(100 + i)
    first = np.full((H, W), C, np.float32) if (B, H, W, C) == (2, 5, 130, 4) else TO.blobby(rng, 1, H, W, C)[0]
    imgs = {1: [TO.corner(H, W)], 2: [first, TO.corner(H, W)],
            3: [first, np.full((H, W), 2.0, np.float32), TO.corner(H, W)]}[B]
    lab = np.stack(imgs)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _distance(i, metric, seeds):
    """the oracle's rings at wmax = 254, computed once per (case, metric, seed mask).  No image here is wider than 130
    pixels, so this is the unclamped distance (255 where the image has no seed) and the ring at any wmax is its clamp."""
    r = TO.rings(_labels(i), CASES[i][3], 254, metric, seeds)
    assert ((r <= 130) | (r == 255)).all()
    r.setflags(write=False)
    return r


def _want_rings(i, wmax, metric, seeds):
    return np.minimum(_distance(i, metric, seeds), wmax + 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pred(i):
    """the label map shifted by (2, 3) pixels, void replaced by random classes (off-diagonal bins fill), and about 2 % each
    of -1 and C, which must be skipped"""
    B, H, W, C = CASES[i]
    rng = np.random.default_rng(200 + i)
    p = np.roll(TO.canon(_labels(i), C), (2, 3), axis=(1, 2))
    p = np.where(p == C, rng.integers(0, C, p.shape), p)
    u = rng.random(p.shape)
    p = np.where(u < 0.02, -1, np.where(u < 0.04, C, p)).astype(np.int32)
    p.setflags(write=False)
    return p


def _widths(wmax, most):
    if not most:
        return (wmax,)
    return {1: (1,), 4: (1, 2, 3, 4), 32: (1, 2, 3, 4, 8, 16, 24, 32), 254: (1, 2, 4, 8, 16, 32, 40, 254)}[wmax]


class Guarded:
    """a device output of n elements inside a larger buffer of sentinels, `offset` elements behind the front guard"""

    def __init__(self, n, dtype, offset=0, fill=FILL):
        import torch
        self.n, self.lo, self.fill = n, GUARD + offset, fill
        self.full = torch.full((n + 2 * GUARD + offset,), fill, dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + n]

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.full[:self.lo] == self.fill).all()) and bool((self.full[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.full == self.fill).all())


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()   # (a copy: the cached inputs are read-only)


def _ints(ws):
    return (ctypes.c_int * len(ws))(*ws)


def _run_rings(lab, C, wmax, metric, seeds, offset):
    """dl3_trimap_rings through the C ABI into a guarded output -> uint8 [B,H,W] on the host"""
    import torch
    from tests import gpu_util as GU
    from dl3_amd import capi
    B, H, W = lab.shape
    dl = _dev(lab, np.float32)
    out = Guarded(B * H * W, torch.uint8, offset)
    nws = capi.lib().dl3_trimap_workspace_bytes(B, H, W)
    ws = Guarded(nws, torch.uint8, 0)        # GUARD = 64 keeps it 4-byte aligned
    GU.call("dl3_trimap_rings", dl.data_ptr(), out.ptr(), ws.ptr(), B, H, W, C, wmax, METRIC_ID[metric], seeds)
    torch.cuda.synchronize()
    assert out.guards_intact() and ws.guards_intact(), "wrote outside its output"
    return out.t.cpu().numpy().reshape(B, H, W)


# ------------------------------------------------------------------------------------------------------------ rings
@pytest.mark.parametrize("i,wmax", RUNS, ids=_ids)
def test_rings_equal_the_oracle(i, wmax):
    B, H, W, C = CASES[i]
    lab = _labels(i)
    for metric in (TO.CHEBYSHEV, TO.EUCLIDEAN):
        for seeds in (1, 2, 3):
            want = _want_rings(i, wmax, metric, seeds)
            if seeds == 3:   # 254 is larger than the image: there the corner image reaches 49, the constant one "beyond"
                assert all((want == v).any() for v in list(range(min(wmax + 1, 36) + 1)) + [wmax + 1]), "a ring value is missing"
            # offset 4: the output is 4- but not 16-byte aligned (dword stores where a row allows); offset 1: byte stores
            got = _run_rings(lab, C, wmax, metric, seeds, offset=4)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (metric, seeds, np.argwhere(got != want)[:5])
            # images never see each other: the batch's rings are those of each image run alone
            for b in range(B):
                alone = _run_rings(lab[b:b + 1], C, wmax, metric, seeds, offset=1)
                assert np.array_equal(alone[0], got[b]), (metric, seeds, b)


# -------------------------------------------------------------------------------------------------------- confusion
@pytest.mark.parametrize("most", [False, True], ids=["K1", "Kmost"])
@pytest.mark.parametrize("i,wmax", RUNS, ids=_ids)
def test_confusion_equals_the_oracle(i, wmax, most):
    import torch
    from tests import gpu_util as GU
    B, H, W, C = CASES[i]
    widths = _widths(wmax, most)
    K = len(widths)
    assert K == (8 if most and wmax >= 32 else K)
    lab, pred = _labels(i), _pred(i)
    ring = _want_rings(i, wmax, TO.CHEBYSHEV, 3)
    want = TO.band_confusion(pred, lab, ring, C, widths)
    assert (want.sum((1, 2)) > 0).all(), "an empty bin: %r" % (want.sum((1, 2)),)
    assert (want.sum(0) - np.diag(np.diag(want.sum(0)))).sum() > 0 and np.array_equal(want.sum(0), TO.confusion(pred, lab, C))
    n = B * H * W
    dl = _dev(lab, np.float32)
    # K = 1: aligned inputs, 16 bytes a lane; the other run: pred and rings off their alignment, the scalar form
    off = 1 if most else 0
    dp = torch.zeros(n + 4, dtype=torch.int32, device="cuda")[off:off + n].copy_(_dev(pred).reshape(-1))
    dr = torch.zeros(n + 4, dtype=torch.uint8, device="cuda")[off:off + n].copy_(_dev(ring).reshape(-1))
    band = Guarded((K + 1) * C * C, torch.int64, 0, fill=0)
    for times in (1, 2):   # band accumulates: a second call doubles it
        GU.call("dl3_trimap_confusion", dp.data_ptr(), dl.data_ptr(), dr.data_ptr(), band.ptr(), B, H, W, C, _ints(widths), K)
        torch.cuda.synchronize()
        got = band.t.cpu().numpy().reshape(K + 1, C, C)
        assert np.array_equal(got, times * want), np.argwhere(got != times * want)[:5]
    assert band.guards_intact()
    assert np.array_equal(got.sum(0), 2 * TO.confusion(pred, lab, C))


@pytest.mark.parametrize("metric", [TO.CHEBYSHEV, TO.EUCLIDEAN])
def test_band_confusion_from_host_arrays_and_tensors(metric):
    """the Python surface end to end (rings and histogram on the device), numpy in and tensors in; integer labels outside
    0..C-1 become void"""
    import torch
    from dl3_amd import trimap
    i, wmax = 0, 32
    B, H, W, C = CASES[i]
    widths = _widths(wmax, True)
    lab, pred = _labels(i), _pred(i)
    want = TO.band_confusion(pred, lab, _want_rings(i, wmax, metric, 3), C, widths)
    lab255 = np.where(lab == C, 255, lab).astype(np.int64)   # VOC's void
    got = trimap.band_confusion(pred, lab255, C, widths, metric=metric)
    assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    again = trimap.band_confusion(torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(lab255).cuda(), C, widths,
                                  metric=metric, out=got)
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * want)
    assert np.array_equal(trimap.cumulative(got).cpu().numpy()[-1], 2 * TO.confusion(pred, lab, C))
    r = trimap.boundary_rings(lab255, C, wmax, metric=metric, seeds="edges")
    assert r.dtype == torch.uint8 and np.array_equal(r.cpu().numpy(), _want_rings(i, wmax, metric, 2))


# -------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_return_minus_one_and_write_nothing():
    import torch
    from dl3_amd import capi
    L = capi.lib()
    B, H, W, C = 2, 8, 12, 3
    n = B * H * W
    lab = torch.zeros(n, dtype=torch.float32, device="cuda")
    pred = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = Guarded(n, torch.uint8, 0)
    ws = Guarded(L.dl3_trimap_workspace_bytes(B, H, W), torch.uint8, 0)
    st = torch.cuda.current_stream().cuda_stream
    good_rings = good = dict(labels=lab.data_ptr(), rings=out.ptr(), workspace=ws.ptr(), B=B, H=H, W=W, C=C, wmax=4, metric=0,
                             seeds=3)
    bad = [dict(wmax=0), dict(wmax=255), dict(C=0), dict(C=256), dict(metric=2), dict(metric=-1), dict(seeds=0), dict(seeds=4),
           dict(B=0), dict(H=-1), dict(W=0), dict(B=4, H=32768, W=16384), dict(labels=None), dict(rings=None),
           dict(workspace=None), dict(workspace=ws.ptr() + 1)]
    for kw in bad:
        a = dict(good, **kw)
        assert L.dl3_trimap_rings(*a.values(), st) == -1, kw
    band = Guarded(3 * C * C, torch.int64, 0, fill=7)
    ring = torch.zeros(n, dtype=torch.uint8, device="cuda")
    good = dict(pred=pred.data_ptr(), labels=lab.data_ptr(), rings=ring.data_ptr(), band=band.ptr(), B=B, H=H, W=W, C=C,
                widths=_ints((1, 2)), K=2)
    bad = [dict(K=0), dict(K=9, widths=_ints(range(1, 10))), dict(widths=_ints((0, 2))), dict(widths=_ints((2, 2))),
           dict(widths=_ints((3, 2))), dict(widths=_ints((1, 255))), dict(widths=None), dict(C=0), dict(C=256), dict(B=0),
           dict(W=-3), dict(B=4, H=32768, W=16384), dict(pred=None), dict(labels=None), dict(rings=None), dict(band=None)]
    for kw in bad:
        a = dict(good, **kw)
        assert L.dl3_trimap_confusion(*a.values(), st) == -1, kw
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched() and band.untouched()
    # and the same buffers take a good call
    assert L.dl3_trimap_rings(*good_rings.values(), st) == 0
    torch.cuda.synchronize()
    assert (out.t == 5).all() and out.guards_intact()   # a constant batch has no seeds: wmax + 1 everywhere


# ----------------------------------------------------------------------------------------------------- graph capture
def test_launch_pair_is_capturable():
    """the two launches, captured once and replayed twice behind one eager run, triple a zeroed band: no allocation, no
    synchronisation in the calls (the chain is linear — no parallel branches)"""
    import torch
    from tests import gpu_util as GU
    from dl3_amd import capi
    i, wmax = 5, 32
    B, H, W, C = CASES[i]
    widths = _widths(wmax, True)
    lab, pred = _labels(i), _pred(i)
    want = TO.band_confusion(pred, lab, _want_rings(i, wmax, TO.EUCLIDEAN, 3), C, widths)
    dl, dp = _dev(lab, np.float32), _dev(pred)
    ring = torch.empty(B * H * W, dtype=torch.uint8, device="cuda")
    ws = torch.empty(capi.lib().dl3_trimap_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    band = torch.zeros(len(widths) + 1, C, C, dtype=torch.int64, device="cuda")
    cw = _ints(widths)

    def pair():
        GU.call("dl3_trimap_rings", dl.data_ptr(), ring.data_ptr(), ws.data_ptr(), B, H, W, C, wmax, 1, 3)
        GU.call("dl3_trimap_confusion", dp.data_ptr(), dl.data_ptr(), ring.data_ptr(), band.data_ptr(), B, H, W, C, cw,
                len(widths))
    pair()
    torch.cuda.synchronize()
    assert np.array_equal(band.cpu().numpy(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    torch.cuda.synchronize()
    assert np.array_equal(band.cpu().numpy(), want), "capturing must not run anything"
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(band.cpu().numpy(), 3 * want)


# ------------------------------------------------------------------------------------------------------- model level
def _model_data(C=3, size=64, n=5):
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (n, size, size, 3)).astype(np.float32)
    lab = TO.blobby(rng, n, size, size, C)
    lab[n - 2] = 1.0                       # a constant image
    lab[n - 1] = TO.corner(size, size)
    return x, lab


def _oracle_cumulative(masks, lab, C, widths, metric=TO.CHEBYSHEV, seeds=3):
    ring = TO.rings(lab, C, widths[-1], metric, seeds)
    return np.cumsum(TO.band_confusion(masks, lab, ring, C, widths), axis=0)


@pytest.mark.parametrize("head", ["original", "subpixel"])
def test_model_confusion_matrix_trimap(head):
    from tests.test_gpu_eval import _model
    from dl3_amd import utils as U
    C, widths = 3, (1, 2, 4, 8, 16, 32)
    model = _model("mobilenetv2", head, classes=C)
    x, lab = _model_data(C)
    y = lab.reshape(len(lab), -1, 1)
    masks = model.predict_mask(x, batch_size=2)
    want = _oracle_cumulative(masks, lab, C, widths)
    assert (np.diff(want.sum((1, 2)), prepend=0) > 0).all(), "an empty bin"
    got = model.confusion_matrix_trimap(x, y, batch_size=2)          # batches of 2, 2, 1
    assert got.dtype == np.int64 and got.shape == (7, C, C)
    assert np.array_equal(got[-1], model.confusion_matrix(x, y, batch_size=2))
    assert np.array_equal(got, want)

    class Gen:
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return x[2 * i:2 * i + 2], y[2 * i:2 * i + 2]
    assert np.array_equal(model.confusion_matrix_trimap(Gen()), want)
    eu = model.confusion_matrix_trimap(x, y, batch_size=2, widths=(3, 9), metric="euclidean", seeds="edges")
    assert np.array_equal(eu, _oracle_cumulative(masks, lab, C, (3, 9), TO.EUCLIDEAN, 2))
    # utils.trimap_iou: the same pass, with VOC's void in the labels, and the mIoU of every band
    lab255 = np.where(lab == C, 255, lab).astype(np.uint8)
    res = U.trimap_iou(model, x, lab255, nb_classes=C, batch_size=2)
    assert res["widths"] == widths and np.array_equal(res["confusion"], want)
    assert np.array_equal(res["miou"], U.iou_from_confusion(want)[1], equal_nan=True) and res["miou"].shape == (7,)
    # behind the dense CRF: the oracle on predict_mask(crf=True)'s masks
    crf_masks = model.predict_mask(x, batch_size=2, crf=True)
    res = U.trimap_iou(model, x, lab255, nb_classes=C, crf=True, batch_size=2)
    assert np.array_equal(res["confusion"], _oracle_cumulative(crf_masks, lab, C, widths))


def test_trimap_iou_from_masks_of_two_sizes():
    from dl3_amd import utils as U
    C, widths = 4, (1, 2, 4, 8)
    rng = np.random.default_rng(11)
    sizes = [(40, 56), (33, 47), (40, 56)]
    labs = [TO.blobby(rng, 1, h, w, C)[0] for h, w in sizes]
    labs[2] = TO.corner(*sizes[2])
    masks = [np.where(l == C, 0, np.roll(l, 2, axis=1)).astype(np.int32) for l in labs]
    want = sum(TO.band_confusion(m[None], l[None], TO.rings(l[None], C, 8), C, widths) for m, l in zip(masks, labs))
    assert (want.sum((1, 2)) > 0).all()
    res = U.trimap_iou_from_masks(masks, [np.where(l == C, 255, l) for l in labs], C, widths=widths)
    assert np.array_equal(res["confusion"], np.cumsum(want, axis=0)) and res["confusion"].dtype == np.int64
    assert np.array_equal(res["miou"], U.iou_from_confusion(np.cumsum(want, axis=0))[1], equal_nan=True)
    # an array of equally sized maps is one launch pair
    stacked = U.trimap_iou_from_masks(np.stack([masks[0], masks[2]]), np.stack([labs[0], labs[2]]), C, widths=widths)
    two = sum(TO.band_confusion(masks[k][None], labs[k][None], TO.rings(labs[k][None], C, 8), C, widths) for k in (0, 2))
    assert np.array_equal(stacked["confusion"], np.cumsum(two, axis=0))
