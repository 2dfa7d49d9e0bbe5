"""CPU: the trimap definitions — the numpy oracle against scipy's distance transforms and against maps
worked out by hand, the host arithmetic (cumulative, iou_from_confusion), every ValueError of the Python surface, and the
header's declarations.  Nothing here needs a GPU."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi, trimap
from dl3_amd import utils as U
from tests import trimap_oracle as TO

METRICS = (TO.CHEBYSHEV, TO.EUCLIDEAN)


# ------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("shape,C", [((3, 37, 53), 21), ((2, 5, 130), 4), ((1, 1, 40), 3), ((1, 40, 1), 3), ((2, 64, 64), 33)])
def test_oracle_agrees_with_scipy(shape, C):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    lab = TO.blobby(rng, *shape, C)
    lab[-1] = TO.corner(*shape[1:])
    for seeds in (1, 2, 3):
        seed = TO.seeds_of(lab, C, seeds)
        for wmax in (1, 4, 32, 254):
            got_c, got_e = TO.rings_from_seeds(seed, wmax, TO.CHEBYSHEV), TO.rings_from_seeds(seed, wmax, TO.EUCLIDEAN)
            for b in range(shape[0]):
                if not seed[b].any():
                    assert (got_c[b] == wmax + 1).all() and (got_e[b] == wmax + 1).all()
                    continue
                cdt = ndi.distance_transform_cdt(~seed[b], metric="chessboard")
                d2 = np.rint(ndi.distance_transform_edt(~seed[b]) ** 2).astype(np.int64)
                assert np.array_equal(got_c[b], np.minimum(cdt, wmax + 1))
                assert np.array_equal(got_e[b], np.minimum(TO.ceil_root(d2), wmax + 1))


def test_ceil_root_is_exact():
    d2 = np.arange(0, 2 * 254 * 254 + 2)
    r = TO.ceil_root(d2)
    assert (r * r >= d2).all() and ((r == 0) | ((r - 1) * (r - 1) < d2)).all()


def test_seed_rules_by_hand():
    lab = np.array([[[0, 0, 1, 1],
                     [0, 0, 1, 1],
                     [0, 2, 0, 0]]], np.float32)   # C = 2: the 2 is void
    void = np.zeros((1, 3, 4), bool)
    void[0, 2, 1] = True
    assert np.array_equal(TO.seeds_of(lab, 2, TO.SEED_VOID), void)
    edges = np.array([[[0, 1, 1, 0],
                       [0, 1, 1, 1],
                       [1, 1, 1, 1]]], bool)     # both sides of every edge; void counts as a value
    assert np.array_equal(TO.seeds_of(lab, 2, TO.SEED_EDGES), edges)
    assert np.array_equal(TO.seeds_of(lab, 2, 3), edges | void)
    # images never see each other's pixels: two constant images of different classes have no seeds
    two = np.stack([np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32)])
    assert not TO.seeds_of(two, 2, 3).any()
    # labels outside 0..C-1 are void
    assert np.array_equal(TO.canon(np.array([-1.0, 0.0, 1.0, 2.0, 255.0]), 2), [2, 0, 1, 2, 2])


def test_rings_by_hand():
    # one seed pixel in a 5 x 7 map
    seed = np.zeros((1, 5, 7), bool)
    seed[0, 2, 3] = True
    cheb = np.array([[3, 2, 2, 2, 2, 2, 3],
                     [3, 2, 1, 1, 1, 2, 3],
                     [3, 2, 1, 0, 1, 2, 3],
                     [3, 2, 1, 1, 1, 2, 3],
                     [3, 2, 2, 2, 2, 2, 3]])
    assert np.array_equal(TO.rings_from_seeds(seed, 8, TO.CHEBYSHEV)[0], cheb)
    eucl = np.array([[4, 3, 3, 2, 3, 3, 4],     # ceil(sqrt(13)) = 4, ceil(sqrt(8)) = 3, ceil(sqrt(5)) = 3
                     [4, 3, 2, 1, 2, 3, 4],     # ceil(sqrt(10)) = 4, ceil(sqrt(2)) = 2
                     [3, 2, 1, 0, 1, 2, 3],
                     [4, 3, 2, 1, 2, 3, 4],
                     [4, 3, 3, 2, 3, 3, 4]])
    assert np.array_equal(TO.rings_from_seeds(seed, 8, TO.EUCLIDEAN)[0], eucl)
    # the clamp: everything above wmax reads wmax + 1
    assert np.array_equal(TO.rings_from_seeds(seed, 2, TO.CHEBYSHEV)[0], np.minimum(cheb, 3))
    assert np.array_equal(TO.rings_from_seeds(seed, 2, TO.EUCLIDEAN)[0], np.minimum(eucl, 3))
    # a 1-pixel-wide vertical line: the distance is the column distance under both metrics
    line = np.zeros((1, 4, 6), bool)
    line[0, :, 1] = True
    for m in METRICS:
        assert np.array_equal(TO.rings_from_seeds(line, 9, m)[0], np.tile([1, 0, 1, 2, 3, 4], (4, 1)))
    # a seed on the border (the corner): nothing wraps
    c = np.zeros((1, 3, 4), bool)
    c[0, 0, 0] = True
    assert np.array_equal(TO.rings_from_seeds(c, 9, TO.CHEBYSHEV)[0], [[0, 1, 2, 3], [1, 1, 2, 3], [2, 2, 2, 3]])
    assert np.array_equal(TO.rings_from_seeds(c, 9, TO.EUCLIDEAN)[0], [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 3, 4]])
    # H = 1 and W = 1
    row = np.zeros((1, 1, 6), bool)
    row[0, 0, 4] = True
    for m in METRICS:
        assert np.array_equal(TO.rings_from_seeds(row, 3, m)[0], [[4, 3, 2, 1, 0, 1]])
        assert np.array_equal(TO.rings_from_seeds(row.transpose(0, 2, 1), 3, m)[0], [[4], [3], [2], [1], [0], [1]])
    # an image without seeds is wmax + 1 everywhere, next to one that has a seed
    both = np.concatenate([np.zeros((1, 5, 7), bool), seed])
    for m in METRICS:
        r = TO.rings_from_seeds(both, 8, m)
        assert (r[0] == 9).all() and r[1, 2, 3] == 0 and r.dtype == np.uint8


def test_bins_and_band_confusion_by_hand():
    assert np.array_equal(TO.bins_of([0, 1, 2, 3, 4, 5, 9], (1, 2, 4)), [0, 0, 1, 2, 2, 3, 3])
    lab = np.array([[[0, 1, 2, 1]]], np.float32)     # C = 2: the third pixel is void
    pred = np.array([[[0, 0, 1, 2]]])                 # the last prediction is out of range
    ring = np.array([[[0, 3, 0, 1]]])
    band = TO.band_confusion(pred, lab, ring, 2, (1, 2))
    want = np.zeros((3, 2, 2), np.int64)
    want[0, 0, 0] = 1      # ring 0 -> bin 0
    want[2, 1, 0] = 1      # ring 3 -> beyond
    assert np.array_equal(band, want)
    assert np.array_equal(band.sum(0), TO.confusion(pred, lab, 2))


# ---------------------------------------------------------------------------------------------- the host arithmetic
def test_cumulative_and_iou_from_confusion():
    band = np.array([[[1, 0], [2, 3]], [[0, 4], [0, 0]], [[5, 0], [0, 0]]])
    cum = trimap.cumulative(band)
    assert cum.dtype == np.int64 and np.array_equal(cum, [[[1, 0], [2, 3]], [[1, 4], [2, 3]], [[6, 4], [2, 3]]])
    with pytest.raises(ValueError):
        trimap.cumulative(np.zeros((2, 2)))
    conf = np.array([[6, 4, 0], [2, 3, 0], [0, 0, 0]])   # class 2 never occurs: union 0
    iou, mean = U.iou_from_confusion(conf)
    assert iou[0] == 6 / 12 and iou[1] == 3 / 9 and np.isnan(iou[2])
    assert mean == pytest.approx((6 / 12 + 3 / 9) / 2, rel=1e-15)
    # the plain layout, not calculate_iou's rolled one; leading axes are kept
    iou3, mean3 = U.iou_from_confusion(np.stack([conf, np.zeros((3, 3)), conf.T]))
    assert iou3.shape == (3, 3) and mean3.shape == (3,)
    assert np.array_equal(iou3[0], iou, equal_nan=True) and np.isnan(iou3[1]).all() and np.isnan(mean3[1])
    assert mean3[0] == mean and mean3[2] == pytest.approx(mean, rel=1e-15)
    with pytest.raises(ValueError):
        U.iou_from_confusion(np.zeros((2, 3)))


# ------------------------------------------------------------------------------------------------- argument errors
LAB = np.zeros((1, 4, 4), np.float32)


@pytest.mark.parametrize("kw", [
    dict(wmax=0), dict(wmax=255), dict(wmax=1.5), dict(wmax="3"), dict(n_classes=0), dict(n_classes=256),
    dict(metric="manhattan"), dict(metric=0), dict(seeds=()), dict(seeds=("void", "corners")), dict(seeds=3),
    dict(labels=np.zeros((4,), np.float32)), dict(labels=np.zeros((1, 0, 4), np.float32)),
    dict(labels=np.zeros((1, 1, 4, 4), np.float32)), dict(labels=np.array([["a"]])),
], ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()).replace(" ", ""))
def test_boundary_rings_refuses(kw):
    args = dict(labels=LAB, n_classes=3, wmax=4)
    args.update(kw)
    with pytest.raises(ValueError):
        trimap.boundary_rings(**args)


@pytest.mark.parametrize("kw", [
    dict(widths=()), dict(widths=(0, 1)), dict(widths=(2, 2)), dict(widths=(3, 2)), dict(widths=(1, 255)),
    dict(widths=tuple(range(1, 10))), dict(widths=(1.5,)), dict(widths=4), dict(metric="l2"), dict(seeds="edge"),
    dict(n_classes=300), dict(pred=np.zeros((1, 4, 5), np.int32)), dict(pred=np.zeros((2, 4, 4), np.int32)),
    dict(out=np.zeros((3, 3, 3), np.int64)),
], ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()).replace(" ", ""))
def test_band_confusion_refuses(kw):
    args = dict(pred=np.zeros((1, 4, 4), np.int32), labels=LAB, n_classes=3, widths=(1, 2))
    args.update(kw)
    with pytest.raises(ValueError):
        trimap.band_confusion(**args)


def test_checks_return_the_launch_arguments():
    assert trimap.check_widths([1, 2, 4]) == (1, 2, 4) and trimap.check_widths(np.array([3, 254])) == (3, 254)
    assert trimap.check_metric("chebyshev") == 0 and trimap.check_metric("euclidean") == 1
    assert trimap.check_seeds("void") == 1 and trimap.check_seeds(["edges"]) == 2 and trimap.check_seeds(("void", "edges")) == 3
    assert trimap.DEFAULT_WIDTHS == (1, 2, 4, 8, 16, 32)


def test_model_level_functions_refuse_before_device_work():
    class NoDevice:   # any device work would need one of these
        class output:
            shape = (4, 4, 3)

        def __getattr__(self, name):
            raise AssertionError("touched the model: %s" % name)
    lab = np.zeros((1, 4, 4))
    for kw in (dict(widths=(2, 1)), dict(metric="l1"), dict(seeds=("none",))):
        with pytest.raises(ValueError):
            U.trimap_iou(NoDevice(), np.zeros((1, 4, 4, 3)), lab, nb_classes=3, **kw)
        with pytest.raises(ValueError):
            U.trimap_iou_from_masks(lab, lab, 3, **kw)
        with pytest.raises(ValueError):
            dl3_amd.graph.Model.confusion_matrix_trimap(NoDevice(), np.zeros((1, 4, 4, 3)), lab, **kw)
    with pytest.raises(ValueError):
        U.trimap_iou_from_masks([np.zeros((4, 4)), np.zeros((3, 4))], [np.zeros((4, 4)), np.zeros((4, 4))], 3)
    with pytest.raises(ValueError):
        U.trimap_iou_from_masks([], [], 3)


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_trimap_entry_points():
    protos = capi.parse_header()
    assert protos["dl3_trimap_workspace_bytes"] == ("size_t", [("int", "B"), ("int", "H"), ("int", "W")])
    ret, args = protos["dl3_trimap_rings"]
    assert ret == "int" and [n for _, n in args] == ["labels", "rings", "workspace", "B", "H", "W", "C", "wmax", "metric",
                                                     "seeds", "stream"]
    assert args[1][0] == "unsigned char *"
    ret, args = protos["dl3_trimap_confusion"]
    assert ret == "int" and [n for _, n in args] == ["pred", "labels", "rings", "band", "B", "H", "W", "C", "widths", "K",
                                                     "stream"]
    names = ("dl3_trimap_workspace_bytes", "dl3_trimap_rings", "dl3_trimap_confusion")
    assert all(t in capi._CTYPES for name in names for t, _ in protos[name][1])
    src = open(capi.HEADER).read()
    for line in ("#define DL3_TRIMAP_CHEBYSHEV 0", "#define DL3_TRIMAP_EUCLIDEAN 1", "#define DL3_TRIMAP_SEED_VOID 1",
                 "#define DL3_TRIMAP_SEED_EDGES 2"):
        assert line in src
    assert trimap.METRICS == {"chebyshev": 0, "euclidean": 1} and trimap.SEEDS == {"void": 1, "edges": 2}


def test_library_exports_the_trimap_entry_points(lib):
    for name in ("dl3_trimap_workspace_bytes", "dl3_trimap_rings", "dl3_trimap_confusion"):
        assert hasattr(lib, name)
    # the sizing query is host arithmetic: rows padded to 4 bytes; 0 for sizes the kernels refuse
    assert lib.dl3_trimap_workspace_bytes(3, 37, 53) == 3 * 37 * 56
    assert lib.dl3_trimap_workspace_bytes(1, 1, 1) == 4
    assert lib.dl3_trimap_workspace_bytes(0, 4, 4) == 0 and lib.dl3_trimap_workspace_bytes(2, 32768, 32768) == 0
