"""CPU tests of sliding-window inference: the window grid on cases computed by hand, the default stride,
the pyramid weights, the oracle (tests/slide_oracle.py) on cases that are right by inspection, its float32 run against its
float64 run, the argument checks that come before any device work, and the prototypes of include/dl3.h."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi
from dl3_amd import graph as G
from dl3_amd import slide
from dl3_amd import utils as U
from tests import slide_oracle as SO

# (image size, window, stride) -> (ny, nx, y origins, x origins), by hand:
#   23 / 16 / 11: ceil(7 / 11) + 1 = 2, origins 0, min(11, 7) = 7;   37 / 16 / 11: ceil(21 / 11) + 1 = 3: 0, 11, min(22, 21)
#   33 / 16 / 1: 17 + 1 = 18 windows at 0 .. 17;   5 x 7 under a 16 window: padded to 16 x 16, one window
#   100 / 64 / 42: ceil(36 / 42) + 1 = 2: 0, 36;   75 / 64 / 42: ceil(11 / 42) + 1 = 2: 0, 11
GRID_KATS = [
    ((16, 16), 16, 8, 1, 1, [0], [0]),
    ((23, 37), 16, 11, 2, 3, [0, 7], [0, 11, 21]),
    ((33, 16), 16, (1, 16), 18, 1, list(range(18)), [0]),
    ((5, 7), 16, 3, 1, 1, [0], [0]),
    ((100, 75), 64, 42, 2, 2, [0, 36], [0, 11]),
]


@pytest.mark.parametrize("size,win,stride,ny,nx,ys,xs", GRID_KATS)
def test_grid_known_answers(size, win, stride, ny, nx, ys, xs):
    got = slide.grid(size, (win, win), stride)
    assert got == (ny, nx, [(y, x) for y in ys for x in xs])
    assert SO.grid(size, (win, win), stride) == got
    origins = got[2]
    assert len(set(origins)) == len(origins) == ny * nx            # no duplicate windows
    cov = SO.coverage(size, (win, win), stride)
    assert cov.shape == tuple(size) and cov.min() >= 1             # every pixel is under a window
    for y0, x0 in origins:                                         # no window leaves the (padded) image
        assert 0 <= y0 <= max(size[0], win) - win and 0 <= x0 <= max(size[1], win) - win


@pytest.mark.parametrize("size", [(1, 1), (16, 17), (17, 16), (31, 47), (48, 48), (49, 33), (64, 200)])
@pytest.mark.parametrize("stride", [1, 5, 10, 16, (3, 16)])
def test_grid_covers_every_pixel_without_duplicates(size, stride):
    ny, nx, origins = slide.grid(size, (16, 16), stride)
    assert (ny, nx, origins) == SO.grid(size, (16, 16), stride)
    assert len(set(origins)) == len(origins) == ny * nx
    assert SO.coverage(size, (16, 16), stride).min() >= 1
    assert origins == sorted(origins)                              # k order is row-major


def test_default_stride():
    assert slide.default_stride((64, 64)) == (42, 42) == SO.default_stride((64, 64))
    assert slide.default_stride((512, 512)) == (341, 341) == SO.default_stride((512, 512))
    assert slide.default_stride((1, 1)) == (1, 1)
    assert slide.default_stride((320, 64)) == (213, 42)
    assert slide.grid((100, 75), (64, 64)) == slide.grid((100, 75), (64, 64), 42)


def test_pyramid_weights():
    assert slide.pyramid_weights(4) == [1, 2, 2, 1] == list(SO.pyramid(4))
    assert slide.pyramid_weights(5) == [1, 2, 3, 2, 1] == list(SO.pyramid(5))
    w = SO.weights((4, 5), "pyramid", np.float32)
    assert w.dtype == np.float32 and np.array_equal(w, np.outer([1, 2, 2, 1], [1, 2, 3, 2, 1]))
    assert np.array_equal(SO.weights((4, 5), "uniform", np.float32), np.ones((4, 5)))


# ------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_gather_is_the_crop_and_pads():
    rng = np.random.default_rng(0)
    im = rng.integers(0, 256, (23, 37, 3)).astype(np.uint8)
    g = SO.gather(im, (16, 16), 11)
    assert g.shape == (6, 16, 16, 3) and g.dtype == np.float32
    assert np.array_equal(g[5], im[7:23, 21:37].astype(np.float32))
    small = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    g = SO.gather(small, (16, 16), 3, pad_value=127.5)
    assert g.shape == (1, 16, 16, 3) and np.array_equal(g[0, :5, :7], small.astype(np.float32))
    assert np.all(g[0, 5:] == 127.5) and np.all(g[0, :, 7:] == 127.5)
    # a batch and a list are the images one behind the other
    both = SO.gather([im, small], (16, 16), 11)
    assert both.shape == (7, 16, 16, 3) and np.array_equal(both[6], SO.gather(small, (16, 16), 11)[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("blend", ["uniform", "pyramid"])
def test_oracle_constant_rows_stay_constant(dtype, blend):
    # 0.25, 0.5, 0.125: w p and the sums are exact in either precision, and so is the quotient
    row = np.array([0.25, 0.5, 0.125, 0.125], dtype)
    for size, stride in (((23, 37), 11), ((5, 7), 3), ((33, 16), (1, 16)), ((16, 16), 8)):
        n = len(SO.grid(size, (16, 16), stride)[2])
        p = np.broadcast_to(row, (n, 16, 16, 4))
        out = SO.blend(p, size, (16, 16), stride, blend, dtype)
        assert out.dtype == dtype and out.shape == size + (4,)
        assert np.array_equal(out, np.broadcast_to(row, size + (4,)))


def test_oracle_two_half_overlapping_windows():
    """a 1 x 6 image under 1 x 4 windows at stride 2: windows at x = 0 and 2, columns 2 and 3 under both.
    window 0 carries p = 0.2, window 1 carries p = 0.6 (one class)"""
    p = np.stack([np.full((1, 4, 1), 0.2), np.full((1, 4, 1), 0.6)])
    assert SO.grid((1, 6), (1, 4), (1, 2)) == (1, 2, [(0, 0), (0, 2)])
    out = SO.blend(p, (1, 6), (1, 4), (1, 2), "uniform", np.float64)[0, :, 0]
    assert np.allclose(out, [0.2, 0.2, 0.4, 0.4, 0.6, 0.6], rtol=0, atol=1e-15)
    # pyramid: wx = 1 2 2 1; column 2 is window 0's c = 2 (w 2) and window 1's c = 0 (w 1): (2 * 0.2 + 0.6) / 3;
    # column 3 is window 0's c = 3 (w 1) and window 1's c = 1 (w 2): (0.2 + 2 * 0.6) / 3
    out = SO.blend(p, (1, 6), (1, 4), (1, 2), "pyramid", np.float64)[0, :, 0]
    assert np.allclose(out, [0.2, 0.2, 1.0 / 3, 1.4 / 3, 0.6, 0.6], rtol=0, atol=1e-15)
    acc, ws = SO.blend(p, (1, 6), (1, 4), (1, 2), "pyramid", np.float64, parts=True)
    assert np.array_equal(ws[0], [1, 2, 3, 3, 2, 1])


def test_oracle_single_uniform_window_returns_its_input_bit_for_bit():
    rng = np.random.default_rng(1)
    p = rng.random((1, 16, 16, 5)).astype(np.float32)
    p[0, 3, 4] = 0.0
    out = SO.blend(p, (16, 16), (16, 16), 8, "uniform", np.float32)
    assert np.array_equal(out.view(np.uint32), p[0].view(np.uint32))
    # an image smaller than the window: the image's part of the window
    out = SO.blend(p, (5, 7), (16, 16), 3, "uniform", np.float32)
    assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(p[0, :5, :7]).view(np.uint32))


CASES = [((16, 16), 16, 8), ((23, 37), 16, 11), ((9, 40), 16, (5, 16)), ((5, 7), 16, 3), ((33, 16), 16, (1, 16)),
         ((40, 41), 16, 10), ((40, 41), 16, 1), ((100, 75), 64, 42)]


@pytest.mark.parametrize("size,win,stride", CASES)
@pytest.mark.parametrize("blend", ["uniform", "pyramid"])
def test_float32_oracle_within_its_bound_of_the_float64_one(size, win, stride, blend):
    rng = np.random.default_rng(3)
    n = len(SO.grid(size, (win, win), stride)[2])
    p = rng.random((n, win, win, 5)).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    lo = SO.blend(p, size, (win, win), stride, blend, np.float32)
    hi = SO.blend(p, size, (win, win), stride, blend, np.float64)
    cov = SO.coverage(size, (win, win), stride)
    d = np.abs(lo.astype(np.float64) - hi).max(-1)
    bound = SO.blend_bound(cov, 1.0)
    print("%s window %d stride %s %s: up to %d windows, |f32 - f64| %.3e, bound %.3e .. %.3e" % (
        size, win, stride, blend, cov.max(), d.max(), bound.min(), bound.max()))
    assert np.all(d <= bound)
    assert np.abs(hi.sum(-1) - 1).max() < 1e-6      # float32 inputs normalised in float32


# ------------------------------------------------------------------------------------------------------ arguments
def _hand_built():
    G.clear_session()
    inp = G.Input(shape=(32, 32, 3))
    x = G.Conv2D(4, (1, 1), padding="same", name="c")(inp)
    x = G.Reshape((32 * 32, 4))(x)
    x = G.Activation("softmax")(x)
    return G.Model(inp, x)


X = np.zeros((2, 40, 50, 3), np.float32)


@pytest.mark.parametrize("stride", [0, 33, (1, 0), (33, 1), -1, (1, 2, 3), 1.5, "a"])
def test_bad_stride_is_refused(stride):
    with pytest.raises(ValueError, match="stride"):
        _hand_built().predict_sliding(X, stride=stride)
    with pytest.raises(ValueError, match="stride"):
        slide.grid((40, 50), (32, 32), stride)


def test_blend_output_and_batch_size_are_checked():
    m = _hand_built()
    with pytest.raises(ValueError, match="blend"):
        m.predict_sliding(X, blend="gauss")
    with pytest.raises(ValueError, match="output"):
        m.predict_sliding(X, output="logits")
    for bad in (0, -4, 2.5, None):
        with pytest.raises(ValueError, match="batch_size"):
            m.predict_sliding(X, batch_size=bad)


def test_x_is_checked_before_any_device_work():
    m = _hand_built()
    for bad in (X[:0], X[0], X[..., :1], np.zeros((2, 0, 50, 3), np.float32), np.zeros((1, 2, 40, 50, 3), np.float32)):
        with pytest.raises(ValueError, match="x must"):
            m.predict_sliding(bad)
    for bad in ([], (), [X], [X[0], X[0, :, :, :2]], [np.zeros((0, 4, 3), np.uint8)]):
        with pytest.raises(ValueError, match="x must"):
            m.predict_sliding(bad)


def test_calculate_iou_sliding_refuses_output():
    with pytest.raises(ValueError, match="output"):
        U.calculate_iou_sliding(_hand_built(), X, np.zeros((2, 40, 50), np.int64), nb_classes=4, output="probs")


def test_window_list_and_chunks():
    # (100, 75) under 64 at stride 42 has 4 windows: three images give 12, cut 5, 5, 2 across the images
    wl = slide.window_list([(100, 75)] * 3, (64, 64), (42, 42))
    assert wl == [(i, k) for i in range(3) for k in range(4)]
    ch = slide.chunks(wl, 5)
    assert [len(c) for c in ch] == [5, 5, 2]
    assert slide._runs(ch[0]) == [[0, 0, 4, 0], [1, 0, 1, 4]]
    assert slide._runs(ch[1]) == [[1, 1, 3, 0], [2, 0, 2, 3]]
    assert slide._runs(ch[2]) == [[2, 2, 2, 0]]
    assert [len(c) for c in slide.chunks(wl, 32)] == [12]          # min(batch_size, n), as predict()


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_slide_entry_points():
    protos = capi.parse_header()
    ret, args = protos["dl3_slide_gather"]
    assert ret == "int" and [n for _, n in args] == ["src", "src_dtype", "Hi", "Wi", "H", "W", "sh", "sw", "k0", "nw", "pad_value",
                                                     "dst", "stream"]
    ret, args = protos["dl3_slide_accumulate"]
    assert ret == "int" and [n for _, n in args] == ["probs", "acc", "wsum", "Hi", "Wi", "H", "W", "C", "sh", "sw", "k0", "nw",
                                                     "blend", "stream"]
    ret, args = protos["dl3_slide_finalize"]
    assert ret == "int" and [n for _, n in args] == ["acc", "wsum", "probs_out", "mask_out", "Hi", "Wi", "H", "W", "C", "sh", "sw",
                                                     "blend", "stream"]
    names = ("dl3_slide_gather", "dl3_slide_accumulate", "dl3_slide_finalize")
    assert all(t in capi._CTYPES for name in names for t, _ in protos[name][1])
    assert slide.BLENDS == {"uniform": 0, "pyramid": 1} and (slide.F32, slide.U8) == (0, 1)
    src = open(capi.HEADER).read()
    assert "#define DL3_SLIDE_UNIFORM 0" in src and "#define DL3_SLIDE_PYRAMID 1" in src


def test_library_exports_the_slide_entry_points(lib):
    for name in ("dl3_slide_gather", "dl3_slide_accumulate", "dl3_slide_finalize"):
        assert getattr(lib, name).restype is not None
