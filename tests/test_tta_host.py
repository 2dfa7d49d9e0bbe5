"""CPU tests of multi-scale / flip inference: pass sizes and order, the argument checks that come before
any device work, the rebuild closures and what building a sibling leaves behind, the oracle (tests/tta_oracle.py) on
cases that are right by inspection, its float32 run against its float64 run, and the prototypes of include/dl3.h."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi
from dl3_amd import graph as G
from dl3_amd import tta
from dl3_amd.deeplabv3p import Deeplabv3
from dl3_amd.utils import SegModel
from tests import tta_oracle as TO

SIZES = {64: (32, 48, 64, 80, 96, 112), 320: (160, 240, 320, 400, 480, 560), 512: (256, 384, 512, 640, 768, 896),
         513: (256, 384, 513, 640, 768, 896)}


@pytest.mark.parametrize("H", sorted(SIZES))
def test_scaled_size_at_the_default_scales(H):
    assert tta.DEFAULT_SCALES == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    assert tuple(tta.scaled_size(H, s) for s in tta.DEFAULT_SCALES) == SIZES[H]
    assert tuple(TO.scaled_size(H, s) for s in tta.DEFAULT_SCALES) == SIZES[H]
    assert tta.scaled_size(H, 1) == H and tta.scaled_size(H, 1.0) == H


def test_scaled_size_floor_and_rounding():
    assert tta.scaled_size(64, 0.1) == 16          # never under 16
    assert tta.scaled_size(40, 0.6) == 32          # 24 / 16 = 1.5: halves go up
    assert tta.scaled_size(513, 1.0) == 513        # s == 1 is the model's own extent, stride-friendly or not


def test_pass_order_and_count():
    p = tta.pass_list((64, 320), tta.DEFAULT_SCALES, True)
    assert len(p) == 12
    assert [q[0] for q in p] == [s for s in tta.DEFAULT_SCALES for _ in range(2)]
    assert [q[3] for q in p] == [False, True] * 6
    assert [(q[1], q[2]) for q in p[::2]] == list(zip(SIZES[64], SIZES[320]))
    q = tta.pass_list((64, 64), (1.5, 0.5), False)
    assert q == [(1.5, 96, 96, False), (0.5, 32, 32, False)]       # the order of `scales`, not sorted
    assert TO.pass_list((64, 320), tta.DEFAULT_SCALES, True) == p


def _hand_built():
    G.clear_session()
    inp = G.Input(shape=(32, 32, 3))
    x = G.Conv2D(4, (1, 1), padding="same", name="c")(inp)
    x = G.Reshape((32 * 32, 4))(x)
    x = G.Activation("softmax")(x)
    return G.Model(inp, x)


@pytest.mark.parametrize("scales", [(), (0.0,), (1.0, -0.5), (float("nan"),)])
def test_bad_scales_are_refused(scales):
    m = _hand_built()
    with pytest.raises(ValueError, match="scales"):
        m.predict_multiscale(np.zeros((1, 32, 32, 3), np.float32), scales=scales)
    with pytest.raises(ValueError, match="scales"):
        tta.pass_list((32, 32), scales, True)


def test_crf_needs_mask_output_and_output_is_checked():
    m = _hand_built()
    x = np.zeros((1, 32, 32, 3), np.float32)
    with pytest.raises(ValueError, match="crf"):
        m.predict_multiscale(x, scales=(1.0,), output="probs", crf=True)
    with pytest.raises(ValueError, match="output"):
        m.predict_multiscale(x, scales=(1.0,), output="logits")


def test_batch_size_and_x_are_checked_before_any_device_work():
    m = _hand_built()
    x = np.zeros((2, 32, 32, 3), np.float32)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="batch_size"):
            m.predict_multiscale(x, scales=(1.0,), batch_size=bad)
    for bad in (x[:0], x[:, :16], x[0], np.zeros((2, 32, 32, 1), np.float32)):
        with pytest.raises(ValueError, match="x must be"):
            m.predict_multiscale(bad, scales=(1.0,))


def test_hand_built_model_needs_a_factory():
    m = _hand_built()
    assert m._tta_rebuild is None
    with pytest.raises(ValueError, match="factory"):
        m.predict_multiscale(np.zeros((1, 32, 32, 3), np.float32), scales=(0.5, 1.0))


def test_rebuild_closure_is_recorded():
    G.clear_session()
    m = Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=5, backbone="mobilenetv2")
    assert callable(m._tta_rebuild)
    s = tta.sibling(m, 32, 48)
    assert s.input.shape == (32, 48, 3) and s.output.shape == (32 * 48, 5)
    assert tta.sibling(m, 32, 48) is s                      # built once, kept on the model
    m.clear_multiscale()
    assert tta.sibling(m, 32, 48) is not s
    for net in ("subpixel", "original"):
        G.clear_session()
        sm = SegModel(image_size=(64, 64)).create_seg_model(net, n=4)
        assert callable(sm._tta_rebuild)
        s = tta.sibling(sm, 96, 96)
        assert s.input.shape == (96, 96, 3) and s.output.shape == (96 * 96, 4)
        assert [l.kind for l in s.layers] == [l.kind for l in sm.layers]


def test_infer_models_keep_their_output_shape():
    G.clear_session()
    m = Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, infer=True)
    assert tta.sibling(m, 32, 32).output.shape == (32, 32, 3)


@pytest.mark.parametrize("kind", ["deeplab", "subpixel"])
def test_building_a_sibling_leaves_seed_stream_and_name_counters(kind):
    def make():
        if kind == "deeplab":
            return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=5, backbone="mobilenetv2")
        return SegModel(image_size=(64, 64)).create_seg_model("subpixel", n=4)

    def run(with_sibling):
        G.clear_session(seed=11)
        a = make()
        if with_sibling:
            tta.sibling(a, 32, 32)
            tta.sibling(a, 96, 96)
        b = make()
        return a, b

    a0, b0 = run(False)
    a1, b1 = run(True)
    for p, q in ((a0, a1), (b0, b1)):
        assert p.name == q.name and [l.name for l in p.layers] == [l.name for l in q.layers]
        wp, wq = p.get_weights(), q.get_weights()
        assert len(wp) == len(wq) and all(np.array_equal(u, v) for u, v in zip(wp, wq))
    # ... and the two constructions of one run do differ: the stream moved on between them
    assert any(not np.array_equal(u, v) for u, v in zip(a0.get_weights(), b0.get_weights()))


# ------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_linear_ramp_resizes_to_the_ramp():
    # weights are dyadic at 5 -> 9 and 3 -> 5: exact
    yy, xx = np.meshgrid(np.arange(5.0), np.arange(3.0), indexing="ij")
    src = (3.0 * yy - 2.0 * xx + 1.0)[None, :, :, None]
    out = TO.resize(src, 9, 5, np.float64)
    Y, X = np.meshgrid(np.arange(9) * 0.5, np.arange(5) * 0.5, indexing="ij")
    assert np.array_equal(out[0, :, :, 0], 3.0 * Y - 2.0 * X + 1.0)
    # any ratio: the ramp up to float64 roundoff
    yy, xx = np.meshgrid(np.arange(7.0), np.arange(11.0), indexing="ij")
    src = (3.0 * yy - 2.0 * xx + 1.0)[None, :, :, None]
    out = TO.resize(src, 17, 4, np.float64)
    Y, X = np.meshgrid(np.arange(17) * 6.0 / 16.0, np.arange(4) * 10.0 / 3.0, indexing="ij")
    assert np.abs(out[0, :, :, 0] - (3.0 * Y - 2.0 * X + 1.0)).max() < 1e-12
    # corners are kept: align_corners = True
    assert out[0, 0, 0, 0] == src[0, 0, 0, 0] and out[0, -1, -1, 0] == src[0, -1, -1, 0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_identity_constant_and_flip(dtype):
    rng = np.random.default_rng(0)
    src = rng.random((2, 7, 11, 3)).astype(dtype)
    assert np.array_equal(TO.resize(src, 7, 11, dtype), src)                      # same size: identity
    u8 = rng.integers(0, 256, (2, 7, 11, 3)).astype(np.uint8)
    assert np.array_equal(TO.resize_image(u8, 7, 11, False, dtype), u8.astype(dtype))
    const = np.full((1, 5, 6, 2), 0.3, dtype)
    assert np.array_equal(TO.resize(const, 13, 4, dtype), np.full((1, 13, 4, 2), 0.3, dtype))
    once = TO.resize_image(src, 7, 11, True, dtype)
    assert np.array_equal(once, src[:, :, ::-1])
    assert np.array_equal(TO.resize_image(once, 7, 11, True, dtype), src)          # flip twice: identity
    # a mirrored pass read mirrored is the plain pass
    assert np.array_equal(TO.accumulate(src[:, :, ::-1], None, 9, 13, True, True, 0, dtype),
                          TO.accumulate(src, None, 9, 13, False, True, 0, dtype))
    # degenerate extents
    one = rng.random((1, 1, 1, 2)).astype(dtype)
    assert np.array_equal(TO.resize(one, 4, 4, dtype), np.broadcast_to(one, (1, 4, 4, 2)))
    assert np.array_equal(TO.resize(src, 1, 1, dtype), src[:, :1, :1])


def test_oracle_probability_rows_stay_probability_rows():
    rng = np.random.default_rng(1)
    p = rng.random((2, 6, 5, 7))
    p /= p.sum(-1, keepdims=True)
    for Ho, Wo in ((12, 9), (3, 4), (6, 5)):
        q = TO.resize(p, Ho, Wo, np.float64)
        assert q.min() >= 0 and np.abs(q.sum(-1) - 1).max() < 1e-14


def test_oracle_accumulate_first_last():
    rng = np.random.default_rng(2)
    p = rng.random((1, 4, 4, 3))
    acc = rng.random((1, 8, 8, 3))
    v = TO.resize(p, 8, 8, np.float64)
    nan = np.full((1, 8, 8, 3), np.nan)
    assert np.array_equal(TO.accumulate(p, nan, 8, 8, False, True, 0, np.float64), v)     # first: acc is not read
    assert np.array_equal(TO.accumulate(p, acc, 8, 8, False, False, 0, np.float64), acc + v)
    assert np.array_equal(TO.accumulate(p, acc, 8, 8, False, False, 3, np.float64), (acc + v) / 3)
    assert np.array_equal(TO.accumulate(p, nan, 8, 8, False, True, 1, np.float64), v)     # a single pass: v / 1


CASES = [((8, 8), (16, 16)), ((3, 5), (17, 33)), ((9, 9), (4, 4)), ((7, 11), (7, 11)), ((1, 1), (4, 4)), ((5, 6), (1, 1)),
         ((32, 32), (64, 64)), ((96, 96), (64, 64)), ((56, 40), (64, 64))]


@pytest.mark.parametrize("si,so", CASES)
def test_float32_oracle_within_its_bound_of_the_float64_one(si, so):
    rng = np.random.default_rng(3)
    # probabilities: M = 1, neighbouring values differ by at most D = 1
    p = rng.random((2,) + si + (5,)).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    d = np.abs(TO.resize(p, so[0], so[1], np.float32).astype(np.float64) - TO.resize(p, so[0], so[1], np.float64)).max()
    bound = TO.resize_bound(si[0], si[1], 1.0, 1.0)
    print("probs %s -> %s: |f32 - f64| %.3e, bound %.3e" % (si, so, d, bound))
    assert d <= bound
    # raw pixels: M = D = 255
    im = rng.integers(0, 256, (2,) + si + (3,)).astype(np.uint8)
    d = np.abs(TO.resize_image(im, so[0], so[1], True, np.float32).astype(np.float64)
               - TO.resize_image(im, so[0], so[1], True, np.float64)).max()
    bound = TO.resize_bound(si[0], si[1], 255.0, 255.0)
    print("image %s -> %s: |f32 - f64| %.3e, bound %.3e" % (si, so, d, bound))
    assert d <= bound


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_tta_entry_points():
    protos = capi.parse_header()
    ret, args = protos["dl3_tta_resize_image"]
    assert ret == "int" and [n for _, n in args] == ["src", "src_dtype", "dst", "B", "Hi", "Wi", "Ho", "Wo", "flip", "stream"]
    ret, args = protos["dl3_tta_accumulate"]
    assert ret == "int" and [n for _, n in args] == ["probs", "acc", "B", "Hi", "Wi", "Ho", "Wo", "C", "flip", "first",
                                                     "n_passes_if_last", "stream"]
    assert all(t in capi._CTYPES for name in ("dl3_tta_resize_image", "dl3_tta_accumulate") for t, _ in protos[name][1])
    assert (tta.F32, tta.U8) == (0, 1)
    src = open(capi.HEADER).read()
    assert "#define DL3_TTA_F32 0" in src and "#define DL3_TTA_U8 1" in src
