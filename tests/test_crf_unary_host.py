"""CPU tests of the softmax-unary feature: unary_from_softmax (package and oracle) against hand-computed values, the
oracle's three gathers (tests/crf_unary_oracle.py) on cases that are right by inspection and against oracle/'s own
operators, the argument checks of the Python surface, and the three new prototypes of include/dl3.h."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi
from dl3_amd import crf as C
from oracle import dl3_oracle as DO
from tests import crf_unary_oracle as UO

# 2 classes, 3 pixels: a sure pixel, an even one, one under the clip
SM = np.array([[0.9, 0.5, 1e-7],
               [0.1, 0.5, 1.0 - 1e-7]])


def _both(scale, clip):
    got = C.unary_from_softmax(SM, scale=scale, clip=clip)
    assert got.dtype == np.float32 and got.shape == (2, 3)
    o64 = UO.unary_from_softmax(SM, scale, clip, np.float64)
    o32 = UO.unary_from_softmax(SM, scale, clip, np.float32)
    assert o64.dtype == np.float64 and o32.dtype == np.float32 and o64.shape == o32.shape == (2, 3)
    return got, o64, o32


def test_unary_from_softmax_default_clips_at_1e_5():
    want = -np.log(np.array([[0.9, 0.5, 1e-5], [0.1, 0.5, 1.0 - 1e-7]]))
    for u in _both(None, 1e-5):
        assert np.allclose(u, want, rtol=1e-6, atol=1e-7)
    assert abs(float(C.unary_from_softmax(SM)[0, 2]) - 11.512925) < 1e-5


def test_unary_from_softmax_without_clip():
    want = -np.log(SM)
    for u in _both(None, None):
        assert np.allclose(u, want, rtol=1e-6, atol=1e-7)
    assert abs(float(C.unary_from_softmax(SM, clip=None)[0, 2]) - 16.118096) < 1e-5
    # an unclipped zero costs +inf, in the package and in both runs of the oracle
    z = np.array([[0.0, 1.0], [1.0, 0.0]])
    assert np.isinf(C.unary_from_softmax(z, clip=None)[0, 0])
    assert np.isinf(UO.unary_from_softmax(z, None, None, np.float32)[1, 1])


def test_unary_from_softmax_scale_mixes_with_the_uniform_distribution():
    # scale 0.5, C = 2: p -> 0.5 p + 0.25
    want = -np.log(np.array([[0.7, 0.5, 0.25 + 0.5e-7], [0.3, 0.5, 0.75 - 0.5e-7]]))
    for u in _both(0.5, 1e-5):
        assert np.allclose(u, want, rtol=1e-6, atol=1e-7)
    for u in _both(0.5, None):   # nothing is under the clip once mixed
        assert np.allclose(u, want, rtol=1e-6, atol=1e-7)


def test_unary_from_softmax_flattens_trailing_axes():
    sm = np.random.default_rng(0).random((3, 4, 5))
    sm /= sm.sum(0)
    got = C.unary_from_softmax(sm)
    assert got.shape == (3, 20) and got.dtype == np.float32
    assert np.allclose(got, -np.log(sm).reshape(3, 20), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ oracle gathers
def test_gather_bilinear_identity_constant_and_oracle_rule():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 5, 7, 3))
    assert np.array_equal(UO.gather_bilinear(x, 5, 7), x)                       # Hi = Ho: the identity
    assert np.array_equal(UO.gather_bilinear(x.astype(np.float32), 5, 7, np.float32), x.astype(np.float32))
    const = np.broadcast_to(np.array([1.5, -2.0, 7.0]), (1, 3, 4, 3))
    up = UO.gather_bilinear(const, 11, 9)
    assert up.shape == (1, 11, 9, 3) and np.array_equal(up, np.broadcast_to(const[:, :1, :1], up.shape))
    # exact integer factor: the legacy rule repeats the source pixel at the multiples and interpolates between them
    row = np.arange(4.0).reshape(1, 1, 4, 1)
    assert np.allclose(UO.gather_bilinear(row, 1, 8)[0, 0, :, 0], [0, .5, 1, 1.5, 2, 2.5, 3, 3])
    # the float32 run's coordinates are oracle/'s, and the float64 run agrees with oracle/'s operator to float32's
    # coordinate rounding
    for out_size, in_size in ((17, 3), (33, 5), (65, 9), (64, 8), (7, 1)):
        lo, hi, w = UO.lerp_coords(out_size, in_size, np.float32)
        lo0, hi0, w0 = DO._tf1_lerp(out_size, in_size)
        assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0) and np.array_equal(w, w0)
    x = rng.standard_normal((2, 9, 9, 4))
    assert np.abs(UO.gather_bilinear(x, 65, 65) - DO.resize_bilinear_tf1(x, 65, 65)).max() < 1e-5


def test_gather_shuffle_identity_constant_and_oracle_rule():
    rng = np.random.default_rng(2)
    u = rng.standard_normal((2, 3, 4, 5))
    assert np.array_equal(UO.gather_shuffle(u, 1), u)                             # r = 1: the identity
    const = np.broadcast_to(np.repeat(np.array([3.0, -1.0]), 16), (1, 2, 3, 32))  # every phase of a class equal
    out = UO.gather_shuffle(const, 4)
    assert out.shape == (1, 8, 12, 2) and np.array_equal(out, np.broadcast_to(np.array([3.0, -1.0]), out.shape))
    # one pixel, one class, r = 2: element p*r + q lands at row q, column p — not depth_to_space's row-major phases
    one = np.arange(4.0).reshape(1, 1, 1, 4)
    assert np.array_equal(UO.gather_shuffle(one, 2)[0, :, :, 0], [[0, 2], [1, 3]])
    u = rng.standard_normal((2, 5, 3, 2 * 16))
    assert np.array_equal(UO.gather_shuffle(u, 4), DO.phase_shift(u, 4))


def test_gather_plain_and_whole_unary():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((2, 6, 3))
    assert np.array_equal(UO.gather_plain(z), z)
    U = UO.unary("plain", z, None, clip=None)
    assert U.shape == (2, 3, 6)
    p = np.exp(-U)
    assert np.allclose(p.sum(1), 1.0, atol=1e-12) and np.array_equal(U.argmin(1), z.argmax(-1))
    # probabilities in = logits in
    assert np.allclose(UO.unary("plain", np.exp(-U).transpose(0, 2, 1), None, is_prob=True, clip=None), U, atol=1e-12)
    # a constant low-resolution field stays constant through either resampling form
    lo = np.broadcast_to(np.array([0.5, -1.0, 2.0]), (1, 3, 3, 3))
    assert np.allclose(UO.unary("bilinear", lo, (7, 5)), UO.unary("plain", lo.reshape(1, 9, 3), None)[:, :, :1])
    sh = np.broadcast_to(np.repeat(np.array([0.5, -1.0, 2.0]), 4), (1, 2, 2, 12))
    assert np.allclose(UO.unary("shuffle", sh, 2), UO.unary("plain", lo.reshape(1, 9, 3), None)[:, :, :1])


# ------------------------------------------------------------------------------------------------ Python surface
def test_predict_mask_rejects_an_unknown_unary():
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone="mobilenetv2", OS=16)
    x = np.zeros((1, 64, 64, 3), np.float32)
    with pytest.raises(ValueError, match="crf_unary"):
        model.predict_mask(x, crf=True, crf_unary="bogus")


def test_dense_crf_softmax_wants_exactly_one_score_tensor():
    im = np.zeros((1, 4, 4, 3), np.uint8)
    p = np.full((1, 4, 4, 2), 0.5, np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        C.dense_crf_softmax(im)
    with pytest.raises(ValueError, match="exactly one"):
        C.dense_crf_softmax(im, probs=p, logits=p)


def test_softmax_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls succeed there, tests/test_gpu_crf_unary.py covers them")
    from dl3_amd import utils as U
    im = np.zeros((1, 4, 4, 3), np.uint8)
    p = np.full((1, 4, 4, 2), 0.5, np.float32)
    with pytest.raises(capi.DL3Error):
        C.dense_crf_softmax(im, probs=p)
    with pytest.raises(capi.DL3Error):
        U.do_crf_softmax(im[0], p[0])


def test_header_declares_the_unary_entry_points():
    protos = capi.parse_header()
    tail = [("float", "scale"), ("float", "clip"), ("void *", "stream")]
    for name in ("dl3_crf_unary_plain", "dl3_crf_unary_bilinear", "dl3_crf_unary_shuffle"):
        ret, args = protos[name]
        assert ret == "int" and args[-3:] == tail, (name, args)
    assert [a for _, a in protos["dl3_crf_unary_plain"][1]] == ["x", "is_prob", "U", "B", "N", "C", "scale", "clip", "stream"]
    assert [a for _, a in protos["dl3_crf_unary_bilinear"][1]][:8] == ["logits_lo", "U", "B", "Hi", "Wi", "Ho", "Wo", "C"]
    assert [a for _, a in protos["dl3_crf_unary_shuffle"][1]][:7] == ["u", "U", "B", "H", "W", "C", "r"]
