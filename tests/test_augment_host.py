"""CPU tests of the training augmentation: the seeded parameter stream against a hand-written replay of the reference's
call order (utils.py:319-350), the train / validation split (utils.py:268-276), known answers of the numpy oracle
(tests/aug_oracle.py) and cross-checks of the oracle against scipy.ndimage."""
import random

import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import augment as A
from dl3_amd.utils import SegModel, SegmentationGenerator
from tests import aug_oracle as O

NOTEBOOK_TRAIN = dict(blur=5, horizontal_flip=True, brightness=0.3, zoom=0.1)
NOTEBOOK_VALID = dict(brightness=.1, zoom=.05)


def _replay(seed, n, blur=0, crop=None, src=(64, 64), horizontal_flip=False, vertical_flip=False, brightness=0.0,
            rotation=0.0, zoom=0.0):
    """the reference's draws for n images, written out call by call (utils.py:319-350, :411-423)"""
    r = random.Random(seed)
    out = []
    for _ in range(n):
        b = bool(blur and r.randint(0, 1))
        cx = cy = 0
        if crop:
            cx = r.randrange(src[1] - crop[0])
            cy = r.randrange(src[0] - crop[1])
        hf = bool(horizontal_flip and r.randint(0, 1))
        vf = bool(vertical_flip and r.randint(0, 1))
        g = None
        if brightness:
            g = 1.0 + r.gauss(mu=0.0, sigma=brightness)
            if r.randint(0, 1):
                g = 1.0 / g
        angle = r.gauss(mu=0.0, sigma=rotation) if rotation else 0.0
        scale = r.gauss(mu=1.0, sigma=zoom) if zoom else 1.0
        out.append(A.ImageParams(b, cx, cy, hf, vf, g, angle, scale))
    return out


def _data(n=6, hw=(64, 64), seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n,) + hw + (3,), dtype=np.uint8),
            rng.integers(0, 4, (n,) + hw, dtype=np.uint8))


@pytest.mark.parametrize("opts", [NOTEBOOK_TRAIN, NOTEBOOK_VALID, dict(blur=5), dict(horizontal_flip=True),
                                  dict(vertical_flip=True), dict(brightness=0.2), dict(rotation=5.0), dict(zoom=0.1),
                                  dict(crop=(48, 40)),
                                  dict(blur=5, crop=(48, 40), horizontal_flip=True, vertical_flip=True, brightness=0.1,
                                       rotation=5.0, zoom=0.1)])
def test_parameter_stream_replays_the_reference_call_order(opts):
    imgs, labs = _data()
    kw = dict(opts)
    crop = kw.pop("crop", None)
    g = SegmentationGenerator(imgs, labs, n_classes=4, batch_size=2, seed=11, crop_shape=crop, **kw)
    got = []
    for i in range(len(g)):
        got += g.raw_batch(i)[2]
    assert got == _replay(11, 6, crop=crop, **kw)


def test_all_flags_off_draws_nothing():
    imgs, labs = _data()
    g = SegmentationGenerator(imgs, labs, n_classes=4, batch_size=2)
    assert not g.plan.active and g.raw_batch(0)[2] is None
    assert g.random.random() == random.Random(7).random()


@pytest.mark.parametrize("mode", ["train", "validation"])
def test_create_generators_split_and_defaults(mode):
    imgs, labs = _data(n=11)
    sm = SegModel(image_size=(64, 64))
    g = sm.create_generators(mode=mode, images=imgs, labels=labs, n_classes=4, seed=3, validation_split=.2)
    np.random.seed(3)
    x = np.random.permutation(11)[:round(11 * .2)]
    if mode == "train":
        x = np.setxor1d(x, np.arange(11))
    np.testing.assert_array_equal(g.images, imgs[x])
    np.testing.assert_array_equal(g.labels, labs[x])
    p = g.plan
    assert (p.hflip, p.vflip, p.blur, p.brightness, p.rotation, p.zoom, p.histeq) == (True, False, 0, 0.1, 5.0, 0.1, True)
    assert (p.H, p.W) == (64, 64)


def test_create_generators_rejects_what_it_cannot_do():
    sm = SegModel(image_size=(64, 64))
    imgs, labs = _data()
    with pytest.raises(ValueError, match="test"):
        sm.create_generators(mode="test", images=imgs, labels=labs)
    with pytest.raises(ValueError, match="out of scope"):
        sm.create_generators()
    with pytest.raises(ValueError, match="resize"):
        SegModel(image_size=(32, 32)).create_generators(images=imgs, labels=labs)
    with pytest.raises(ValueError, match="blur"):
        SegmentationGenerator(imgs, labs, blur=3)
    with pytest.raises(ValueError, match="int32"):
        SegmentationGenerator(imgs, labs.astype(np.int32), zoom=0.1)


def test_epoch_shuffle_uses_the_parameter_stream():
    imgs, labs = _data()
    g = SegmentationGenerator(imgs, labs, n_classes=4, batch_size=2, horizontal_flip=True, seed=5)
    draws = [g.raw_batch(i)[2] for i in range(len(g))]
    g.on_epoch_end()
    r = random.Random(5)
    for _ in range(6):
        r.randint(0, 1)
    order = list(range(6))
    r.shuffle(order)
    assert list(g.order) == order and len(draws) == 3


# ---------------------------------------------------------------- oracle known answers
def test_identity_warp_is_exact():
    img, lab = _data(1, (37, 50))
    np.testing.assert_array_equal(O.warp_affine(img[0], 0.0, 1.0), img[0])
    np.testing.assert_array_equal(O.warp_affine(lab[0], 0.0, 1.0), lab[0])


def test_blur_of_a_delta_and_of_a_constant():
    img = np.zeros((11, 11, 3), np.uint8)
    img[5, 5] = 255
    k = np.array([1, 4, 6, 4, 1], np.int64)
    want = np.zeros((11, 11), np.int64)
    want[3:8, 3:8] = (np.outer(k, k) * 255 + 128) >> 8
    got = O.gaussian_blur5(img)
    for c in range(3):
        np.testing.assert_array_equal(got[..., c], want)
    const = np.full((9, 13, 3), 77, np.uint8)
    np.testing.assert_array_equal(O.gaussian_blur5(const), const)


def test_gamma_lut_is_the_reference_expression():
    """the vectorised LUT of augment.py against the reference's per-element expression (utils.py:339-340), over the
    factors the notebook's brightness=0.3 stream draws and a few fixed ones"""
    r = random.Random(0)
    plan = A.Plan((8, 8), brightness=0.3)
    factors = [0.7, 1.0, 1.3, 1 / 1.3, 2.5, 0.2] + [plan.draw(r).gamma for _ in range(3000)]
    for f in factors:
        want = np.array([((i / 255.0) ** f) * 255 for i in np.arange(0, 256)]).astype(np.uint8)
        np.testing.assert_array_equal(A.gamma_lut(f), want, err_msg="factor %r" % f)
        np.testing.assert_array_equal(O.gamma_lut(f), want)


def test_clahe_of_a_constant_and_of_a_ramp():
    # constant 100 on 64x64: tiles of 8x8 = 64 px, clip = max(int(2*64/256), 1) = 1; bin 100 keeps 1, excess 63 <
    # 256 -> no batch, residual 63, step = 256 // 63 = 4: bins 0, 4, ..., 248 get +1 (63 bins), bin 100 = 1 + 1
    # cumsum at 100: bins 0..100 step 4 -> 26 redistributed (0..100) + own 1 = 27 ; lut = rint(27 * 255/64)
    plane = np.full((64, 64), 100, np.uint8)
    luts, (th, tw) = O.clahe_luts(plane)
    assert (th, tw) == (8, 8)
    want = np.float32(27) * (np.float32(255.0) / np.float32(64))
    assert luts[0, 0, 100] == int(np.rint(want))
    out = O.clahe(plane)
    assert (out == int(np.rint(want))).all()
    # horizontal ramp 0..255 over 256 columns, 8 rows: tiles 1x32 px, every value once -> no clipping (clip = 1)
    ramp = np.tile(np.arange(256, dtype=np.uint8), (8, 1))
    luts, (th, tw) = O.clahe_luts(ramp)
    assert (th, tw) == (1, 32)
    t = 3
    cs = np.cumsum(np.bincount(np.arange(32 * t, 32 * t + 32), minlength=256)).astype(np.float32)
    np.testing.assert_array_equal(luts[0, t], np.rint(cs * (np.float32(255.0) / np.float32(32))).astype(np.uint8))


def test_zoomed_label_map_voids_interpolated_values():
    lab = np.zeros((32, 32), np.uint8)
    lab[:, 16:] = 15
    p = A.ImageParams(False, 0, 0, False, False, None, 0.0, 1.3)
    img = np.zeros((32, 32, 3), np.uint8)
    _, out = O.augment_image(img, lab, p, (32, 32), True, False, 21)
    warped = O.warp_affine(lab, 0.0, 1.3)
    inter = (warped != 0) & (warped != 15)
    assert inter.any()
    assert (out[inter] == 21).all() and (out[~inter] == warped[~inter]).all()
    # a value created by the interpolation that WAS present in the source stays
    lab2 = lab.copy()
    lab2[0, 0] = warped[inter][0]
    _, out2 = O.augment_image(img, lab2, p, (32, 32), True, False, 21)
    v = warped[inter][0]
    assert (out2[O.warp_affine(lab2, 0.0, 1.3) == v] == v).all()


def test_host_tables_agree_with_the_oracle():
    for H, W, a, s in ((64, 64, 3.7, 1.08), (40, 57, -8.2, 0.93)):
        ad, bd, X0, Y0 = A.warp_tables(H, W, a, s)
        X, Y = O.warp_coords(H, W, a, s)
        np.testing.assert_array_equal((X0[:, None] + ad[None, :]) >> 5, X)
        np.testing.assert_array_equal((Y0[:, None] + bd[None, :]) >> 5, Y)


# ---------------------------------------------------------------- oracle vs scipy
def test_warp_matches_scipy_map_coordinates():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (45, 61), dtype=np.uint8)
    for angle, scale in ((7.5, 1.1), (-12.0, 0.9)):
        X, Y = O.warp_coords(45, 61, angle, scale)
        got = O.warp_affine(img, angle, scale).astype(np.int64)
        want = nd.map_coordinates(img.astype(np.float64), [Y / 32.0, X / 32.0], order=1, mode="grid-constant", cval=0)
        assert np.abs(got - np.rint(want)).max() <= 1


def test_blur_matches_scipy_convolve():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    got = O.gaussian_blur5(img)
    for c in range(3):
        s = nd.convolve(img[..., c].astype(np.int64), np.outer(k, k), mode="mirror")
        np.testing.assert_array_equal(got[..., c], ((s + 128) >> 8).astype(np.uint8))
