"""-m gpu: multi-scale / flip inference (csrc/tta.hip, tta.py, Model.predict_multiscale).

No tolerance anywhere in this file.  dl3_tta_resize_image and dl3_tta_accumulate evaluate the IEEE fp32 operations of
tests/tta_oracle.py's float32 run in the same order, so they must equal it BIT FOR BIT; and Model.predict_multiscale must
equal, bit for bit, the composition built here from independently constructed models: per pass the image resized by
dl3_tta_resize_image, an ordinary Deeplabv3 / SegModel of that input size carrying the model's weights run through its
ordinary predict(), and the float32 oracle's accumulate."""
import numpy as np
import pytest

from tests import tta_oracle as TO

pytestmark = pytest.mark.gpu

GUARD = 8            # floats in front of and behind every output
SENTINEL = -12345.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _guarded(n, offset, fill):
    """a device buffer of GUARD + offset sentinels, n floats of `fill` (an array or a scalar), GUARD sentinels; torch
    allocations are 256-byte aligned and GUARD is a multiple of 4, so `offset` is the output's distance from 16-byte
    alignment in floats"""
    import torch
    from tests import gpu_util as GU
    host = np.full(GUARD + offset + n + GUARD, SENTINEL, np.float32)
    host[GUARD + offset:GUARD + offset + n] = np.asarray(fill, np.float32).reshape(-1) if np.ndim(fill) else fill
    t = torch.from_numpy(host).cuda()
    GU._KEEP.append(t)
    assert t.data_ptr() % 16 == 0
    return t


def _check_guards(t, n, offset):
    h = t.cpu().numpy()
    assert np.all(h[:GUARD + offset] == SENTINEL) and np.all(h[GUARD + offset + n:] == SENTINEL), "guard words written"
    return h[GUARD + offset:GUARD + offset + n]


# ---------------------------------------------------------------------------------------------------------- operators
def _device_resize_image(src, Ho, Wo, flip, offset=0):
    import torch
    from tests import gpu_util as GU
    B, Hi, Wi, _ = src.shape
    d = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    GU._KEEP.append(d)
    n = B * Ho * Wo * 3
    out = _guarded(n, offset, np.nan)
    GU.call("dl3_tta_resize_image", d.data_ptr(), 1 if src.dtype == np.uint8 else 0, GU.ptr(out, GUARD + offset), B, Hi, Wi,
            Ho, Wo, int(flip))
    return _check_guards(out, n, offset).reshape(B, Ho, Wo, 3)


IMAGE_CASES = [((8, 8), (16, 16)), ((3, 5), (17, 33)), ((9, 9), (4, 4)), ((7, 11), (7, 11)), ((1, 1), (4, 4)), ((5, 6), (1, 1))]


@pytest.mark.parametrize("si,so", IMAGE_CASES)
def test_resize_image_equals_the_float32_oracle_bit_for_bit(si, so):
    rng = np.random.default_rng(hash((si, so)) % 2 ** 31)
    for B in (1, 3):
        u8 = rng.integers(0, 256, (B,) + si + (3,)).astype(np.uint8)
        f32 = (rng.random((B,) + si + (3,)) * 255.0).astype(np.float32)
        for src in (u8, f32):
            for flip in (0, 1):
                got = _device_resize_image(src, so[0], so[1], flip, offset=flip)
                want = TO.resize_image(src, so[0], so[1], bool(flip), np.float32)
                assert _same_bits(got, want), (si, so, B, src.dtype, flip)
                if si == so:   # the identity case is a bit copy
                    ident = src.astype(np.float32)
                    assert _same_bits(got, ident[:, :, ::-1] if flip else ident)


ACC_CASES = [((4, 4), (8, 8)), ((12, 12), (8, 8)), ((8, 8), (8, 8)), ((3, 5), (7, 9)), ((1, 1), (4, 4)), ((6, 5), (1, 1))]


@pytest.mark.parametrize("si,so", ACC_CASES)
def test_accumulate_equals_the_float32_oracle_bit_for_bit(si, so):
    from tests import gpu_util as GU
    rng = np.random.default_rng(hash((si, so, 1)) % 2 ** 31)
    Ho, Wo = so
    seen_ragged = False
    for C in (1, 2, 5, 21, 32):
        for B in (1, 3):
            p = rng.random((B,) + si + (C,)).astype(np.float32)
            p /= p.sum(-1, keepdims=True)
            dp = GU.dev(p)
            n = B * Ho * Wo * C
            seen_ragged |= (Ho * Wo * C) % 4 != 0
            old = rng.random((B, Ho, Wo, C)).astype(np.float32)
            for offset in (0, 1):     # 16-byte aligned, and one float past alignment
                for flip in (0, 1):
                    for first in (0, 1):
                        for n_last in (0, 3):
                            # first: NaN everywhere — a finite result proves the accumulator is not read
                            acc = _guarded(n, offset, np.nan if first else old)
                            GU.call("dl3_tta_accumulate", GU.ptr(dp), GU.ptr(acc, GUARD + offset), B, si[0], si[1], Ho, Wo, C,
                                    flip, first, n_last)
                            got = _check_guards(acc, n, offset).reshape(B, Ho, Wo, C)
                            want = TO.accumulate(p, old, Ho, Wo, bool(flip), bool(first), n_last, np.float32)
                            what = (si, so, C, B, offset, flip, first, n_last)
                            assert np.isfinite(got).all(), what
                            assert _same_bits(got, want), what
    if (si, so) in (((3, 5), (7, 9)), ((6, 5), (1, 1))):
        assert seen_ragged    # H * W * C is no multiple of 4 here: the scalar tail runs


def test_accumulate_spans_several_workgroups_and_both_alignments():
    """more than one workgroup (256 pixels each) with rows that straddle the workgroup cut: 40 x 40 x 21 from 24 x 56"""
    from tests import gpu_util as GU
    rng = np.random.default_rng(5)
    B, si, so, C = 2, (24, 56), (40, 40), 21
    p = rng.random((B,) + si + (C,)).astype(np.float32)
    old = rng.random((B,) + so + (C,)).astype(np.float32)
    dp = GU.dev(p)
    n = B * so[0] * so[1] * C
    for offset in (0, 1, 2, 3):
        acc = _guarded(n, offset, old)
        GU.call("dl3_tta_accumulate", GU.ptr(dp), GU.ptr(acc, GUARD + offset), B, si[0], si[1], so[0], so[1], C, 1, 0, 12)
        got = _check_guards(acc, n, offset).reshape(old.shape)
        assert _same_bits(got, TO.accumulate(p, old, so[0], so[1], True, False, 12, np.float32)), offset


def test_bad_arguments_are_refused(lib):
    from tests import gpu_util as GU
    from dl3_amd.capi import DL3Error
    a = GU.empty(64)
    with pytest.raises(DL3Error):
        GU.call("dl3_tta_accumulate", GU.ptr(a), GU.ptr(a), 1, 0, 4, 4, 4, 1, 0, 1, 0)
    with pytest.raises(DL3Error):
        GU.call("dl3_tta_accumulate", GU.ptr(a), GU.ptr(a), 1, 2, 2, 2, 2, 1, 2, 1, 0)
    with pytest.raises(DL3Error):
        GU.call("dl3_tta_resize_image", GU.ptr(a), 2, GU.ptr(a), 1, 2, 2, 2, 2, 0)


# ---------------------------------------------------------------------------------------------------------- models
B = 2
SHAPE = (64, 64, 3)
CLASSES = 5
SCALES = (0.5, 1.0, 1.5)


def _deeplab(shape, classes=CLASSES):
    from dl3_amd.deeplabv3p import Deeplabv3
    return Deeplabv3(weights=None, input_shape=tuple(shape), classes=classes, backbone="mobilenetv2")


def _images(seed=0, shape=SHAPE):
    return np.random.default_rng(seed).integers(0, 256, (B,) + tuple(shape)).astype(np.float32)


def _calibrate(m, shape, classes, head="deeplab"):
    """moving statistics of the BatchNorm layers <- the batch statistics of one training-mode pass of the CPU oracle over
    the model's own seeded weights on the images the tests use, _images() (the recipe of smoke()).  As constructed (mean 0, variance 1) the signal dies out
    through the 50 layers: the logits of this model are ~3e-11, EVERY probability is exactly 0.2, and bit-for-bit
    comparisons of such outputs would hold for any resize and any weights."""
    from oracle import dl3_oracle as O
    params = {n: w for l in m.layers for n, w in l.weights.items()}
    params = O.calibrate_bn(params, _images(0, shape), backbone="mobilenetv2", input_shape=tuple(shape), classes=classes,
                            head=head)
    for l in m.layers:
        if l.weights:
            l.set_weights([params[n] for n in l.weights])
    return m


def _spread(p):
    """the probabilities are not the uniform row: a comparison of them says something"""
    return float(np.asarray(p).std()) > 0.05


def _compose(weights, build, x, scales, flip):
    """the composition rule: per pass dl3_tta_resize_image, an independently built model of that size with `weights`
    through its ordinary predict(), the float32 oracle's accumulate.  -> probabilities [B,H,W,C] float32"""
    H, W = x.shape[1:3]
    passes = TO.pass_list((H, W), scales, flip)
    models, acc = {}, None
    for i, (_, hs, ws, flipped) in enumerate(passes):
        if (hs, ws) not in models:
            m = build((hs, ws, 3))
            m.set_weights(weights)
            models[(hs, ws)] = m
        xi = _device_resize_image(x, hs, ws, int(flipped))
        p = models[(hs, ws)].predict(xi, batch_size=B)
        p = p.reshape(B, hs, ws, -1)
        acc = TO.accumulate(p, acc, H, W, flipped, i == 0, len(passes) if i == len(passes) - 1 else 0, np.float32)
    return acc


@pytest.fixture(scope="module")
def model():
    from dl3_amd import graph as G
    G.clear_session(seed=21)
    return _calibrate(_deeplab(SHAPE), SHAPE, CLASSES)


def test_single_plain_pass_is_predict(model):
    x = _images()
    want = model.predict(x, batch_size=B)
    got = model.predict_multiscale(x, scales=(1.0,), flip=False, batch_size=B)
    assert got.dtype == np.float32 and np.isfinite(got).all() and _spread(want)
    assert _same_bits(got, want)
    mask = model.predict_multiscale(x, scales=(1.0,), flip=False, batch_size=B, output="mask")
    assert mask.dtype == np.int32 and mask.shape == (B, 64, 64)
    assert np.array_equal(mask, model.predict_mask(x, batch_size=B))
    # uint8 pixels and a device tensor are the same images
    import torch
    assert _same_bits(model.predict_multiscale(x.astype(np.uint8), scales=(1.0,), flip=False, batch_size=B), want)
    assert _same_bits(model.predict_multiscale(torch.from_numpy(x).cuda(), scales=(1.0,), flip=False, batch_size=B), want)


def test_three_scales_and_flip_equal_the_composition(model):
    x = _images()
    got = model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B)
    assert sorted(model._tta_siblings) == [(32, 32), (96, 96)]
    want = _compose(model.get_weights(), _deeplab, x, SCALES, True)
    assert got.shape == (B, 64 * 64, CLASSES) and np.isfinite(got).all() and _spread(got)
    assert _same_bits(got.reshape(want.shape), want)
    assert np.abs(got.sum(-1) - 1).max() < 1e-5
    mask = model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B, output="mask")
    assert np.array_equal(mask, TO.first_argmax(want))
    assert _same_bits(model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B), got)   # two calls
    # the averaging does something: it is not the single-scale prediction
    assert not _same_bits(got, model.predict(x, batch_size=B))


def test_current_weights_on_every_call():
    from dl3_amd import graph as G
    G.clear_session(seed=23)
    model = _calibrate(_deeplab(SHAPE), SHAPE, CLASSES)   # a model of its own: the test changes its weights
    x = _images()
    stale = model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B)   # siblings exist, with the old weights
    rng = np.random.default_rng(3)
    # 5 % of every value, relative: the moving variances stay positive
    ws = [w * (1 + 0.05 * rng.standard_normal(w.shape)).astype(np.float32) for w in model.get_weights()]
    model.set_weights(ws)
    try:
        def fresh_result():
            fresh = _deeplab(SHAPE)
            fresh.set_weights(model.get_weights())
            return fresh.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B)

        before = model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B)
        assert _spread(before) and not _same_bits(before, stale)
        assert _same_bits(before, fresh_result())
        y = np.random.default_rng(4).integers(0, CLASSES, (B, 64 * 64, 1)).astype(np.float32)
        model.compile(optimizer=dict(lr=7e-4))
        model.train_on_batch(x, y)
        after = model.predict_multiscale(x, scales=SCALES, flip=True, batch_size=B)
        assert np.isfinite(after).all() and not _same_bits(after, before)
        assert _same_bits(after, fresh_result())
    finally:
        model.clear_multiscale()
    assert not getattr(model, "_tta_siblings", None)


@pytest.mark.parametrize("net", ["subpixel", "original"])
def test_segmodel_heads_equal_the_composition(net):
    from dl3_amd import graph as G
    from dl3_amd.utils import SegModel
    G.clear_session(seed=5)
    n = 4

    def build(shape):
        return SegModel(image_size=tuple(shape[:2])).create_seg_model(net, n=n)

    m = build(SHAPE)
    if net == "subpixel":
        # the ICNR initialisation hands every class the same kernel: identical logits, every probability exactly 1 / n
        lyr = [l for l in m.layers if l.kind == "Subpixel"][0]
        k, b = lyr.get_weights()
        lyr.set_weights([np.random.default_rng(13).normal(0, 0.05, k.shape).astype(np.float32), b])
    m = _calibrate(m, SHAPE, n, head=net)
    x = _images()
    got = m.predict_multiscale(x, scales=(1.0, 1.5), flip=True, batch_size=B)
    want = _compose(m.get_weights(), build, x, (1.0, 1.5), True)
    assert got.shape == (B, 64 * 64, n) and np.isfinite(got).all() and _spread(got)
    assert _same_bits(got.reshape(want.shape), want)


def test_crf_on_the_averaged_probabilities():
    from dl3_amd import crf, graph as G
    G.clear_session(seed=7)
    m = _calibrate(_deeplab((32, 32, 3), classes=3), (32, 32, 3), 3)
    x = _images(0, (32, 32, 3))
    kw = dict(scales=(1.0, 1.5), flip=True, batch_size=B)
    probs = m.predict_multiscale(x, **kw)
    mask = m.predict_multiscale(x, output="mask", crf=True, **kw)
    assert mask.dtype == np.int32 and mask.shape == (B, 32, 32) and _spread(probs)
    assert np.array_equal(mask, crf.dense_crf_softmax(x, probs=probs))


def test_factory_builds_the_siblings_of_a_rewired_model():
    """a Model re-wired by hand has no rebuild closure: factory= supplies one"""
    from dl3_amd import graph as G
    G.clear_session(seed=9)
    d = _calibrate(_deeplab(SHAPE), SHAPE, CLASSES)
    m = G.Model(d.input, d.output)
    assert m._tta_rebuild is None
    x = _images()
    got = m.predict_multiscale(x, scales=(0.5, 1.0), flip=False, batch_size=B, factory=_deeplab)
    assert _same_bits(got.reshape(B, 64, 64, CLASSES), _compose(m.get_weights(), _deeplab, x, (0.5, 1.0), False))


def test_calculate_iou_multiscale_single_pass_is_calculate_iou(model):
    from dl3_amd import utils as U
    x = _images()
    label = np.random.default_rng(12).integers(0, CLASSES + 1, (B, 64, 64))
    label[label == CLASSES] = 255
    want = U.calculate_iou(model, x, label, nb_classes=CLASSES)
    got = U.calculate_iou_multiscale(model, x, label, nb_classes=CLASSES, scales=(1.0,), flip=False, batch_size=B)
    assert got.shape == want.shape == (CLASSES, CLASSES) and got.dtype == want.dtype
    assert np.array_equal(got, want) and got.sum() == (label < CLASSES).sum()
