"""-m gpu: sliding-window inference (csrc/slide.hip, slide.py, Model.predict_sliding).

No tolerance on values anywhere in this file.  dl3_slide_gather is a crop; dl3_slide_accumulate and dl3_slide_finalize
evaluate the IEEE fp32 operations of tests/slide_oracle.py's float32 run in the same order, so they must equal it BIT FOR
BIT however the window sequence is cut into launches; and Model.predict_sliding must equal, bit for bit, the composition
built here: the oracle's gather, the model's ordinary predict() over the windows in the same batches, the float32
oracle's blend."""
import numpy as np
import pytest

from tests import slide_oracle as SO

pytestmark = pytest.mark.gpu

GUARD = 8            # floats in front of and behind every output
SENTINEL = -12345.5
UNIFORM, PYRAMID = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _guarded(n, offset, fill, dtype=np.float32):
    """a device buffer of GUARD + offset sentinels, n elements of `fill` (an array or a scalar), GUARD sentinels; torch
    allocations are 256-byte aligned and GUARD is a multiple of 4, so `offset` is the output's distance from 16-byte
    alignment in elements of 4 bytes"""
    import torch
    from tests import gpu_util as GU
    host = np.full(GUARD + offset + n + GUARD, SENTINEL, dtype)
    host[GUARD + offset:GUARD + offset + n] = np.asarray(fill, dtype).reshape(-1) if np.ndim(fill) else fill
    t = torch.from_numpy(host).cuda()
    GU._KEEP.append(t)
    assert t.data_ptr() % 16 == 0
    return t


def _check_guards(t, n, offset):
    h = t.cpu().numpy()
    s = h.dtype.type(SENTINEL)
    assert np.all(h[:GUARD + offset] == s) and np.all(h[GUARD + offset + n:] == s), "guard words written"
    return h[GUARD + offset:GUARD + offset + n]


def _pair(v):
    return (v, v) if np.ndim(v) == 0 else tuple(v)


def _cuts(n, cut):
    return [(k, min(cut, n - k)) for k in range(0, n, cut)]


# ---------------------------------------------------------------------------------------------------------- operators
def _device_gather(img, win, stride, k0, nw, pad, offset):
    import torch
    from tests import gpu_util as GU
    Hi, Wi = img.shape[:2]
    sh, sw = _pair(stride)
    d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    GU._KEEP.append(d)
    n = nw * win * win * 3
    out = _guarded(n, offset, np.nan)
    GU.call("dl3_slide_gather", d.data_ptr(), 1 if img.dtype == np.uint8 else 0, Hi, Wi, win, win, sh, sw, k0, nw, float(pad),
            GU.ptr(out, GUARD + offset))
    return _check_guards(out, n, offset).reshape(nw, win, win, 3)


def _device_accumulate(p, size, win, stride, blend, cut, offset, with_wsum=False):
    """the windows of p [n,win,win,C] folded into a zeroed, guarded canvas in launches of `cut` windows
    -> (canvas tensor, wsum tensor or None)"""
    from tests import gpu_util as GU
    Hi, Wi = size
    sh, sw = _pair(stride)
    n, _, _, C = p.shape
    dp = GU.dev(p)
    acc = _guarded(Hi * Wi * C, offset, 0.0)
    ws = _guarded(Hi * Wi, (offset + 1) % 4, 0.0) if with_wsum else None
    for k0, nw in _cuts(n, cut):
        GU.call("dl3_slide_accumulate", GU.ptr(dp, k0 * win * win * C), GU.ptr(acc, GUARD + offset),
                None if ws is None else GU.ptr(ws, GUARD + (offset + 1) % 4), Hi, Wi, win, win, C, sh, sw, k0, nw, blend)
    return acc, ws


def _device_finalize(canvas, ws, size, win, stride, C, blend, mode, offset):
    """canvas: host float32 [Hi*Wi*C]; mode "alias": probabilities in place, "separate": into a buffer of its own at
    another alignment, "mask": the mask alone -> (probs or None, mask)"""
    from tests import gpu_util as GU
    Hi, Wi = size
    sh, sw = _pair(stride)
    n = Hi * Wi * C
    acc = _guarded(n, offset, canvas)
    dws = None if ws is None else GU.dev(ws)
    mask = _guarded(Hi * Wi, 1, 0, np.int32)
    out, ooff = None, (offset + 2) % 4
    if mode == "alias":
        pout = GU.ptr(acc, GUARD + offset)
    elif mode == "separate":
        out = _guarded(n, ooff, np.nan)
        pout = GU.ptr(out, GUARD + ooff)
    else:
        pout = None
    GU.call("dl3_slide_finalize", GU.ptr(acc, GUARD + offset), GU.ptr(dws), pout, GU.ptr(mask, GUARD + 1), Hi, Wi, win, win, C,
            sh, sw, blend)
    m = _check_guards(mask, Hi * Wi, 1).reshape(Hi, Wi)
    a = _check_guards(acc, n, offset)
    if mode == "alias":
        return a.reshape(Hi, Wi, C), m
    assert np.array_equal(_bits(a), _bits(canvas)), "finalize wrote its input"
    if mode == "separate":
        return _check_guards(out, n, ooff).reshape(Hi, Wi, C), m
    return None, m


def _probabilities(rng, n, win, C):
    """positive random rows that sum to 1, with exact zeros among them"""
    p = rng.random((n, win, win, C)).astype(np.float32)
    if C > 1:
        p[rng.random(p.shape) < 0.1] = 0.0
        p[..., 0] += np.float32(1e-3)
        p /= p.sum(-1, keepdims=True)
    else:
        p[rng.random(p.shape) < 0.1] = 0.0
    return p


def _check_blend(size, win, stride, C, blend, rng, cuts=(None, 1, 3)):
    name = "pyramid" if blend == PYRAMID else "uniform"
    n = len(SO.grid(size, (win, win), stride)[2])
    p = _probabilities(rng, n, win, C)
    assert (p == 0).any() and p.min() >= 0
    want_acc, want_ws = SO.blend(p, size, (win, win), stride, name, np.float32, parts=True)
    want = SO.blend(p, size, (win, win), stride, name, np.float32)
    what = (size, win, stride, C, name)
    canvas = None
    for i, cut in enumerate(cuts):      # one launch, one window per launch, chunks of 3 (k0 > 0): the same bits
        offset = (i + C) % 4
        acc, ws = _device_accumulate(p, size, win, stride, blend, cut or n, offset, with_wsum=(i == 2))
        canvas = _check_guards(acc, want_acc.size, offset)
        assert _same_bits(canvas.reshape(want_acc.shape), want_acc), what + (cut,)
        if ws is not None:
            plane = _check_guards(ws, want_ws.size, (offset + 1) % 4)
            assert _same_bits(plane.reshape(want_ws.shape), want_ws), what + (cut, "wsum")
    for j, (mode, plane) in enumerate((("alias", None), ("separate", None), ("mask", None), ("separate", want_ws))):
        probs, mask = _device_finalize(canvas, plane, size, win, stride, C, blend, mode, (j + C) % 4)
        if probs is not None:
            assert _same_bits(probs, want), what + (mode, plane is not None)
        assert mask.dtype == np.int32 and np.array_equal(mask, SO.first_argmax(want)), what + (mode,)
    if n == 1 and blend == UNIFORM and tuple(size) == (win, win):
        assert _same_bits(want, p[0])        # a single uniform window is a bit copy


OP_CASES = [((16, 16), 8), ((23, 37), 11), ((9, 40), (5, 16)), ((5, 7), 3), ((33, 16), (1, 16)), ((40, 41), 10)]


@pytest.mark.parametrize("size,stride", OP_CASES)
def test_accumulate_and_finalize_equal_the_float32_oracle_bit_for_bit(size, stride):
    rng = np.random.default_rng(abs(hash((size, stride))) % 2 ** 31)
    for C in (1, 5, 21):
        for blend in (UNIFORM, PYRAMID):
            _check_blend(size, 16, stride, C, blend, rng)


def test_accumulate_spans_several_workgroups():
    """window 64 x 64, C = 21, image (100, 75), stride 42: four windows, one workgroup per canvas row — up to 100 of them in
    a launch — and rows of 1575 floats, so consecutive rows start at every distance from a 16-byte boundary"""
    rng = np.random.default_rng(7)
    for blend in (UNIFORM, PYRAMID):
        _check_blend((100, 75), 64, 42, 21, blend, rng)


def test_accumulate_rows_longer_than_a_workgroup():
    """a row span of 600 pixels: three workgroups per row, pixels that straddle their cuts (C = 5, 21)"""
    rng = np.random.default_rng(8)
    for C in (5, 21):
        _check_blend((17, 600), 16, (16, 13), C, PYRAMID, rng, cuts=(None, 7))


@pytest.mark.parametrize("size,stride", OP_CASES)
def test_gather_equals_the_crop_bit_for_bit(size, stride):
    rng = np.random.default_rng(abs(hash((size, stride, 1))) % 2 ** 31)
    n = len(SO.grid(size, (16, 16), stride)[2])
    u8 = rng.integers(0, 256, size + (3,)).astype(np.uint8)
    f32 = (rng.random(size + (3,)) * 255.0).astype(np.float32)
    for src in (u8, f32):
        for pad in (127.5, 0.0):
            want = SO.gather(src, (16, 16), stride, pad)
            for i, cut in enumerate((n, 3)):
                got = np.concatenate([_device_gather(src, 16, stride, k0, nw, pad, (i + k0) % 4) for k0, nw in _cuts(n, cut)])
                assert _same_bits(got, want), (size, stride, src.dtype, pad, cut)
    if size == (5, 7):
        assert np.all(want[0, 5:] == 0.0) and np.all(want[0, :, 7:] == 0.0)


def test_gather_window_64():
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (100, 75, 3)).astype(np.uint8)
    got = _device_gather(src, 64, 42, 1, 3, 127.5, 1)
    assert _same_bits(got, SO.gather(src, (64, 64), 42)[1:4])


def test_bad_arguments_are_refused(lib):
    from tests import gpu_util as GU
    from dl3_amd.capi import DL3Error
    a = GU.empty(16 * 16 * 3 * 4)
    m = GU.empty(64)
    pa = GU.ptr(a)

    # (23, 37) under 16 x 16 at stride 11 has 6 windows
    bad_gather = [
        (pa, 0, 23, 37, 16, 16, 0, 11, 0, 1, 127.5, pa),      # stride 0
        (pa, 0, 23, 37, 16, 16, 11, 17, 0, 1, 127.5, pa),     # stride > window
        (pa, 0, 23, 37, 16, 16, 11, 11, 5, 2, 127.5, pa),     # k0 + nw beyond the grid
        (pa, 0, 23, 37, 16, 16, 11, 11, -1, 1, 127.5, pa),
        (pa, 0, 23, 37, 16, 16, 11, 11, 0, 0, 127.5, pa),     # nw < 1
        (pa, 2, 23, 37, 16, 16, 11, 11, 0, 1, 127.5, pa),     # unknown dtype
        (pa, 0, 0, 37, 16, 16, 11, 11, 0, 1, 127.5, pa),      # empty image
        (pa, 0, 65536, 65536, 16, 16, 11, 11, 0, 1, 127.5, pa),   # 2^32 pixels
        (None, 0, 23, 37, 16, 16, 11, 11, 0, 1, 127.5, pa),
    ]
    for args in bad_gather:
        with pytest.raises(DL3Error, match="slide_gather"):
            GU.call("dl3_slide_gather", *args)
    bad_acc = [
        (pa, pa, None, 23, 37, 16, 16, 1, 0, 11, 0, 1, 0),
        (pa, pa, None, 23, 37, 16, 16, 1, 11, 17, 0, 1, 0),
        (pa, pa, None, 23, 37, 16, 16, 1, 11, 11, 4, 3, 0),
        (pa, pa, None, 23, 37, 16, 16, 1, 11, 11, 0, 0, 0),
        (pa, pa, None, 23, 37, 16, 16, 1, 11, 11, 0, 1, 2),       # unknown blend
        (pa, pa, None, 23, 37, 16, 16, 0, 11, 11, 0, 1, 0),       # C = 0
        (pa, pa, None, 65536, 65536, 16, 16, 1, 11, 11, 0, 1, 0),
        (pa, pa, None, 16, 40000, 16, 16, 65536, 11, 11, 0, 1, 0),   # a row of 2^31.3 floats
        (pa, None, None, 23, 37, 16, 16, 1, 11, 11, 0, 1, 0),
    ]
    for args in bad_acc:
        with pytest.raises(DL3Error, match="slide_accumulate"):
            GU.call("dl3_slide_accumulate", *args)
    pm = m.data_ptr()
    bad_fin = [
        (pa, None, None, None, 23, 37, 16, 16, 1, 11, 11, 0),     # both outputs NULL
        (pa, None, pa, pm, 23, 37, 16, 16, 1, 11, 0, 0),
        (pa, None, pa, pm, 23, 37, 16, 16, 1, 17, 11, 0),
        (pa, None, pa, pm, 23, 37, 16, 16, 1, 11, 11, 7),
        (pa, None, pa, pm, 23, 37, 16, 16, 0, 11, 11, 0),
        (pa, None, pa, pm, 65536, 65536, 16, 16, 1, 11, 11, 0),
        (None, None, pa, pm, 23, 37, 16, 16, 1, 11, 11, 0),
    ]
    for args in bad_fin:
        with pytest.raises(DL3Error, match="slide_finalize"):
            GU.call("dl3_slide_finalize", *args)
    assert np.isnan(GU.host(a)).all() and np.isnan(GU.host(m)).all()      # nothing was launched


# ---------------------------------------------------------------------------------------------------------- models
B = 2
SHAPE = (64, 64, 3)
WIN = (64, 64)
CLASSES = 5


def _deeplab(shape, classes=CLASSES):
    from dl3_amd.deeplabv3p import Deeplabv3
    return Deeplabv3(weights=None, input_shape=tuple(shape), classes=classes, backbone="mobilenetv2")


def _images(seed=0, shape=SHAPE, n=B):
    return np.random.default_rng(seed).integers(0, 256, (n,) + tuple(shape)).astype(np.float32)


def _calibrate(m, shape, classes, head="deeplab"):
    """moving statistics of the BatchNorm layers <- the batch statistics of one training-mode pass of the CPU oracle over
    the model's own seeded weights on _images() (the recipe of smoke()).  As constructed (mean 0, variance 1) the signal
    dies out through the 50 layers and EVERY probability is exactly 1 / classes: bit-for-bit comparisons of such outputs
    would hold for any blend and any weights."""
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


def _compose(model, images, stride, blend, batch_size, pad_value=127.5):
    """the composition rule: the oracle's gather over all images (image-major, then k), the model's ordinary predict()
    over that window list in the same batches, the float32 oracle's blend per image -> [probabilities [Hi,Wi,C], ...]"""
    windows = SO.gather(images, WIN, stride, pad_value)
    p = model.predict(windows, batch_size=batch_size).reshape(len(windows), WIN[0], WIN[1], -1)
    outs, k = [], 0
    for im in images:
        size = im.shape[:2]
        n = len(SO.grid(size, WIN, stride)[2])
        outs.append(SO.blend(p[k:k + n], size, WIN, stride, blend, np.float32))
        k += n
    assert k == len(windows)
    return outs, p


@pytest.fixture(scope="module")
def model():
    from dl3_amd import graph as G
    G.clear_session(seed=21)
    return _calibrate(_deeplab(SHAPE), SHAPE, CLASSES)


def test_model_size_images_are_predict(model):
    x = _images()
    want = model.predict(x, batch_size=B)
    got = model.predict_sliding(x, blend="uniform", batch_size=B, output="probs")
    assert got.dtype == np.float32 and got.shape == (B, 64, 64, CLASSES) and np.isfinite(got).all() and _spread(want)
    assert _same_bits(got, want.reshape(got.shape))
    mask = model.predict_sliding(x, blend="uniform", batch_size=B)
    assert mask.dtype == np.int32 and mask.shape == (B, 64, 64)
    assert np.array_equal(mask, model.predict_mask(x, batch_size=B))
    assert np.array_equal(mask, SO.first_argmax(got))


@pytest.mark.parametrize("blend", ["uniform", "pyramid"])
def test_larger_images_equal_the_composition(model, blend):
    """[3,100,75,3] at stride 42: 4 windows per image, 12 in all, in chunks of 5, 5, 2 that span the images"""
    x = np.random.default_rng(1).integers(0, 256, (3, 100, 75, 3)).astype(np.float32)
    got = model.predict_sliding(x, stride=42, blend=blend, batch_size=5, output="probs")
    want, p = _compose(model, list(x), 42, blend, 5)
    want = np.stack(want)
    assert got.shape == (3, 100, 75, CLASSES) and got.dtype == np.float32 and np.isfinite(got).all() and _spread(got)
    assert _same_bits(got, want)
    rows = np.abs(got.astype(np.float64).sum(-1) - 1).max()
    print("row sums within %.3e of 1" % rows)
    assert rows < 1e-5
    assert _same_bits(model.predict_sliding(x, stride=42, blend=blend, batch_size=5, output="probs"), got)   # two calls
    mask = model.predict_sliding(x, stride=42, blend=blend, batch_size=5)
    assert mask.shape == (3, 100, 75) and np.array_equal(mask, SO.first_argmax(want))
    # pixel (10, 20) of image 0 lies under windows 0 (x0 = 0) and 1 (x0 = 11) only: the blend is not window 0's value
    assert SO.coverage((100, 75), WIN, 42)[10, 20] == 2
    assert not np.array_equal(_bits(got[0, 10, 20]), _bits(p[0, 10, 20]))
    # ... while pixel (5, 5) lies under window 0 alone and is its value
    assert SO.coverage((100, 75), WIN, 42)[5, 5] == 1
    assert _same_bits(got[0, 5, 5], p[0, 5, 5])


def test_ragged_list_equals_the_composition(model):
    """sizes (100, 75), (64, 64), (40, 90): 4 + 1 + 2 windows in chunks of 5 and 2; the third image is padded below"""
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((100, 75), (64, 64), (40, 90))]
    for blend in ("uniform", "pyramid"):
        got = model.predict_sliding(images, stride=42, blend=blend, batch_size=5, output="probs")
        want, _ = _compose(model, images, 42, blend, 5)
        assert isinstance(got, list) and len(got) == 3
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and _spread(g) and _same_bits(g, w)
        masks = model.predict_sliding(images, stride=42, blend=blend, batch_size=5)
        for mk, w, im in zip(masks, want, images):
            assert mk.dtype == np.int32 and mk.shape == im.shape[:2] and np.array_equal(mk, SO.first_argmax(w))
    # another pad value reaches the network: the padded image changes, the others do not
    other = model.predict_sliding(images, stride=42, batch_size=5, output="probs", pad_value=0.0)
    want0, _ = _compose(model, images, 42, "uniform", 5, pad_value=0.0)
    assert all(_same_bits(g, w) for g, w in zip(other, want0))
    assert not _same_bits(other[2], got[2])


def test_uint8_float32_and_device_input_are_the_same_images(model):
    import torch
    x = np.random.default_rng(3).integers(0, 256, (2, 70, 64, 3)).astype(np.uint8)
    kw = dict(stride=(6, 64), blend="pyramid", batch_size=3, output="probs")
    want = model.predict_sliding(x, **kw)
    assert _spread(want)
    assert _same_bits(model.predict_sliding(x.astype(np.float32), **kw), want)
    assert _same_bits(model.predict_sliding(torch.from_numpy(x).cuda(), **kw), want)
    assert _same_bits(model.predict_sliding(torch.from_numpy(x.astype(np.float32)).cuda(), **kw), want)
    as_list = model.predict_sliding([torch.from_numpy(x[0]).cuda(), x[1].astype(np.float32)], **kw)
    assert _same_bits(np.stack(as_list), want)


@pytest.mark.parametrize("net", ["subpixel", "original"])
def test_segmodel_heads_equal_the_composition(net):
    from dl3_amd import graph as G
    from dl3_amd.utils import SegModel
    G.clear_session(seed=5)
    n = 4
    m = SegModel(image_size=SHAPE[:2]).create_seg_model(net, n=n)
    if net == "subpixel":
        # the ICNR initialisation hands every class the same kernel: identical logits, every probability exactly 1 / n
        lyr = [l for l in m.layers if l.kind == "Subpixel"][0]
        k, b = lyr.get_weights()
        lyr.set_weights([np.random.default_rng(13).normal(0, 0.05, k.shape).astype(np.float32), b])
    m = _calibrate(m, SHAPE, n, head=net)
    x = np.random.default_rng(4).integers(0, 256, (2, 80, 100, 3)).astype(np.uint8)
    got = m.predict_sliding(x, blend="pyramid", batch_size=3, output="probs")      # the default stride: 42
    want, _ = _compose(m, list(x), None, "pyramid", 3)
    assert got.shape == (2, 80, 100, n) and np.isfinite(got).all() and _spread(got)
    assert _same_bits(got, np.stack(want))


def test_current_weights_on_every_call():
    from dl3_amd import graph as G
    G.clear_session(seed=23)
    m = _calibrate(_deeplab(SHAPE), SHAPE, CLASSES)   # a model of its own: the test changes its weights
    x = np.random.default_rng(6).integers(0, 256, (1, 64, 100, 3)).astype(np.uint8)
    kw = dict(stride=36, blend="uniform", batch_size=2, output="probs")
    stale = m.predict_sliding(x, **kw)
    rng = np.random.default_rng(3)
    # 5 % of every value, relative: the moving variances stay positive
    m.set_weights([w * (1 + 0.05 * rng.standard_normal(w.shape)).astype(np.float32) for w in m.get_weights()])
    got = m.predict_sliding(x, **kw)
    assert _spread(got) and not _same_bits(got, stale)
    fresh = _deeplab(SHAPE)
    fresh.set_weights(m.get_weights())
    assert _same_bits(got, fresh.predict_sliding(x, **kw))
    want, _ = _compose(m, list(x), 36, "uniform", 2)
    assert _same_bits(got, np.stack(want))


def test_calculate_iou_sliding_on_model_size_images_is_calculate_iou(model):
    from dl3_amd import utils as U
    x = _images()
    label = np.random.default_rng(12).integers(0, CLASSES + 1, (B, 64, 64))
    label[label == CLASSES] = 255
    want = U.calculate_iou(model, x, label, nb_classes=CLASSES)
    got = U.calculate_iou_sliding(model, x, label, nb_classes=CLASSES, batch_size=B)
    assert got.shape == want.shape == (CLASSES, CLASSES) and got.dtype == want.dtype
    assert np.array_equal(got, want) and got.sum() == (label < CLASSES).sum()
    as_lists = U.calculate_iou_sliding(model, list(x), list(label), nb_classes=CLASSES, batch_size=B)
    assert np.array_equal(as_lists, want)
