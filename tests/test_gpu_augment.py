"""-m gpu: the augmentation kernels (dl3_augment, csrc/augment.hip) against the numpy oracle (tests/aug_oracle.py) bit
for bit — float32 image and label map, then dl3_prepare_targets on the device labels against the oracle's
prepare_targets —, the generator with every flag off against today's contract, and the device feed of an augmenting
generator against its own host-array batches (same losses, bit for bit)."""
import random

import numpy as np
import pytest
import torch

import dl3_amd  # noqa: F401
from dl3_amd import augment as A
from dl3_amd import capi
from dl3_amd import utils as U
from oracle import dl3_oracle as DO
from tests import aug_oracle as O

pytestmark = pytest.mark.gpu

C = 21
ALL = dict(blur=5, horizontal_flip=True, vertical_flip=True, brightness=0.3, rotation=10.0, zoom=0.15, do_ahisteq=True)
# the notebook's create_generators calls (cells 4 / 10) on top of create_generators' defaults (utils.py:216-218)
NB_TRAIN = dict(blur=5, horizontal_flip=True, brightness=0.3, zoom=0.1, rotation=5.0, do_ahisteq=True)
NB_VALID = dict(horizontal_flip=True, brightness=.1, zoom=.05, rotation=5.0, do_ahisteq=True)


def _data(B, hw, seed, ldtype=np.uint8):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)
    # smooth-ish images so that CLAHE / blur see structure; label maps with a few regions and void
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    imgs[..., 0] = (imgs[..., 0] // 4 + (xx * 3 + yy) % 192).astype(np.uint8)
    labs = np.zeros((B,) + hw, ldtype)
    for b in range(B):
        labs[b][(xx + b * 7) % 40 < 20] = 3 + b
        labs[b][(yy + xx) % 53 < 9] = 255
        labs[b][yy > hw[0] * 2 // 3] = 7
    return imgs, labs


def _params(plan, B, seed):
    """drawn from the seeded stream, then forced so that every image-level switch is exercised both ways"""
    r = random.Random(seed)
    ps = [plan.draw(r) for _ in range(B)]
    out = []
    for n, p in enumerate(ps):
        p = p._replace(blur=bool(plan.blur) and n != 1, hflip=plan.hflip and n != 2, vflip=plan.vflip and n != 0)
        out.append(p)
    return out


def _run(plan, params, imgs, labs):
    B = len(params)
    tab, offs = A.tables(plan, params)
    tab = torch.from_numpy(tab).cuda()
    di, dl = torch.from_numpy(imgs).cuda(), torch.from_numpy(labs).cuda()
    X = torch.full((B, plan.H, plan.W, 3), float("nan"), device="cuda")
    L = torch.full((B, plan.H * plan.W), 99, dtype=dl.dtype, device="cuda")
    ws = torch.full((A.workspace_bytes(plan, B),), 0xA5, dtype=torch.uint8, device="cuda")
    A.launch(plan, tab, offs, di, dl, C, X, L, ws)
    torch.cuda.synchronize()
    return X, L


CASES = []
for hw in ((100, 76), (96, 60)):
    for k in ("blur", "horizontal_flip", "vertical_flip", "brightness", "rotation", "zoom", "do_ahisteq"):
        CASES.append((hw, None, {k: ALL[k]}, np.uint8))
for hw in ((512, 512), (320, 320), (100, 76), (96, 60)):
    CASES.append((hw, None, ALL, np.uint8))
for hw in ((512, 512), (320, 320)):
    CASES.append((hw, None, NB_TRAIN, np.uint8))
    CASES.append((hw, None, NB_VALID, np.uint8))
CASES.append(((90, 120), (96, 64), ALL, np.uint8))                   # crop (w, h) from a larger source
CASES.append(((90, 120), (96, 64), dict(horizontal_flip=True), np.uint8))
CASES.append(((100, 76), None, dict(blur=5, horizontal_flip=True, vertical_flip=True, brightness=0.3, do_ahisteq=True),
              np.int32))                                             # int32 labels: everything but the warp
CASES.append(((90, 120), (96, 64), dict(blur=5, brightness=0.2), np.int32))
# H*W odd (99*77): the scalar tail stores of the warp and CLAHE kernels and the byte path of the label-set pass
CASES.append(((99, 77), None, ALL, np.uint8))
CASES.append(((99, 77), None, dict(rotation=10.0, zoom=0.15, horizontal_flip=True), np.uint8))
CASES.append(((99, 77), None, dict(do_ahisteq=True, blur=5), np.uint8))


@pytest.mark.parametrize("hw,crop,opts,ldtype", CASES,
                         ids=["%dx%d-%s-%s-%s" % (c[0] + (c[1] and "crop" or "full", "+".join(sorted(c[2])),
                                                          np.dtype(c[3]).name)) for c in CASES])
def test_kernels_match_the_oracle_bit_exactly(hw, crop, opts, ldtype):
    B = 3
    plan = A.Plan(hw, crop_shape=crop, **opts)
    imgs, labs = _data(B, hw, seed=hw[0] + len(opts), ldtype=ldtype)
    params = _params(plan, B, seed=17 + hw[1])
    X, L = _run(plan, params, imgs, labs)
    Xo, Lo = O.augment_batch(imgs, labs, params, (plan.H, plan.W), plan.warp, plan.histeq, C)
    Xg = X.cpu().numpy()
    Lg = L.cpu().numpy().reshape(Lo.shape)
    bad = np.argwhere(Xg != Xo)
    assert bad.size == 0, ("X differs at %d places, first %s: gpu %s oracle %s"
                           % (len(bad), bad[0], Xg[tuple(bad[0])], Xo[tuple(bad[0])]))
    np.testing.assert_array_equal(Lg, Lo)
    Y, SW = U.prepare_targets(L.reshape(B, plan.H, plan.W), C)
    Yo, SWo, _ = DO.prepare_targets(Lo.reshape(B, -1), C)
    np.testing.assert_array_equal(Y.cpu().numpy(), Yo)
    np.testing.assert_array_equal(SW.cpu().numpy(), SWo)


def test_int32_labels_cannot_be_warped():
    plan = A.Plan((32, 32), zoom=0.1)
    imgs, labs = _data(1, (32, 32), 0, np.int32)
    with pytest.raises(capi.DL3Error, match="rc=-4"):
        _run(plan, _params(plan, 1, 0), imgs, labs)


def test_all_flags_off_equals_todays_generator():
    from dl3_amd.utils import SegModel, SegmentationGenerator
    imgs, labs = _data(6, (64, 48), 3)
    g = SegmentationGenerator(imgs, labs, n_classes=C, batch_size=2, seed=4, resize_shape=(48, 64),
                              horizontal_flip=False, vertical_flip=False, blur=0, brightness=0, rotation=0, zoom=0,
                              do_ahisteq=False)
    sm = SegModel(image_size=(64, 48))
    sm.set_batch_size(2)
    gc = sm.create_generators(images=imgs, labels=labs, n_classes=C, validation_split=0.0, horizontal_flip=False,
                              brightness=0, rotation=0, zoom=0, do_ahisteq=False, seed=4)
    SegModel.set_batch_size(16)
    for gen in (g, gc):
        for ep in range(2):
            for i in range(len(gen)):
                X, Y, SW = gen[i]
                idx = gen.order[2 * i:2 * i + 2]
                np.testing.assert_array_equal(X, imgs[idx].astype(np.float32))
                Yo, SWo, _ = DO.prepare_targets(labs[idx].reshape(2, -1), C)
                np.testing.assert_array_equal(Y.cpu().numpy(), Yo)
                np.testing.assert_array_equal(SW["pred_mask"].cpu().numpy(), SWo)
            gen.on_epoch_end()
    rs = np.random.RandomState(4)
    order = np.arange(6)
    rs.shuffle(order)
    rs.shuffle(order)
    np.testing.assert_array_equal(g.order, order)


def test_augmenting_generator_batches_match_the_oracle():
    from dl3_amd.utils import SegmentationGenerator
    imgs, labs = _data(4, (72, 80), 9)
    g = SegmentationGenerator(imgs, labs, n_classes=C, batch_size=2, seed=12, crop_shape=(64, 64), **NB_TRAIN)
    twin = SegmentationGenerator(imgs, labs, n_classes=C, batch_size=2, seed=12, crop_shape=(64, 64), **NB_TRAIN)
    for i in range(2):
        X, Y, SW = g[i]
        im, lb, ps = twin.raw_batch(i)
        Xo, Lo = O.augment_batch(im, lb, ps, (64, 64), True, True, C)
        assert isinstance(X, np.ndarray) and X.dtype == np.float32
        np.testing.assert_array_equal(X, Xo)
        Yo, SWo, _ = DO.prepare_targets(Lo.reshape(2, -1), C)
        np.testing.assert_array_equal(Y.cpu().numpy(), Yo)
        np.testing.assert_array_equal(SW["pred_mask"].cpu().numpy(), SWo)


def test_device_feed_trains_exactly_like_the_host_batches():
    """fit_generator(device_feed=True) on an augmenting generator (crop from a larger source: the feeder's slots follow
    the source size) gives the losses fit_generator(device_feed=False) gets from the same seeded generator's host-array
    batches, bit for bit, over two epochs (the epoch-end shuffle draws from the same stream)"""
    from dl3_amd.utils import SegmentationGenerator
    from tests.test_gpu_model import _build, _load
    classes, shape = 5, (64, 64, 3)
    rng = np.random.default_rng(23)
    imgs = rng.integers(0, 256, (6, 80, 72, 3), dtype=np.uint8)
    labs = rng.integers(0, classes, (6, 80, 72), dtype=np.uint8)
    labs[:, :10] = 255

    def run(device_feed):
        model, params = _build("mobilenetv2", shape, classes, "deeplab")
        _load(model, params)
        model.compile(optimizer=dict(lr=1e-3))
        g = SegmentationGenerator(imgs, labs, n_classes=classes, batch_size=2, seed=31, crop_shape=(64, 64), **NB_TRAIN)
        return model.fit_generator(g, epochs=2, device_feed=device_feed, n_classes=classes)

    host = run(False)
    fed = run(True)
    assert len(host) == 6 and all(np.isfinite(host))
    assert fed == host, (fed, host)


@pytest.mark.parametrize("read_back", [24576, 262144])
def test_host_read_back_between_steps(read_back):
    """a pageable device-to-host read-back (here `.cpu()` of 96 KB / 1 MB, what the augmenting generator's X and any
    host-side metric do) between two train_on_batch calls after the hipGraph capture changes nothing: the losses equal
    those of the same steps without it (Engine.train_step drains the stream before it enqueues a step)"""
    from dl3_amd.utils import SegmentationGenerator
    from tests.test_gpu_model import _build, _load
    classes, shape = 5, (64, 64, 3)
    rng = np.random.default_rng(23)
    imgs = rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8)
    labs = rng.integers(0, classes, (8, 64, 64), dtype=np.uint8)

    def run(extra):
        model, params = _build("mobilenetv2", shape, classes, "deeplab")
        _load(model, params)
        model.compile(optimizer=dict(lr=1e-3))
        g = SegmentationGenerator(imgs, labs, n_classes=classes, batch_size=2, shuffle=False)
        out = []
        for i in range(len(g)):
            X, Y, SW = g[i]
            if extra:
                torch.zeros(read_back, device="cuda").cpu()
            out.append(model.train_on_batch(X, Y, SW["pred_mask"], lazy_loss=True))
        return [float(l) for l in out]

    plain = run(False)
    assert run(True) == plain, plain
