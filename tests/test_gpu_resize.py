"""-m gpu: the cv2.resize front end (dl3_cv_resize, csrc/cvresize.hip) against the numpy oracle (tests/resize_oracle.py)
bit for bit over one ragged batch — up, down, 1- and 2-pixel sources, an equal-size image, a crop, blur on for some, uint8
and int32 label maps, images that start off every alignment in the pools —, the label sets of the source maps, the error
codes, the stand-alone cv_resize, the generator over images of different sizes against the oracles of the whole chain, and
the device feed of such a generator against its twin's host batches (same losses, bit for bit)."""
import numpy as np
import pytest
import torch

import dl3_amd  # noqa: F401
from dl3_amd import augment as A
from dl3_amd import capi
from dl3_amd import utils as U
from oracle import dl3_oracle as DO
from tests import aug_oracle as O
from tests import resize_oracle as R

pytestmark = pytest.mark.gpu

C = 21
NB_TRAIN = dict(blur=5, horizontal_flip=True, brightness=0.3, zoom=0.1, rotation=5.0, do_ahisteq=True)

# one ragged batch to 32x32: (size, blur, crop origin).  37 * 50 = 1850 pixels first: every later map starts off a
# 4-byte boundary (1850, 2106, ...), and so do the images (3 * 1850 bytes)
BATCH9 = [((37, 50), 1, None), ((16, 16), 0, None), ((64, 64), 0, None), ((64, 50), 1, None), ((1, 1), 0, None),
          ((2, 33), 0, None), ((33, 2), 1, None), ((32, 32), 1, None), ((40, 48), 1, (5, 3))]
BATCH1 = [((40, 24), 1, None)]          # to 17x19: H * W odd, the byte stores


def _source(hw, seed, ldtype):
    rng = np.random.default_rng(seed)
    H, W = hw
    yy, xx = np.mgrid[:H, :W]
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    img[..., 0] = (img[..., 0] // 4 + (xx * 3 + yy) % 192).astype(np.uint8)
    lab = np.zeros(hw, ldtype)
    lab[(xx + seed) % 12 < 6] = 10
    lab[yy > H * 2 // 3] = 7
    lab[(yy + xx) % 23 == 0] = 255
    if H > 1 and W > 1:
        lab[1, 1] = 5                   # one pixel a shrinking nearest resize skips: in the source's set only
    if ldtype == np.int32:
        lab[0, 0] = 70000               # outside 0..255: carried by the resize, absent from the label set
    return img, lab


def _batch(spec, ldtype):
    src = [_source(hw, 11 + n, ldtype) for n, (hw, _, _) in enumerate(spec)]
    return [s[0] for s in src], [s[1] for s in src], [b for _, b, _ in spec], [c for _, _, c in spec]


def _front(images, labels, dst, blur, crops):
    B = len(images)
    tab, offs, info = A.front_tables([i.shape[:2] for i in images], dst, crops, blur)
    ipool, lpool = A.pack_pools(images, labels)
    dtab, di, dl = (torch.from_numpy(a).cuda() for a in (tab, ipool, lpool))
    out = torch.full((B,) + dst + (3,), 0xA5, dtype=torch.uint8, device="cuda")
    lout = torch.full((B,) + dst, 99, dtype=dl.dtype, device="cuda")
    present = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
    ws = torch.full((A.front_workspace_bytes(info),), 0x5A, dtype=torch.uint8, device="cuda")
    A.launch_front(info, dtab, offs, di, dl, out, lout, present, ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lout.cpu().numpy(), present.cpu().numpy()


@pytest.mark.parametrize("ldtype", [np.uint8, np.int32], ids=["uint8", "int32"])
@pytest.mark.parametrize("spec,dst", [(BATCH9, (32, 32)), (BATCH1, (17, 19))], ids=["B9-32x32", "B1-17x19"])
def test_front_end_matches_the_oracle_bit_exactly(spec, dst, ldtype):
    images, labels, blur, crops = _batch(spec, ldtype)
    got, lgot, present = _front(images, labels, dst, blur, crops)
    want, lwant = R.front_batch(images, labels, dst, blur, crops)
    for n in range(len(images)):
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, ("image %d %r differs at %d places, first %s: gpu %s oracle %s"
                               % (n, spec[n], len(bad), bad[0], got[n][tuple(bad[0])], want[n][tuple(bad[0])]))
        np.testing.assert_array_equal(lgot[n], lwant[n], err_msg="label map %d %r" % (n, spec[n]))
        # the set of the SOURCE map (np.unique before the resize, utils.py:317)
        np.testing.assert_array_equal(present[n], R.present_bits(labels[n]), err_msg="label set %d" % n)
        vals = [v for v in range(256) if (int(present[n][v >> 5]) >> (v & 31)) & 1]
        assert vals == [int(v) for v in np.unique(labels[n]) if 0 <= v < 256]
    # the case is only worth its name if a shrink lost a label the source had
    assert any(set(np.unique(l)) - set(np.unique(r)) for l, r in zip(labels, lwant)) or len(images) == 1


def test_error_codes():
    L = capi.lib()
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    b = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p, q = t.data_ptr(), b.data_ptr()

    def call(H=2, W=2, hs=2, ws=2, ldt=capi.LABEL_U8, out=q, lout=q, blur=0, wsb=0):
        return L.dl3_cv_resize(q, 12, q, ldt, 1, hs, ws, H, W, blur, p, p, out, lout, None, None, wsb, None)

    assert call(H=0) == -1 and call(W=0) == -1 and call(hs=0) == -1 and call(ws=-3) == -1
    assert "positive" in L.dl3_last_error().decode()
    assert call(ldt=7) == -4
    assert call(out=None) == -1          # a pool without its output
    assert call(blur=1) == -1            # blur without a workspace
    assert "workspace" in L.dl3_last_error().decode()
    # dl3_augment_present without the sets
    assert L.dl3_augment_present(q, q, 0, 1, 4, 4, 4, 4, 0, p, p, None, None, None, 3, None, p, q, None, 0, None) == -1


def test_cv_resize_round_trip():
    images, labels, _, _ = _batch(BATCH9[:4], np.uint8)
    got = A.cv_resize(images, (24, 40))                      # cv2's (width, height)
    assert got.shape == (4, 40, 24, 3) and got.dtype == np.uint8
    for g, i in zip(got, images):
        np.testing.assert_array_equal(g, R.resize_linear(i, (40, 24)))
    # a mask back to its image's size, nearest; int64 class ids come back as int32
    m = A.cv_resize(labels[0].astype(np.int64) * 1000, (100, 74), interpolation="nearest")
    assert m.shape == (74, 100) and m.dtype == np.int32
    np.testing.assert_array_equal(m, R.resize_nearest(labels[0].astype(np.int32) * 1000, (74, 100)))
    lm = A.cv_resize(labels, (32, 32), interpolation="nearest")
    assert lm.dtype == np.uint8
    for g, l in zip(lm, labels):
        np.testing.assert_array_equal(g, R.resize_nearest(l, (32, 32)))
    # one bare image in, one image out; up and back down by 2 is the identity (2x2 mean of a doubled image)
    one = A.cv_resize(images[1], (32, 32))
    np.testing.assert_array_equal(one, R.resize_linear(images[1], (32, 32)))
    np.testing.assert_array_equal(A.cv_resize(np.repeat(np.repeat(images[1], 2, 0), 2, 1), (16, 16)), images[1])
    np.testing.assert_array_equal(A.cv_resize(images[2], (64, 64)), images[2])


GEN_SIZES = [(37, 50), (16, 16), (64, 64), (40, 48), (33, 34), (64, 50)]


@pytest.mark.parametrize("shape_kw,opts", [(dict(crop_shape=(32, 32)), NB_TRAIN), (dict(resize_shape=(32, 32)), NB_TRAIN),
                                           (dict(resize_shape=(32, 32)), {}),
                                           (dict(crop_shape=(32, 32)), dict(blur=5, vertical_flip=True))],
                         ids=["crop-notebook", "resize-notebook", "resize-plain", "crop-blur-vflip"])
def test_generator_batches_match_the_oracles(shape_kw, opts):
    """gen[i] = the resize oracle (blur, resize or per-image crop) followed by aug_oracle's chain, bit for bit; warp + CLAHE
    at 32x32 in the notebook's flag set; every flag off: X is the widened resized image (the notebook's calculate_iou
    generator)"""
    src = [_source(hw, 40 + n, np.uint8) for n, hw in enumerate(GEN_SIZES)]
    imgs, labs = [s[0] for s in src], [s[1] for s in src]
    kw = dict(n_classes=C, batch_size=3, seed=12, device_resize=True, **shape_kw, **opts)
    g, twin = U.SegmentationGenerator(imgs, labs, **kw), U.SegmentationGenerator(imgs, labs, **kw)
    plan = twin.plan
    cropped = 0
    for i in range(2):
        X, Y, SW = g[i]
        im, lb, ps = twin.raw_batch(i)
        crops = [(p.cx, p.cy) if (shape_kw.get("crop_shape") and 32 < a.shape[1] and 32 < a.shape[0]) else None
                 for a, p in zip(im, ps)]
        cropped += sum(c is not None for c in crops)
        fi, fl = R.front_batch(im, lb, (32, 32), [p.blur for p in ps], crops)
        rest = [p._replace(blur=False, cx=0, cy=0) for p in ps]
        Xo, Lo = O.augment_batch(fi, fl, rest, (32, 32), plan.warp, plan.histeq, C)
        assert isinstance(X, np.ndarray) and X.dtype == np.float32
        np.testing.assert_array_equal(X, Xo)
        # the void relabel reads the SOURCE map's label set: aug_oracle's chain with that set in place of the resized map's
        Ls = np.stack([R.chain_image(a, b, s, p, plan.warp, plan.histeq, C)[1] for a, b, s, p in zip(fi, fl, lb, rest)])
        for n in range(3):
            if set(np.unique(lb[n])) == set(np.unique(fl[n])):
                np.testing.assert_array_equal(Ls[n], Lo[n])
        Yo, SWo, _ = DO.prepare_targets(Ls.reshape(3, -1), C)
        np.testing.assert_array_equal(Y.cpu().numpy(), Yo)
        np.testing.assert_array_equal(SW["pred_mask"].cpu().numpy(), SWo)
        if not opts:
            np.testing.assert_array_equal(X, fi.astype(np.float32))
    assert cropped == (5 if "crop_shape" in shape_kw else 0)   # 37x50, 64x64, 40x48, 33x34, 64x50 crop; 16x16 resizes


def test_device_feed_of_a_ragged_generator_trains_like_its_host_batches():
    """fit_generator(device_feed=True) over images of different sizes (crop_shape: some crop, some resize; the feeder's
    slots hold the packed pools) gives the losses fit_generator gets from a twin generator's gen[i], bit for bit"""
    from tests.test_gpu_model import _build, _load
    classes, shape = 5, (64, 64, 3)
    rng = np.random.default_rng(23)
    sizes = [(80, 72), (64, 64), (50, 70), (100, 90), (64, 80), (72, 72)]
    imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes]
    labs = [rng.integers(0, classes, hw, dtype=np.uint8) for hw in sizes]
    for l in labs:
        l[:10] = 255

    def run(device_feed):
        model, params = _build("mobilenetv2", shape, classes, "deeplab")
        _load(model, params)
        model.compile(optimizer=dict(lr=1e-3))
        g = U.SegmentationGenerator(imgs, labs, n_classes=classes, batch_size=2, seed=31, crop_shape=(64, 64),
                                    device_resize=True, **NB_TRAIN)
        return model.fit_generator(g, epochs=1, device_feed=device_feed, n_classes=classes)

    host = run(False)
    fed = run(True)
    assert len(host) == 3 and all(np.isfinite(host))
    assert fed == host, (fed, host)
