"""CPU tests of the device cv2.resize front end: known answers of the numpy oracle (tests/resize_oracle.py) and its
distance from float64 bilinear, the host tables of augment.resize_tables against the oracle's, the border rules, the
parameter stream of a generator over images of different sizes against a hand replay of the reference's call order
(utils.py:319-350, :411-423), the keyword's default (off: today's behaviour, the pinned refusal included), argument
checks and the C ABI."""
import random

import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import augment as A
from dl3_amd import capi
from dl3_amd.utils import SegModel, SegmentationGenerator
from tests import resize_oracle as R

# (source, destination) as (H, W): up, down, 1x1 source, 2-wide sources, a VOC size to 512x512, exact 2x shrink
SHAPES = [((37, 50), (32, 32)), ((16, 16), (32, 32)), ((64, 64), (32, 32)), ((64, 50), (32, 32)), ((1, 1), (32, 32)),
          ((2, 33), (32, 32)), ((33, 2), (32, 32)), ((40, 24), (17, 19)), ((5, 5), (3, 3)), ((3, 3), (7, 7)),
          ((375, 500), (512, 512))]
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in SHAPES]


def _plane(hw, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, hw, dtype=np.uint8)


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_oracle_is_within_one_grey_level_of_float_bilinear(src, dst):
    """11-bit coefficients and two truncating shifts: the integer path may differ from the float64 value by less than
    one grey level; it never leaves 0..255 (so the uint8 store keeps every value)"""
    img = _plane(src, 3)
    img.flat[0], img.flat[-1] = 255, 0
    wide = R.resize_linear_wide(img, dst)
    assert wide.min() >= 0 and wide.max() <= 255
    assert np.abs(wide - R.float_bilinear(img, dst)).max() < 1.0
    if dst[0] * dst[1] <= 2048:
        np.testing.assert_array_equal(R.resize_linear(img, dst), wide.astype(np.uint8))


@pytest.mark.parametrize("src,dst", SHAPES[:10], ids=IDS[:10])
def test_oracle_maps_a_constant_image_to_itself(src, dst):
    for v in (0, 1, 77, 254, 255):
        out = R.resize_linear(np.full(src + (3,), v, np.uint8), dst)
        assert out.shape == dst + (3,) and (out == v).all()


def test_oracle_identity_and_two_times_shrink():
    img = np.random.default_rng(0).integers(0, 256, (24, 36, 3), dtype=np.uint8)
    np.testing.assert_array_equal(R.resize_linear(img, (24, 36)), img)
    # equal sizes through the formula itself (not the shortcut): s = d, f = 0 -> (2048 * (p * 2048 >> 4) >> 16) + 2 >> 2 = p
    for d in range(36):
        assert R.column_taps(d, 36, 36)[2:] == (2048, 0) and R.column_taps(d, 36, 36)[0] == d
    p = img.astype(np.int64)
    mean = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    np.testing.assert_array_equal(R.resize_linear(img, (12, 18)), mean.astype(np.uint8))


def test_nearest_index_rule_by_hand():
    # 5 -> 3: scale 5/3; floor(0), floor(1.67), floor(3.33)
    assert [R.nearest_index(d, 5, 3) for d in range(3)] == [0, 1, 3]
    # 3 -> 7: scale 1 / (7/3) = 0.428...; d * scale = 0, .43, .86, 1.29, 1.71, 2.14, 2.57
    assert [R.nearest_index(d, 3, 7) for d in range(7)] == [0, 0, 0, 1, 1, 2, 2]
    # 1 -> 4: everything reads the one pixel; 4 -> 4: identity
    assert [R.nearest_index(d, 1, 4) for d in range(4)] == [0] * 4
    assert [R.nearest_index(d, 4, 4) for d in range(4)] == [0, 1, 2, 3]
    lab = np.arange(15, dtype=np.int32).reshape(3, 5) * 1000
    np.testing.assert_array_equal(R.resize_nearest(lab, (7, 3)), lab[[0, 0, 0, 1, 1, 2, 2]][:, [0, 1, 3]])


def test_border_rules():
    # 16 -> 32, d = 0: f = 0.25 - 0.5 = -0.25 -> s = -1, fraction 0.75
    assert R.linear_coord(0, 16, 32) == (-1, np.float32(0.75))
    # columns: s < 0 -> s = 0, f = 0
    assert R.column_taps(0, 16, 32) == (0, 1, 2048, 0)
    # rows keep the fraction and clip both taps: rows (0, 0), coefficients (512, 1536)
    assert R.row_taps(0, 16, 32) == (0, 0, 512, 1536)
    # d = 31: f = 15.25 -> s = 15 >= Ws - 1: column s = 15, f = 0, second tap min(16, 15)
    assert R.column_taps(31, 16, 32) == (15, 15, 2048, 0)
    assert R.row_taps(31, 16, 32) == (15, 15, 1536, 512)
    # a 1-pixel axis: every coordinate reads pixel 0 twice
    for d in range(5):
        assert R.column_taps(d, 1, 5)[:2] == (0, 0) and R.row_taps(d, 1, 5)[:2] == (0, 0)
    # 5 -> 3 by hand: f = (d + .5) * 5/3 - .5 = 1/3, 2, 3 2/3
    assert [R.column_taps(d, 5, 3) for d in range(3)] == [(0, 1, 1365, 683), (2, 3, 2048, 0), (3, 4, 683, 1365)]


# ---------------------------------------------------------------- the host tables
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_resize_tables_equal_the_oracle(src, dst):
    np.testing.assert_array_equal(A.resize_tables(src, dst), R.tables(src, dst))
    t = A.resize_tables(src, dst)
    assert t.dtype == np.int32 and t.size == 4 * dst[1] + 4 * dst[0]


def test_front_tables_layout_and_dedup():
    sizes = [(37, 50), (16, 16), (37, 50), (40, 48), (37, 50)]
    tab, offs, info = A.front_tables(sizes, (32, 32), crops=[None, None, None, (3, 5), None], blur=[1, 0, 0, 1, 0])
    B = len(sizes)
    desc = tab[:B * A.FRONT_DESC].reshape(B, A.FRONT_DESC)
    px = np.array([h * w for h, w in sizes])
    start = np.concatenate([[0], np.cumsum(px)[:-1]])
    np.testing.assert_array_equal(desc[:, 0], 3 * start)
    np.testing.assert_array_equal(desc[:, 1], start)
    assert desc[:, 2:4].tolist() == [list(s) for s in sizes]
    assert desc[:, 4].tolist() == [1, 0, 0, 1, 0] and desc[:, 5].tolist() == [0, 0, 0, 1, 0]
    assert desc[3, 6:8].tolist() == [3, 5]
    # two distinct resized sizes -> two tables; the three 37x50 images share one
    assert tab.size == B * A.FRONT_DESC + 2 * 8 * 32 and desc[0, 8] == desc[2, 8] == desc[4, 8] == 0 and desc[1, 8] == 256
    assert offs == {"fdesc": 0, "ftab": B * A.FRONT_DESC}
    np.testing.assert_array_equal(tab[offs["ftab"] + 256:], R.tables((16, 16), (32, 32)))
    assert info == A.FrontInfo(B, 32, 32, 40, 50, 1, int(px.sum()))
    assert desc[1, 1] % 4 != 0   # 37 * 50 = 1850: maps do not start on a 4-byte boundary


def test_descriptors_are_checked_before_upload():
    with pytest.raises(ValueError, match="crop"):
        A.front_tables([(40, 48)], (32, 32), crops=[(17, 0)])
    with pytest.raises(ValueError, match="crop"):
        A.front_tables([(20, 48)], (32, 32), crops=[(0, 0)])
    with pytest.raises(ValueError, match="empty"):
        A.front_tables([(0, 48)], (32, 32))
    with pytest.raises(ValueError, match="pool"):
        A.front_tables([(8, 8), (8, 8)], (4, 4), pool_px=100)
    with pytest.raises(ValueError, match="pool"):
        A.front_tables([(8, 8)], (4, 4), px_offsets=[-1])
    with pytest.raises(ValueError, match="positive"):
        A.front_tables([(8, 8)], (0, 4))


# ---------------------------------------------------------------- the generator
def _ragged(sizes, seed=0, ldtype=np.uint8):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes],
            [rng.integers(0, 4, hw).astype(ldtype) for hw in sizes])


def test_ragged_draw_stream_is_the_reference_call_order():
    """crop_shape = (32, 32): the 40x48 images crop (two randrange draws), the 20x60 and 32x64 ones resize (no draw: the
    crop must be smaller BOTH ways, utils.py:415) — in one batch"""
    sizes = [(40, 48), (20, 60), (32, 64), (48, 40)]
    imgs, labs = _ragged(sizes)
    g = SegmentationGenerator(imgs, labs, n_classes=4, batch_size=4, seed=13, crop_shape=(32, 32), blur=5,
                              horizontal_flip=True, brightness=0.2, zoom=0.1, shuffle=False, device_resize=True)
    im, lb, got = g.raw_batch(0)
    r = random.Random(13)
    want = []
    for hs, ws in sizes:
        b = bool(r.randint(0, 1))
        cx = cy = 0
        if 32 < ws and 32 < hs:
            cx = r.randrange(ws - 32)
            cy = r.randrange(hs - 32)
        hf = bool(r.randint(0, 1))
        gm = 1.0 + r.gauss(mu=0.0, sigma=0.2)
        if r.randint(0, 1):
            gm = 1.0 / gm
        want.append(A.ImageParams(b, cx, cy, hf, False, gm, 0.0, r.gauss(mu=1.0, sigma=0.1)))
    assert got == want
    assert [g.plan.crops(s) for s in sizes] == [True, False, False, True]
    assert all(a is b for a, b in zip(im, imgs)) and all(a is b for a, b in zip(lb, labs))
    assert (g.plan.H, g.plan.W) == (32, 32) and g.pool_pixels == sum(h * w for h, w in sizes)
    # resize_shape alone draws no crop at all
    g = SegmentationGenerator(imgs, labs, n_classes=4, batch_size=2, seed=13, resize_shape=(24, 16), device_resize=True)
    assert g.raw_batch(0)[2] == [A.ImageParams(False, 0, 0, False, False, None, 0.0, 1.0)] * 2
    assert (g.plan.H, g.plan.W) == (16, 24) and g.random.random() == random.Random(13).random()
    assert g.pool_pixels == 48 * 40 + 32 * 64


def test_keyword_off_is_todays_behaviour():
    imgs = np.zeros((6, 64, 64, 3), np.uint8)
    labs = np.zeros((6, 64, 64), np.uint8)
    with pytest.raises(ValueError, match="resize"):
        SegModel(image_size=(32, 32)).create_generators(images=imgs, labels=labs)
    with pytest.raises(ValueError, match="resize"):
        SegmentationGenerator(imgs, labs, resize_shape=(32, 32))
    ri, rl = _ragged([(40, 48), (20, 60)])
    with pytest.raises(Exception):
        SegmentationGenerator(ri, rl, resize_shape=(32, 32))
    with pytest.raises(Exception):
        SegModel(image_size=(32, 32)).create_generators(images=ri, labels=rl)
    # ... and with it on the same calls are served
    g = SegModel(image_size=(32, 48)).create_generators(images=imgs, labels=labs, device_resize=True, validation_split=.5)
    assert g.device_resize and (g.plan.H, g.plan.W) == (32, 48) and len(g.images) == 3
    g = SegModel(image_size=(32, 32)).create_generators(images=ri * 3, labels=rl * 3, device_resize=True, mode="validation",
                                                        validation_split=.5, seed=3)
    x = np.random.RandomState(3).permutation(6)[:3]
    assert [i.shape for i in g.images] == [(ri * 3)[j].shape for j in x]


def test_argument_checks():
    ri, rl = _ragged([(40, 48), (20, 60)])
    with pytest.raises(ValueError, match="resize_shape or crop_shape"):
        SegmentationGenerator(ri, rl, device_resize=True)
    with pytest.raises(ValueError, match="label map"):
        SegmentationGenerator(ri, rl[::-1], resize_shape=(8, 8), device_resize=True)
    with pytest.raises(ValueError, match="one label map per image"):
        SegmentationGenerator(ri, rl[:1], resize_shape=(8, 8), device_resize=True)
    with pytest.raises(ValueError, match="uint8"):
        SegmentationGenerator([i.astype(np.float32) for i in ri], rl, resize_shape=(8, 8), device_resize=True)
    with pytest.raises(ValueError, match="int32"):
        SegmentationGenerator(ri, [l.astype(np.int32) for l in rl], resize_shape=(8, 8), zoom=0.1, device_resize=True)
    with pytest.raises(ValueError, match="blur"):
        SegmentationGenerator(ri, rl, resize_shape=(8, 8), blur=3, device_resize=True)
    # a uniform array needs no shape: the images keep their size
    u = SegmentationGenerator(np.zeros((2, 8, 9, 3), np.uint8), np.zeros((2, 8, 9), np.uint8), device_resize=True)
    assert (u.plan.H, u.plan.W) == (8, 9)
    with pytest.raises(ValueError, match="interpolation"):
        A.cv_resize(ri, (8, 8), interpolation="cubic")
    with pytest.raises(ValueError, match="dsize"):
        A.cv_resize(ri, (0, 8))
    with pytest.raises(ValueError, match="linear"):
        A.cv_resize(rl, (8, 8))
    with pytest.raises(ValueError, match="nearest"):
        A.cv_resize(ri, (8, 8), interpolation="nearest")
    with pytest.raises(ValueError, match="src_hw"):
        A.Plan(None, resize_shape=(8, 8))


def test_ragged_batches_cannot_be_sharded():
    """under distribute() a device_resize generator is refused before anything is built or drawn"""
    import types
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=(32, 32, 3), classes=3, backbone="mobilenetv2", OS=16)
    model._dp = types.SimpleNamespace(world=2, comm=None)
    ri, rl = _ragged([(40, 48), (20, 60)])
    g = SegmentationGenerator(ri, rl, n_classes=3, batch_size=2, resize_shape=(32, 32), horizontal_flip=True,
                              device_resize=True)
    with pytest.raises(ValueError, match="distribute"):
        model.fit_generator(g, device_feed=True, n_classes=3)
    assert g.random.random() == random.Random(7).random()


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_resize_entry_points():
    protos = capi.parse_header()
    ret, args = protos["dl3_cv_resize"]
    assert ret == "int" and [n for _, n in args] == [
        "image_pool", "image_pool_bytes", "label_pool", "label_dtype", "B", "max_hs", "max_ws", "H", "W", "blur_any", "desc",
        "tab", "images_out", "labels_out", "present", "workspace", "workspace_bytes", "stream"]
    ret, args = protos["dl3_cv_resize_workspace_bytes"]
    assert ret == "size_t" and [n for _, n in args] == ["image_pool_bytes", "blur_any"]
    # the sibling of dl3_augment: the same arguments with `present` in front of the outputs
    aug, sib = protos["dl3_augment"], protos["dl3_augment_present"]
    assert sib[0] == "int" and [a for a in sib[1] if a[1] != "present"] == aug[1]
    assert [n for _, n in sib[1]].index("present") == [n for _, n in aug[1]].index("X")
    names = ("dl3_cv_resize", "dl3_cv_resize_workspace_bytes", "dl3_augment_present")
    assert all(t in capi._CTYPES for name in names for t, _ in protos[name][1])
    assert "THE DEVICE TRUSTS desc AND tab" in open(capi.HEADER).read()


def test_library_exports_the_resize_entry_points(lib):
    for name in ("dl3_cv_resize", "dl3_cv_resize_workspace_bytes", "dl3_augment_present"):
        assert getattr(lib, name).restype is not None
    assert lib.dl3_cv_resize_workspace_bytes(1000, 0) == 0
    assert lib.dl3_cv_resize_workspace_bytes(1000, 1) == 1024
