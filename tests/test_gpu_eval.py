"""-m gpu: the evaluation tail (dl3_eval_tail_*), the engine's evaluation plan, Model.evaluate(device=True) /
evaluate_generator / confusion_matrix, and fit / fit_generator with validation_data= and callbacks=.

Bounds (none of them tuned to the device's output):
  * mask — bit for bit the existing kernels' (dl3_resize_bilinear_fwd / dl3_phase_shift + dl3_argmax); against the float64
    oracle equal wherever the float64 top-two margin exceeds tau = 32 * 2^-24 * max|logit| (three roundings per lerp,
    two lerp levels, two candidates -> <= 24 units of 2^-24 * max; 32 leaves a third on top); the pixels under tau must
    be <= 0.1 % of a case, asserted on the float64 margins before the device result is looked at.
  * counts / nnz / confusion — exactly numpy's integers from the DEVICE's mask and the labels.
  * loss_sum — |device - float64| / |float64| per image <= 2 x the same distance of the oracle's own float32 run (the
    yardstick and factor of tests/test_gpu_crf.py: a float32 evaluation in another summation order cannot be asked to be
    closer than float32 itself; 2 covers the order).
  * two runs bit-identical in every output.

Measured on the MI355X, loss_sum, worst case of each form, device distance / float32-oracle distance: see DESIGN.md §10.
"""
import numpy as np
import pytest

from tests import eval_oracle as EO

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- operator
def _inputs(form, dims, C, N, seed):
    """standard normal logits from default_rng(seed); labels with void pixels; weights with zeros"""
    rng = np.random.default_rng(seed)
    if form == "bilinear":
        Hi, Wi, Ho, Wo = dims
        x = rng.standard_normal((N, Hi, Wi, C)).astype(np.float32)
        shape = (Ho, Wo)
    elif form == "shuffle":
        H, W, r = dims
        x = rng.standard_normal((N, H, W, C * r * r)).astype(np.float32)
        Ho, Wo, shape = H * r, W * r, r
    else:
        Ho, Wo = dims
        x = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
        shape = None
    labels = rng.integers(0, C + 1, (N, Ho, Wo)).astype(np.float32)   # C = void
    weights = (rng.random((N, Ho, Wo)) * (rng.random((N, Ho, Wo)) > 0.25)).astype(np.float32)
    return x, shape, labels, weights, Ho, Wo


def _device_tail(form, x, dims, C, N, labels, weights, Ho, Wo, conf, want_mask=True):
    """one call through the C ABI -> dict of host arrays (conf: the int64 device tensor the call accumulates into)"""
    import torch
    from tests import gpu_util as GU
    from dl3_amd import capi
    L = capi.lib()
    dx, dl = GU.dev(x), GU.dev(labels)
    dw = GU.dev(weights) if weights is not None else None
    if form == "bilinear":
        Hi, Wi = dims[0], dims[1]
        P = L.dl3_eval_tail_bilinear_partials(N, Hi, Wi, Ho, Wo, C)
        tail = (N, Hi, Wi, Ho, Wo, C)
    elif form == "shuffle":
        H, W, r = dims
        P = L.dl3_eval_tail_shuffle_partials(N, H, W, C, r)
        tail = (N, H, W, C, r)
    else:
        P = L.dl3_eval_tail_plain_partials(N, Ho * Wo, C)
        tail = (N, Ho * Wo, C)
    assert P > 0, "the %s form refuses %r x %d" % (form, dims, C)
    part = torch.full((N * P,), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    nnz = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((N, 3, C), -1, dtype=torch.int32, device="cuda")
    mask = torch.full((N, Ho, Wo), -1, dtype=torch.int32, device="cuda") if want_mask else None
    GU._KEEP.extend([part, loss, nnz, counts, mask, conf])
    GU.call("dl3_eval_tail_" + form, GU.ptr(dx), GU.ptr(dl), GU.ptr(dw), part.data_ptr(), loss.data_ptr(), nnz.data_ptr(),
            counts.data_ptr(), conf.data_ptr() if conf is not None else None, mask.data_ptr() if want_mask else None, *tail)
    torch.cuda.synchronize()
    return dict(loss_sum=loss.cpu().numpy(), nnz=nnz.cpu().numpy(), counts=counts.cpu().numpy(),
                mask=mask.cpu().numpy() if want_mask else None, part=part.cpu().numpy())


def _existing_mask(form, x, dims, C, N, Ho, Wo):
    """the parent commit's kernels: dl3_resize_bilinear_fwd / dl3_phase_shift, then dl3_argmax"""
    import torch
    from tests import gpu_util as GU
    dx = GU.dev(x)
    if form == "plain":
        full = dx
    else:
        full = GU.empty(N * Ho * Wo * C)
        if form == "bilinear":
            GU.call("dl3_resize_bilinear_fwd", GU.ptr(dx), C, None, None, 0, GU.ptr(full), C, N, dims[0], dims[1], Ho, Wo, C)
        else:
            GU.call("dl3_phase_shift", GU.ptr(dx), GU.ptr(full), N, dims[0], dims[1], C, dims[2], 0)
    out = torch.full((N * Ho * Wo,), -1, dtype=torch.int32, device="cuda")
    GU._KEEP.append(out)
    GU.call("dl3_argmax", GU.ptr(full), out.data_ptr(), N * Ho * Wo, C)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(N, Ho, Wo)


BILINEAR = [  # (Hi, Wi, Ho, Wo), C, N, weights?
    ((8, 8, 64, 64), 2, 3, True), ((8, 8, 64, 64), 3, 1, False), ((8, 8, 64, 64), 21, 3, False),
    ((8, 8, 64, 64), 32, 3, True), ((20, 20, 320, 320), 21, 1, True), ((20, 20, 320, 320), 3, 3, False),
    ((64, 64, 512, 512), 21, 1, True), ((33, 33, 513, 513), 32, 1, False), ((33, 33, 513, 513), 2, 1, True),
    ((16, 24, 128, 192), 21, 3, True), ((16, 24, 128, 192), 2, 1, False),
]
SHUFFLE = [  # (H, W, r), C, N, weights?
    ((8, 8, 8), 2, 3, True), ((8, 8, 8), 21, 1, False), ((8, 8, 8), 32, 3, True), ((16, 16, 4), 3, 3, False),
    ((16, 16, 4), 32, 1, True), ((80, 80, 4), 21, 1, True), ((64, 64, 8), 21, 1, False), ((16, 24, 8), 3, 3, True),
    ((32, 48, 4), 21, 3, False),
]
PLAIN = [  # (Ho, Wo), C, N, weights?
    ((64, 64), 2, 3, True), ((64, 64), 3, 1, False), ((64, 64), 21, 3, True), ((64, 64), 32, 1, False),
    ((64, 64), 40, 3, True), ((128, 192), 40, 1, False), ((320, 320), 21, 1, True), ((513, 513), 3, 1, True),
]
CASES = [("bilinear",) + c for c in BILINEAR] + [("shuffle",) + c for c in SHUFFLE] + [("plain",) + c for c in PLAIN]


@pytest.mark.parametrize("form,dims,C,N,weighted", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_eval_tail_operator(form, dims, C, N, weighted):
    import torch
    x, shape, labels, weights, Ho, Wo = _inputs(form, dims, C, N, seed=0)
    if not weighted:
        weights = None
    ref = EO.eval_tail(form, x, shape, labels, weights, np.float64)
    f32 = EO.eval_tail(form, x, shape, labels, weights, np.float32)
    # the input itself must be decidable: pixels whose float64 top-two margin is within tau, at most 0.1 %
    tau = 32.0 * 2.0 ** -24 * float(np.abs(ref["logits"]).max())
    unsure = ref["margin"] <= tau
    print("%s %r C=%d N=%d: %d of %d pixels under tau=%.3g" % (form, dims, C, N, unsure.sum(), unsure.size, tau))
    assert unsure.mean() <= 1e-3

    conf = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    a = _device_tail(form, x, dims, C, N, labels, weights, Ho, Wo, conf)
    conf1 = conf.cpu().numpy().copy()
    b = _device_tail(form, x, dims, C, N, labels, weights, Ho, Wo, conf)
    conf2 = conf.cpu().numpy().copy()

    # mask: the existing kernels', bit for bit; the oracle's wherever it is decidable
    assert np.array_equal(a["mask"], _existing_mask(form, x, dims, C, N, Ho, Wo))
    assert np.array_equal(a["mask"][~unsure], ref["mask"][~unsure])
    # integers: exactly numpy's from the DEVICE's mask
    from oracle import dl3_oracle as O
    assert np.array_equal(a["counts"], O.seg_counts(a["mask"], labels, C))
    w = np.ones_like(labels) if weights is None else weights
    assert np.array_equal(a["nnz"], (w != 0).reshape(N, -1).sum(1))
    cm = EO.confusion(a["mask"], labels, C)
    assert np.array_equal(conf1, cm)
    assert np.array_equal(conf2, 2 * cm)   # it accumulates across calls
    # loss: the float32 oracle's own distance to float64 is the yardstick
    for n in range(N):
        r64 = ref["loss_sum"][n]
        d_dev = abs(a["loss_sum"][n] - r64) / abs(r64)
        d_f32 = abs(float(f32["loss_sum"][n]) - r64) / abs(r64)
        print("  image %d: loss_sum device %.9g float64 %.9g | device %.3e float32-oracle %.3e ratio %.2f"
              % (n, a["loss_sum"][n], r64, d_dev, d_f32, d_dev / max(d_f32, 1e-300)))
        assert d_dev <= 2.0 * d_f32
    # two runs: bit-identical in every output
    for k in ("loss_sum", "nnz", "counts", "mask", "part"):
        assert np.array_equal(a[k], b[k]), k


def test_eval_tail_nullable_outputs_and_refusals():
    """mask = NULL and confusion = NULL leave the other outputs unchanged; shapes the fused forms do not support answer
    0 from the query"""
    from dl3_amd import capi
    import torch
    L = capi.lib()
    assert L.dl3_eval_tail_bilinear_partials(1, 8, 8, 64, 64, 33) == 0
    assert L.dl3_eval_tail_shuffle_partials(1, 8, 8, 40, 4) == 0
    assert L.dl3_eval_tail_bilinear_partials(1, 64, 512, 512, 4096, 32) == 0   # two source rows exceed the LDS stage
    assert L.dl3_eval_tail_plain_partials(1, 4096, 40) > 0
    for form, dims in (("bilinear", (8, 8, 64, 64)), ("shuffle", (8, 8, 8)), ("plain", (64, 64))):
        x, shape, labels, weights, Ho, Wo = _inputs(form, dims, 21, 2, seed=1)
        conf = torch.zeros(21, 21, dtype=torch.int64, device="cuda")
        a = _device_tail(form, x, dims, 21, 2, labels, weights, Ho, Wo, conf)
        b = _device_tail(form, x, dims, 21, 2, labels, weights, Ho, Wo, None, want_mask=False)
        for k in ("loss_sum", "nnz", "counts"):
            assert np.array_equal(a[k], b[k]), (form, k)


@pytest.mark.parametrize("C", [5, 21])
def test_eval_tail_bilinear_variants_agree(C):
    """dl3_eval_tail_bilinear has a 16-byte variant (Wo % 4 == 0; labels, weights and mask 16-byte aligned: a lane owns four
    pixels) and a scalar one.  Both interpolate the loss's logits with the weight TF states (tailmath.h, Lerp::wl), so the
    per-pixel terms are the same floats and only the order of the 20 * 24 = 480 double additions of an image differs: at
    most 479 * 2^-53 = 5e-14 relative, asserted as 1e-12.  At 6x8 -> 20x24 both scale factors are inexact in float32 and
    the stated weight differs from the fused one (Lerp::w) at 11 of the 20 rows and 16 of the 24 columns; a fused weight
    along either axis moves loss_sum by 7e-9 to 3e-8 relative (numpy emulation), four orders above the bound."""
    import torch
    from tests import gpu_util as GU
    N, Hi, Wi, Ho, Wo = 2, 6, 8, 20, 24
    rng = np.random.default_rng(7)
    x = GU.dev(3.0 * rng.standard_normal((N, Hi, Wi, C)))
    labels = rng.integers(0, C, N * Ho * Wo).astype(np.float32)   # all legal
    from dl3_amd import capi
    P = capi.lib().dl3_eval_tail_bilinear_partials(N, Hi, Wi, Ho, Wo, C)
    assert P > 0
    out = {}
    for off in (0, 1):   # element offset into every per-pixel buffer: 0 -> the 16-byte variant, 1 -> the scalar one
        lab = GU.dev(np.concatenate([np.zeros(off, np.float32), labels]))
        wgt = GU.dev(np.ones(off + labels.size, np.float32))
        part = torch.full((N * P,), float("nan"), dtype=torch.float64, device="cuda")
        loss = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        nnz = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((N, 3, C), -1, dtype=torch.int32, device="cuda")
        mask = torch.full((off + N * Ho * Wo,), -1, dtype=torch.int32, device="cuda")
        GU._KEEP.extend([part, loss, nnz, counts, mask])
        assert (GU.ptr(lab, off) % 16 == 0) == (off == 0) and (GU.ptr(mask, off) % 16 == 0) == (off == 0)
        GU.call("dl3_eval_tail_bilinear", GU.ptr(x), GU.ptr(lab, off), GU.ptr(wgt, off), part.data_ptr(), loss.data_ptr(),
                nnz.data_ptr(), counts.data_ptr(), None, GU.ptr(mask, off), N, Hi, Wi, Ho, Wo, C)
        torch.cuda.synchronize()
        out[off] = dict(loss_sum=loss.cpu().numpy(), nnz=nnz.cpu().numpy(), counts=counts.cpu().numpy(),
                        mask=mask.cpu().numpy()[off:])
    a, b = out[0], out[1]
    assert np.array_equal(a["mask"], b["mask"])
    assert np.array_equal(a["nnz"], b["nnz"]) and np.array_equal(a["nnz"], np.full(N, Ho * Wo))
    assert np.array_equal(a["counts"], b["counts"])
    for n in range(N):
        d = abs(a["loss_sum"][n] - b["loss_sum"][n]) / abs(b["loss_sum"][n])
        print("C=%d image %d: loss_sum 16-byte %.17g scalar %.17g relative difference %.3e" % (C, n, a["loss_sum"][n],
                                                                                             b["loss_sum"][n], d))
        assert d <= 1e-12


# ------------------------------------------------------------------------------------------------- engine and model
def _model(backbone, head, classes=3, size=64, seed=1):
    import dl3_amd  # noqa: F401
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    from dl3_amd.utils import SegModel
    from oracle import dl3_oracle as O
    G.clear_session()
    if head == "deeplab":
        model = Deeplabv3(weights=None, input_shape=(size, size, 3), classes=classes, backbone=backbone, OS=16)
    else:
        model = SegModel(image_size=(size, size)).create_seg_model(head, n=classes, backbone=backbone)
    params = O.init_params(O.param_shapes(backbone, classes, head=head), seed=seed)
    for l in model.layers:
        if l.weights:
            l.set_weights([params[n] for n in l.weights])
    return model


def _data(n, classes, size=64, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, size, size, 3)).astype(np.float32)
    y = rng.integers(0, classes + 1, (n, size * size, 1)).astype(np.float32)
    sw = (rng.random((n, size * size)) * (rng.random((n, size * size)) > 0.3)).astype(np.float32)
    return x, y, sw


@pytest.mark.parametrize("head,gone", [("original", "dl3_resize_bilinear_fwd"), ("subpixel", "dl3_phase_shift")])
def test_engine_evaluation_plan(head, gone):
    """the plan holds neither the final resize / phase shift nor a softmax, and leaves the forward plan intact"""
    model = _model("mobilenetv2", head)
    x, y, sw = _data(2, 3)
    eng = model._engine(2, False)
    before_p, before_m = eng.predict(x), None
    eng.set_input(x)
    eng.forward()
    before_m = eng.argmax()
    names = eng.eval_op_names()
    assert names[-1] == "dl3_eval_tail_" + ("bilinear" if head == "original" else "shuffle")
    assert "dl3_softmax_fwd" not in names
    assert names.count(gone) == [r[0] for r in eng.ops_fwd].count(gone) - 1 and eng.ops_fwd[-1][0] == gone
    for _ in range(3):   # eager, capture, replay
        m = eng.evaluate_batch(x, y, sw, mask=True)
        assert np.array_equal(m.cpu().numpy(), before_m)
    loss, nnz, counts = eng.read_evaluation()
    assert loss.shape == (3, 2) and np.array_equal(loss[0], loss[1]) and np.array_equal(loss[0], loss[2])
    assert np.array_equal(nnz[0], (sw != 0).sum(1)) and np.array_equal(counts[0], counts[2])
    assert np.array_equal(eng.predict(x), before_p)
    eng.set_input(x)
    eng.forward()
    assert np.array_equal(eng.argmax(), before_m)


@pytest.mark.parametrize("backbone", ["mobilenetv2", "xception"])
@pytest.mark.parametrize("head", ["original", "subpixel"])
def test_model_evaluate_device(backbone, head):
    from oracle import dl3_oracle as O
    C = 3
    model = _model(backbone, head, classes=C)
    x, y, sw = _data(5, C)
    for w in (sw, None):
        host = model.evaluate(x, y, batch_size=5, sample_weight=w)          # ONE batch: the parent's host path
        devv = model.evaluate(x, y, batch_size=5, sample_weight=w, device=True)
        assert devv[1] == host[1] and devv[2] == host[2], (host, devv)
        # loss: the float32 oracle's distance on the device's own logits is the yardstick (rule of the operator test)
        eng = model._engine(5, False)
        eng.set_input(x)
        eng.forward()
        z = eng.logits()
        ww = np.ones((5, 64 * 64)) if w is None else w
        n = max(int((ww != 0).sum()), 1)
        l64 = float((EO.pixel_loss(z.reshape(5, -1, C), y[:, :, 0], np.float64) * ww).sum() / n)
        l32 = float((EO.pixel_loss(z.reshape(5, -1, C), y[:, :, 0], np.float32) * ww.astype(np.float32)).sum(dtype=np.float32) / n)
        d_dev, d_f32 = abs(devv[0] - host[0]) / abs(host[0]), abs(l32 - l64) / abs(l64)
        print("%s/%s weights=%s: loss host %.9g device %.9g | device %.3e float32 %.3e" %
              (backbone, head, w is not None, host[0], devv[0], d_dev, d_f32))
        assert d_dev <= 2.0 * d_f32
    # several batches with a ragged last one: the batch-size-weighted average of one host-path call per batch
    per, sizes = [], []
    for i in range(0, 5, 2):
        per.append(model.evaluate(x[i:i + 2], y[i:i + 2], batch_size=2, sample_weight=sw[i:i + 2]))
        sizes.append(len(x[i:i + 2]))
    want = EO.weighted_average(per, sizes)
    got = model.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    assert got[1] == pytest.approx(want[1], rel=1e-12) and got[2] == pytest.approx(want[2], rel=1e-12)
    assert got[0] == pytest.approx(want[0], rel=1e-6)

    class Gen:   # batches of 2, 2, 1 as a Sequence
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return x[2 * i:2 * i + 2], y[2 * i:2 * i + 2], {"pred_mask": sw[2 * i:2 * i + 2]}
    assert model.evaluate_generator(Gen()) == got
    cm = model.confusion_matrix(x, y, batch_size=2)
    t = y[:, :, 0].astype(np.int64).ravel()
    assert cm.dtype == np.int64 and np.array_equal(cm.sum(1), np.bincount(t[t < C], minlength=C))
    eng = model._engine(5, False)
    eng.set_input(x)
    eng.forward()
    assert np.array_equal(np.diag(cm), eng.seg_counts(y)[:, 2].sum(0))
    assert np.array_equal(model.confusion_matrix(Gen()), cm)


# ------------------------------------------------------------------------------------------------------- the loop
def _squares(n=24, H=64, W=64, seed=33):
    """bright squares on a dark, noisy background (the task of test_gpu_model.py::test_learns_a_toy_segmentation_task)"""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 60, (n, H, W, 3)).astype(np.uint8)
    labs = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        y0, x0 = rng.integers(4, 32, 2)
        s = rng.integers(16, 28)
        imgs[i, y0:y0 + s, x0:x0 + s] = rng.integers(180, 256, 3)
        labs[i, y0:y0 + s, x0:x0 + s] = 1
        labs[i, :2] = 255  # a void border
    return imgs, labs


def _loop_model():
    from dl3_amd import utils as U
    model = _model("mobilenetv2", "deeplab", classes=2)
    model.compile(optimizer=dict(lr=3e-3, epsilon=1e-8, decay=1e-6),
                  metrics={"pred_mask": [U.Jaccard, U.sparse_accuracy_ignoring_last_label]})
    return model


def _gens():
    from dl3_amd import utils as U
    imgs, labs = _squares()
    train = U.SegmentationGenerator(imgs[:16], labs[:16], n_classes=2, batch_size=8, seed=1, shuffle=False)
    valid = U.SegmentationGenerator(imgs[16:], labs[16:], n_classes=2, batch_size=4, seed=1, shuffle=False)
    return train, valid


def test_fit_generator_with_validation_and_callbacks(tmp_path):
    from dl3_amd import callbacks as CB
    E = 5
    path = str(tmp_path / "best_{epoch:02d}.h5")
    results = {}
    for feed in (False, True):
        model = _loop_model()
        train, valid = _gens()
        seen = []
        cbs = [CB.ModelCheckpoint(path if not feed else str(tmp_path / "feed_{epoch:02d}.h5"), save_best_only=True,
                                  save_weights_only=True, monitor="val_Jaccard", mode="max"),
               CB.ReduceLROnPlateau(monitor="val_loss", patience=0, factor=0.5, min_delta=1e9),   # halves every epoch
               CB.EarlyStopping(monitor="val_Jaccard", patience=100, mode="max"),
               CB.LambdaCallback(on_batch_end=lambda b, logs: seen.append(logs["loss"]))]
        h = model.fit_generator(train, epochs=E, validation_data=valid, callbacks=cbs, device_feed=feed, n_classes=2)
        assert isinstance(h, CB.History)
        assert set(h.history) == {"loss", "val_loss", "val_Jaccard", "val_sparse_accuracy_ignoring_last_label", "lr"}
        assert all(len(v) == E for v in h.history.values()) and h.epoch == list(range(E))
        results[feed] = (h.history, [float(l) for l in seen])
        if feed:
            continue
        # the last val_* entries are what evaluate_generator says afterwards
        after = model.evaluate_generator(valid)
        assert [h.history[k][-1] for k in ("val_loss", "val_Jaccard", "val_sparse_accuracy_ignoring_last_label")] == after
        # the checkpoint of the best epoch loads into a fresh model that reproduces its val_Jaccard
        best = int(np.argmax(h.history["val_Jaccard"]))   # first maximum: later epochs must be strictly greater to save
        fresh = _loop_model()
        fresh.load_weights(path.format(epoch=best + 1))
        assert fresh.evaluate_generator(valid)[1] == h.history["val_Jaccard"][best]
        # the training losses, bit for bit, from a hand-written loop that changes lr where the History says so
        hand = _loop_model()
        train2, _ = _gens()
        losses = []
        for ep in range(E):
            hand._set_lr(h.history["lr"][ep])   # the rate the History reports for this epoch; nothing else changes
            for i in range(len(train2)):
                X, Y, SW = train2[i]
                losses.append(float(hand.train_on_batch(X, Y, SW["pred_mask"])))
            train2.on_epoch_end()
        assert losses == results[False][1]
    assert results[True][0] == results[False][0] and results[True][1] == results[False][1]
    # min_delta = 1e9: only the first epoch "improves" (on +inf); patience 0 then halves after every later epoch
    assert results[False][0]["lr"] == [3e-3, 3e-3, 1.5e-3, 7.5e-4, 3.75e-4]


def test_early_stopping_ends_the_run_and_plain_fit_is_unchanged():
    from dl3_amd import callbacks as CB
    model = _loop_model()
    train, valid = _gens()
    # val_loss can never beat the baseline of 0: epoch 0 -> wait 1, epoch 1 -> wait 2 = patience -> stop after 2 epochs
    h = model.fit_generator(train, epochs=6, validation_data=valid,
                            callbacks=[CB.EarlyStopping(monitor="val_loss", patience=2, baseline=0.0)])
    assert len(h.history["loss"]) == 2 and model.stop_training
    h = model.fit_generator(train, epochs=6, validation_data=valid,
                            callbacks=[CB.EarlyStopping(monitor="val_loss", patience=1, baseline=0.0)])
    assert len(h.history["loss"]) == 1
    # without the new keywords: the plain list, equal to the same steps driven by hand
    a, b = _loop_model(), _loop_model()
    ta, _ = _gens()
    tb, _ = _gens()
    plain = a.fit_generator(ta, epochs=2)
    assert isinstance(plain, list) and len(plain) == 4
    hand = []
    for ep in range(2):
        for i in range(len(tb)):
            X, Y, SW = tb[i]
            hand.append(float(b.train_on_batch(X, Y, SW["pred_mask"])))
        tb.on_epoch_end()
    assert plain == hand
    # a metric this package does not know: ValueError when validation starts
    c = _loop_model()
    c.compile(optimizer=dict(lr=3e-3), metrics=["mse"])
    tc, vc = _gens()
    with pytest.raises(ValueError, match="mse"):
        c.fit_generator(tc, epochs=1, validation_data=vc)
    # fit() on arrays with validation_data=(x, y, sw)
    X, Y, SW = ta[0]
    Xv, Yv, SWv = valid[0]
    h = _loop_model().fit(X, Y.cpu().numpy(), batch_size=4, epochs=2, sample_weight=SW["pred_mask"].cpu().numpy(),
                          validation_data=(Xv, Yv.cpu().numpy(), SWv["pred_mask"].cpu().numpy()))
    assert len(h.history["val_loss"]) == 2 and len(h.history["val_Jaccard"]) == 2


def test_segmodel_train_generator_end_to_end(tmp_path):
    """segmentation.ipynb cell 5 at 64x64: create_generators(mode='train' / 'validation') -> train_generator"""
    from dl3_amd import graph as G
    from dl3_amd import utils as U
    from dl3_amd.optimizers import Adam
    G.clear_session()
    imgs, labs = _squares(n=20)
    S = U.SegModel(image_size=(64, 64))
    S.set_batch_size(4)
    S.set_num_epochs(2)
    try:
        model = S.create_seg_model("original", n=2, backbone="mobilenetv2")
        model.compile(optimizer=Adam(lr=7e-4, epsilon=1e-8, decay=1e-6),
                      loss=U.sparse_crossentropy_ignoring_last_label, sample_weight_mode="temporal",
                      metrics={"pred_mask": [U.Jaccard, U.sparse_accuracy_ignoring_last_label]})
        tg = S.create_generators(mode="train", n_classes=2, do_ahisteq=False, images=imgs, labels=labs)
        vg = S.create_generators(mode="validation", n_classes=2, do_ahisteq=False, horizontal_flip=False, brightness=0.0,
                                 rotation=0.0, zoom=0.0, images=imgs, labels=labs)
        path = str(tmp_path / "w.h5")
        cbs = [U.ModelCheckpoint(path, save_best_only=True, save_weights_only=True, monitor="val_Jaccard", mode="max"),
               U.ReduceLROnPlateau(monitor="val_Jaccard", factor=0.5, patience=5, min_lr=1e-6),
               U.EarlyStopping(monitor="val_Jaccard", patience=100, mode="max")]
        h = S.train_generator(model, tg, vg, cbs, mp=True)
    finally:
        U.SegModel.set_batch_size(16)
        U.SegModel.set_num_epochs(20)
    assert len(h.history["val_Jaccard"]) == 2 and np.isfinite(h.history["loss"]).all()
    import os
    assert os.path.exists(path)
