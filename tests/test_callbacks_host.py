"""CPU: the callbacks' decision rules (Keras 2.2.4 semantics) against scripted log sequences with hand-computed
outcomes, calculate_iou's layout against the notebook's loop, and known-answer cases of the evaluation-tail oracle."""
import warnings

import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import callbacks as CB
from tests import eval_oracle as EO


class FakeModel:
    """records what the callbacks do to a model"""

    def __init__(self, lr=1.0):
        self.lr, self.saved, self.weights, self.stop_training, self.set_calls = lr, [], [0], False, []

    def _get_lr(self):
        return self.lr

    def _set_lr(self, v):
        self.lr = float(v)

    def save_weights(self, path):
        self.saved.append(path)

    def get_weights(self):
        return list(self.weights)

    def set_weights(self, w):
        self.set_calls.append(list(w))
        self.weights = list(w)


def _drive(cb, seq, key="val_loss", model=None):
    """run a callback over scripted per-epoch values; -> (model, list of per-epoch logs)"""
    model = model or FakeModel()
    cb.set_model(model)
    cb.on_train_begin()
    out = []
    for ep, v in enumerate(seq):
        logs = {} if v is None else {key: v}
        model.weights = [ep]
        cb.on_epoch_end(ep, logs)
        out.append(logs)
        if model.stop_training:
            break
    cb.on_train_end()
    return model, out


def test_reduce_lr_patience_cooldown_min_lr():
    # min mode, min_delta 0.1: an epoch improves only below best - 0.1
    # ep: 0 (1.0 best) | 1 (0.95: no, wait 1) | 2 (0.95: wait 2 = patience -> lr 0.5, cooldown 2, wait 0)
    #     3 (cooldown 2->1, wait 0; no improvement; in cooldown: nothing) | 4 (cooldown 1->0; not in cooldown: wait 1)
    #     5 (wait 2 -> lr 0.25 -> min_lr clamps to 0.3) | 6 (cooldown 2->1) | 7 (cooldown 1->0, wait 1)
    #     8 (wait 2: old lr 0.3 is not above min_lr: no change)
    cb = CB.ReduceLROnPlateau(monitor="val_loss", factor=0.5, patience=2, min_delta=0.1, cooldown=2, min_lr=0.3)
    model, logs = _drive(cb, [1.0, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95])
    assert [l["lr"] for l in logs] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.3, 0.3, 0.3]   # logs carry the rate BEFORE the change
    assert model.lr == 0.3
    # an improvement resets the wait
    cb = CB.ReduceLROnPlateau(monitor="val_loss", factor=0.5, patience=2, min_delta=0.0)
    model, _ = _drive(cb, [1.0, 1.0, 0.9, 0.9, 0.8, 0.8, 0.8])
    assert model.lr == 0.5   # only the last two stagnant epochs in a row reach patience
    # max mode
    cb = CB.ReduceLROnPlateau(monitor="val_Jaccard", factor=0.1, patience=1, mode="max", min_delta=0.0)
    model, _ = _drive(cb, [0.5, 0.6, 0.6, 0.7], key="val_Jaccard")
    assert model.lr == pytest.approx(0.1)
    with pytest.raises(ValueError):
        CB.ReduceLROnPlateau(factor=1.0)


def test_early_stopping_min_delta_baseline_restore():
    # min mode, min_delta 0.1, patience 2: 1.0 best | 0.95 wait 1 | 0.85 best (0.85 + 0.1 < 1.0) | 0.8 wait 1 | 0.8 wait 2: stop
    cb = CB.EarlyStopping(monitor="val_loss", min_delta=0.1, patience=2, restore_best_weights=True)
    model, logs = _drive(cb, [1.0, 0.95, 0.85, 0.8, 0.8, 0.1, 0.1])
    assert cb.stopped_epoch == 4 and len(logs) == 5 and model.stop_training
    assert model.set_calls == [[2]] and model.weights == [2]    # the weights of the best epoch (2) are put back
    # baseline: nothing beats 0.5 -> stops after `patience` epochs
    cb = CB.EarlyStopping(monitor="val_loss", patience=3, baseline=0.5)
    model, logs = _drive(cb, [0.9, 0.8, 0.7, 0.6, 0.4])
    assert cb.stopped_epoch == 2 and len(logs) == 3
    # max mode never stops while it improves
    cb = CB.EarlyStopping(monitor="val_Jaccard", patience=1, mode="max")
    model, logs = _drive(cb, [0.1, 0.2, 0.3, 0.4], key="val_Jaccard")
    assert not model.stop_training and len(logs) == 4


def test_model_checkpoint_best_only_period_and_names():
    # max mode, period 2: looked at after epochs 1, 3, 5, 7 (0-based) -> values 0.2 (best), 0.1 (no), 0.5 (best), 0.5 (no)
    cb = CB.ModelCheckpoint("w.{epoch:02d}-{val_Jaccard:.2f}.h5", monitor="val_Jaccard", save_best_only=True,
                            save_weights_only=True, mode="max", period=2)
    model, _ = _drive(cb, [0.9, 0.2, 0.9, 0.1, 0.0, 0.5, 0.9, 0.5], key="val_Jaccard")
    assert model.saved == ["w.02-0.20.h5", "w.06-0.50.h5"]
    cb = CB.ModelCheckpoint("e{epoch}.h5", save_weights_only=True)   # every epoch, whatever the logs
    model, _ = _drive(cb, [3.0, 2.0, 4.0])
    assert model.saved == ["e1.h5", "e2.h5", "e3.h5"]
    with pytest.raises(ValueError):
        CB.ModelCheckpoint("x.h5")   # save_weights_only=False: whole-model files are not built

    class Rank1(FakeModel):
        class _dp:
            rank, world = 1, 2
    model, _ = _drive(CB.ModelCheckpoint("e{epoch}.h5", save_weights_only=True), [1.0], model=Rank1())
    assert model.saved == []   # under distribute() only rank 0 writes


def test_auto_mode_and_missing_monitor():
    assert CB.ModelCheckpoint("x", monitor="val_acc", save_weights_only=True).mode == "max"
    assert CB.ModelCheckpoint("x", monitor="fmeasure", save_weights_only=True).mode == "max"
    assert CB.ModelCheckpoint("x", monitor="val_iou", save_weights_only=True).mode == "min"   # a score without 'acc' in its name needs mode='max'
    assert CB.ModelCheckpoint("x", monitor="val_Jaccard", save_weights_only=True).mode == "max"   # 'J-acc-ard' contains 'acc'
    assert CB.ModelCheckpoint("x", monitor="val_sparse_accuracy_ignoring_last_label", save_weights_only=True).mode == "max"
    assert CB.EarlyStopping(monitor="val_loss").mode == "min"
    for cb in (CB.EarlyStopping(monitor="val_nope"), CB.ReduceLROnPlateau(monitor="val_nope"),
               CB.ModelCheckpoint("x", monitor="val_nope", save_best_only=True, save_weights_only=True)):
        with pytest.warns(RuntimeWarning, match="val_nope"):
            model, _ = _drive(cb, [1.0, 2.0])
        assert not model.stop_training and model.saved == [] and model.lr == 1.0
    with pytest.warns(RuntimeWarning):
        assert CB.EarlyStopping(mode="sideways").mode == "min"


def test_history_and_lambda_and_list_order():
    order = []
    h = CB.History()
    lam = CB.LambdaCallback(on_epoch_end=lambda ep, logs: logs.setdefault("extra", ep * 10),
                            on_batch_end=lambda b, logs: order.append(("batch", b)),
                            on_train_begin=lambda logs: order.append("begin"), on_train_end=lambda logs: order.append("end"))
    lst = CB.CallbackList([lam, h])
    lst.set_model(FakeModel())
    lst.on_train_begin()
    for ep in range(3):
        lst.on_epoch_begin(ep)
        lst.on_batch_end(0, {"loss": object()})   # never converted: a lazy loss costs nothing here
        lst.on_epoch_end(ep, {"loss": 1.0 / (ep + 1)})
    lst.on_train_end()
    assert h.epoch == [0, 1, 2] and h.history == {"loss": [1.0, 0.5, 1.0 / 3], "extra": [0, 10, 20]}
    assert order == ["begin", ("batch", 0), ("batch", 0), ("batch", 0), "end"]


def test_utils_reexports_the_callbacks():
    from dl3_amd import utils as U
    for name in ("Callback", "History", "LambdaCallback", "ModelCheckpoint", "EarlyStopping", "ReduceLROnPlateau"):
        assert getattr(U, name) is getattr(CB, name)
    assert callable(U.SegModel.train_generator) and not hasattr(U.SegModel, "train")


def test_calculate_iou_layout_is_the_notebooks():
    from dl3_amd import utils as U
    rng = np.random.default_rng(5)
    nb, n, H, W = 5, 3, 6, 7
    label = rng.integers(0, nb, (n, H, W))
    label[rng.random((n, H, W)) < 0.2] = 255
    pred = rng.integers(0, nb, (n, H, W))

    class Fake:
        def confusion_matrix(self, X, y, batch_size=32):
            return EO.confusion(pred, y.reshape(n, H, W), nb)
    got = U.calculate_iou(Fake(), np.zeros((n, H, W, 3)), label, nb_classes=nb)
    conf_m = np.zeros((nb, nb), dtype=float)     # segmentation.ipynb cell 10, written out
    for i in range(n):
        flat_pred, flat_label = np.ravel(pred[i]), np.ravel(label[i])
        for p, l in zip(flat_pred, flat_label):
            if l < 255:
                conf_m[l - 1, p - 1] += 1
    assert got.dtype == np.float64 and np.array_equal(got, conf_m)
    assert got[-1, -1] == ((label == 0) & (pred == 0)).sum()   # class 0 sits in the last row / column


# ------------------------------------------------------------------------------------------------ oracle known answers
def test_oracle_constant_logits():
    C, N, Hi = 4, 2, 4
    x = np.zeros((N, Hi, Hi, C), np.float32)
    labels = np.full((N, 16, 16), 2.0, np.float32)
    r = EO.eval_tail("bilinear", x, (16, 16), labels)
    assert np.allclose(r["loss_sum"], 256 * np.log(C), rtol=1e-12)
    assert np.array_equal(r["mask"], np.zeros((N, 16, 16), np.int32))    # first maximum wins
    assert np.array_equal(r["nnz"], [256, 256])
    assert np.array_equal(r["counts"][0], [[0, 0, 256, 0], [256, 0, 0, 0], [0, 0, 0, 0]])
    assert r["confusion"][2, 0] == 512 and r["confusion"].sum() == 512


def test_oracle_one_hot_image_and_clip():
    C = 3
    t = np.arange(8 * 8).reshape(1, 8, 8) % C
    x = np.where(np.arange(C)[None, None, None] == t[..., None], 40.0, 0.0).astype(np.float32)   # p_true ~ 1: clipped
    r = EO.eval_tail("plain", x, None, t.astype(np.float32))
    assert np.array_equal(r["mask"], t)
    assert np.allclose(r["loss_sum"], 64 * -np.log(1 - 1e-7), rtol=1e-9)
    assert np.array_equal(r["confusion"], np.diag(np.bincount(t.ravel(), minlength=C)))
    wrong = EO.eval_tail("plain", x, None, ((t + 1) % C).astype(np.float32))
    assert np.allclose(wrong["loss_sum"], 64 * -np.log(1e-7), rtol=1e-9) and np.trace(wrong["confusion"]) == 0
    # shuffle: the phase shift is a permutation of the same pixels
    u = np.random.default_rng(0).standard_normal((1, 2, 2, C * 16)).astype(np.float32)
    s = EO.eval_tail("shuffle", u, 4, np.zeros((1, 8, 8), np.float32))
    from oracle import dl3_oracle as O
    assert np.array_equal(s["mask"], O.phase_shift(u, 4).argmax(-1))


def test_oracle_all_void_and_all_zero_weights():
    rng = np.random.default_rng(1)
    C = 5
    x = rng.standard_normal((2, 4, 4, C)).astype(np.float32)
    void = EO.eval_tail("bilinear", x, (8, 8), np.full((2, 8, 8), float(C), np.float32))
    assert np.array_equal(void["loss_sum"], [0, 0]) and void["confusion"].sum() == 0
    assert void["counts"][:, 0].sum() == 0 and void["counts"][:, 1].sum() == 128 and np.array_equal(void["nnz"], [64, 64])
    labels = rng.integers(0, C, (2, 8, 8)).astype(np.float32)
    zero = EO.eval_tail("bilinear", x, (8, 8), labels, np.zeros((2, 8, 8), np.float32))
    assert np.array_equal(zero["loss_sum"], [0, 0]) and np.array_equal(zero["nnz"], [0, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no division by the zero count
        assert EO.batch_metrics(zero["loss_sum"], zero["nnz"], zero["counts"])[0] == 0.0
    for dt in (np.float32, np.float64):
        assert EO.eval_tail("bilinear", x, (8, 8), labels, dtype=dt)["loss_sum"].dtype == dt


def test_oracle_batch_weighted_average_with_a_ragged_batch():
    per = [[1.0, 0.5, 0.8], [2.0, 0.7, 0.6], [4.0, 0.1, 1.0]]
    got = EO.weighted_average(per, [2, 2, 1])
    assert got == pytest.approx([(2 + 4 + 4) / 5, (1.0 + 1.4 + 0.1) / 5, (1.6 + 1.2 + 1.0) / 5])
    assert got != pytest.approx(list(np.mean(per, 0)))   # not the plain mean over batches
