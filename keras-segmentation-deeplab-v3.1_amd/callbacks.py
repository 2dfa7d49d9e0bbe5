"""The callbacks the reference's training call uses (segmentation.ipynb cell 5; `from utils import *` provides them
through `from keras.callbacks import *`): Callback, History, LambdaCallback, ModelCheckpoint, EarlyStopping,
ReduceLROnPlateau, LearningRateScheduler — Keras 2.2.4 constructor signatures, defaults and decision rules [TF-semantics, restated from
memory of keras/callbacks.py 2.2.4; the package is not installed].  Pure host-side control plane: nothing here touches
the device except through the model's own methods (save_weights, get_weights / set_weights, the learning rate).

What differs from Keras, on purpose:
  * `on_batch_end` logs carry the loss as an engine.LazyLoss — float(logs['loss']) reads it (one device read); a
    callback that ignores it costs nothing.
  * ModelCheckpoint(save_weights_only=False) raises at construction: this package stores weights only.
  * The learning rate is read / written through `model._get_lr()` / `model._set_lr(v)`: the compiled hyper-parameter
    dict and the optimizer object's `lr`; the change takes effect at the next step, without a new engine.
  * TensorBoard is not built.
  * poly_decay(base_lr, max_epochs, power) is not in Keras: the "poly" schedule DeepLab is trained with, as a function
    LearningRateScheduler takes.
"""
import warnings

import numpy as np


class Callback:
    def __init__(self):
        self.validation_data = None
        self.model = None
        self.params = {}

    def set_params(self, params):
        self.params = params

    def set_model(self, model):
        self.model = model

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_batch_begin(self, batch, logs=None):
        pass

    def on_batch_end(self, batch, logs=None):
        pass

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass


class CallbackList:
    """the container Model.fit drives (keras.callbacks.CallbackList without the timing statistics)"""

    def __init__(self, callbacks=None):
        self.callbacks = list(callbacks or [])

    def append(self, cb):
        self.callbacks.append(cb)

    def set_params(self, params):
        for cb in self.callbacks:
            cb.set_params(params)

    def set_model(self, model):
        for cb in self.callbacks:
            cb.set_model(model)

    def _call(self, hook, *args):
        for cb in self.callbacks:
            getattr(cb, hook)(*args)

    def on_epoch_begin(self, epoch, logs=None):
        self._call("on_epoch_begin", epoch, logs if logs is not None else {})

    def on_epoch_end(self, epoch, logs=None):
        self._call("on_epoch_end", epoch, logs if logs is not None else {})

    def on_batch_begin(self, batch, logs=None):
        self._call("on_batch_begin", batch, logs if logs is not None else {})

    def on_batch_end(self, batch, logs=None):
        self._call("on_batch_end", batch, logs if logs is not None else {})

    def on_train_begin(self, logs=None):
        self._call("on_train_begin", logs if logs is not None else {})

    def on_train_end(self, logs=None):
        self._call("on_train_end", logs if logs is not None else {})

    def __iter__(self):
        return iter(self.callbacks)


class History(Callback):
    """what fit / fit_generator return when callbacks= or validation_data= is given: .epoch and .history[name] lists"""

    def on_train_begin(self, logs=None):
        self.epoch = []
        self.history = {}

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


class LambdaCallback(Callback):
    def __init__(self, on_epoch_begin=None, on_epoch_end=None, on_batch_begin=None, on_batch_end=None,
                 on_train_begin=None, on_train_end=None, **kwargs):
        super().__init__()
        self.__dict__.update(kwargs)
        noop2, noop1 = (lambda a, logs: None), (lambda logs: None)
        self.on_epoch_begin = on_epoch_begin if on_epoch_begin is not None else noop2
        self.on_epoch_end = on_epoch_end if on_epoch_end is not None else noop2
        self.on_batch_begin = on_batch_begin if on_batch_begin is not None else noop2
        self.on_batch_end = on_batch_end if on_batch_end is not None else noop2
        self.on_train_begin = on_train_begin if on_train_begin is not None else noop1
        self.on_train_end = on_train_end if on_train_end is not None else noop1


def _resolve_mode(mode, monitor, who):
    """'min' / 'max' as Keras 2.2.4 resolves it: 'auto' -> max if 'acc' in monitor or it starts with 'fmeasure', else min"""
    if mode not in ("auto", "min", "max"):
        warnings.warn("%s mode %s is unknown, fallback to auto mode." % (who, mode), RuntimeWarning)
        mode = "auto"
    if mode == "auto":
        mode = "max" if ("acc" in monitor or monitor.startswith("fmeasure")) else "min"
    return mode


class ModelCheckpoint(Callback):
    """keras.callbacks.ModelCheckpoint: `filepath.format(epoch=epoch + 1, **logs)`, every `period` epochs, with
    save_best_only only when the monitored quantity improved.  Under Model.distribute() only rank 0 writes."""

    def __init__(self, filepath, monitor="val_loss", verbose=0, save_best_only=False, save_weights_only=False,
                 mode="auto", period=1):
        super().__init__()
        if not save_weights_only:
            raise ValueError("ModelCheckpoint(save_weights_only=False): this package stores weights only "
                             "(Model.save_weights); pass save_weights_only=True as the reference's notebook does")
        self.monitor, self.verbose, self.filepath = monitor, verbose, filepath
        self.save_best_only, self.save_weights_only, self.period = save_best_only, save_weights_only, period
        self.epochs_since_last_save = 0
        self.mode = _resolve_mode(mode, monitor, "ModelCheckpoint")
        if self.mode == "min":
            self.monitor_op, self.best = np.less, np.inf
        else:
            self.monitor_op, self.best = np.greater, -np.inf

    def _writes(self):
        dp = getattr(self.model, "_dp", None)
        return dp is None or getattr(dp, "rank", 0) == 0

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        self.epochs_since_last_save += 1
        if self.epochs_since_last_save < self.period:
            return
        self.epochs_since_last_save = 0
        filepath = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = logs.get(self.monitor)
            if current is None:
                warnings.warn("Can save best model only with %s available, skipping." % self.monitor, RuntimeWarning)
                return
            if not self.monitor_op(current, self.best):
                if self.verbose > 0:
                    print("\nEpoch %05d: %s did not improve from %0.5f" % (epoch + 1, self.monitor, self.best))
                return
            if self.verbose > 0:
                print("\nEpoch %05d: %s improved from %0.5f to %0.5f, saving model to %s"
                      % (epoch + 1, self.monitor, self.best, current, filepath))
            self.best = current
        elif self.verbose > 0:
            print("\nEpoch %05d: saving model to %s" % (epoch + 1, filepath))
        if self._writes():
            self.model.save_weights(filepath)


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping (2.2.4): stop when `monitor` has not improved by more than min_delta for more than
    `patience` epochs; `baseline`: the value to beat from the start; restore_best_weights: put the best epoch's weights
    back when stopping."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, verbose=0, mode="auto", baseline=None,
                 restore_best_weights=False):
        super().__init__()
        self.monitor, self.baseline, self.patience, self.verbose = monitor, baseline, patience, verbose
        self.min_delta = abs(min_delta)
        self.wait = 0
        self.stopped_epoch = 0
        self.restore_best_weights = restore_best_weights
        self.best_weights = None
        self.mode = _resolve_mode(mode, monitor, "EarlyStopping")
        self.monitor_op = np.less if self.mode == "min" else np.greater
        if self.mode == "min":
            self.min_delta *= -1

    def on_train_begin(self, logs=None):
        self.wait = 0
        self.stopped_epoch = 0
        if self.baseline is not None:
            self.best = self.baseline
        else:
            self.best = np.inf if self.monitor_op == np.less else -np.inf

    def on_epoch_end(self, epoch, logs=None):
        current = (logs or {}).get(self.monitor)
        if current is None:
            warnings.warn("Early stopping conditioned on metric `%s` which is not available. Available metrics are: %s"
                          % (self.monitor, ",".join(list((logs or {}).keys()))), RuntimeWarning)
            return
        if self.monitor_op(current - self.min_delta, self.best):
            self.best = current
            self.wait = 0
            if self.restore_best_weights:
                self.best_weights = self.model.get_weights()
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                self.model.stop_training = True
                if self.restore_best_weights and self.best_weights is not None:
                    if self.verbose > 0:
                        print("Restoring model weights from the end of the best epoch")
                    self.model.set_weights(self.best_weights)

    def on_train_end(self, logs=None):
        if self.stopped_epoch > 0 and self.verbose > 0:
            print("Epoch %05d: early stopping" % (self.stopped_epoch + 1))


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau (2.2.4): lr <- max(lr * factor, min_lr) when `monitor` has not improved by
    more than min_delta for `patience` epochs; `cooldown` epochs after a reduction during which `wait` is held at 0;
    adds logs['lr']."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, verbose=0, mode="auto", min_delta=1e-4, cooldown=0,
                 min_lr=0, **kwargs):
        super().__init__()
        self.monitor = monitor
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0.")
        if "epsilon" in kwargs:
            min_delta = kwargs.pop("epsilon")
            warnings.warn("`epsilon` argument is deprecated and will be removed, use `min_delta` instead.")
        self.factor, self.min_lr, self.min_delta, self.patience = factor, min_lr, min_delta, patience
        self.verbose, self.cooldown = verbose, cooldown
        self.cooldown_counter = 0
        self.wait = 0
        self.best = 0
        self.mode = mode
        self.monitor_op = None
        self._reset()

    def _reset(self):
        if self.mode not in ("auto", "min", "max"):
            warnings.warn("Learning Rate Plateau Reducing mode %s is unknown, fallback to auto mode." % self.mode,
                          RuntimeWarning)
            self.mode = "auto"
        if self.mode == "min" or (self.mode == "auto" and "acc" not in self.monitor):
            self.monitor_op = lambda a, b: np.less(a, b - self.min_delta)
            self.best = np.inf
        else:
            self.monitor_op = lambda a, b: np.greater(a, b + self.min_delta)
            self.best = -np.inf
        self.cooldown_counter = 0
        self.wait = 0

    def on_train_begin(self, logs=None):
        self._reset()

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs["lr"] = float(self.model._get_lr())
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn("Reduce LR on plateau conditioned on metric `%s` which is not available. Available metrics "
                          "are: %s" % (self.monitor, ",".join(list(logs.keys()))), RuntimeWarning)
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self.monitor_op(current, self.best):
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old_lr = float(self.model._get_lr())
                if old_lr > self.min_lr:
                    new_lr = max(old_lr * self.factor, self.min_lr)
                    self.model._set_lr(new_lr)
                    if self.verbose > 0:
                        print("\nEpoch %05d: ReduceLROnPlateau reducing learning rate to %s." % (epoch + 1, new_lr))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler (2.2.4): at the start of every epoch the learning rate becomes
    schedule(epoch, lr) — or schedule(epoch), the older one-argument form, when the call with two raises TypeError; the
    result must be a float.  Adds logs['lr'] at the end of the epoch."""

    def __init__(self, schedule, verbose=0):
        super().__init__()
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch, logs=None):
        lr = float(self.model._get_lr())
        try:  # new API
            lr = self.schedule(epoch, lr)
        except TypeError:  # old API for backward compatibility
            lr = self.schedule(epoch)
        if not isinstance(lr, (float, np.float32, np.float64)):
            raise ValueError('The output of the "schedule" function should be float.')
        self.model._set_lr(float(lr))
        if self.verbose > 0:
            print("\nEpoch %05d: LearningRateScheduler setting learning rate to %s." % (epoch + 1, lr))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs["lr"] = float(self.model._get_lr())


def poly_decay(base_lr, max_epochs, power=0.9):
    """the "poly" learning-rate policy of the DeepLab papers, per epoch: schedule(epoch) = base_lr * (1 - epoch /
    max_epochs) ** power (0 from max_epochs on) — for LearningRateScheduler"""
    base_lr, max_epochs, power = float(base_lr), int(max_epochs), float(power)
    if not (max_epochs > 0 and base_lr >= 0 and power > 0):
        raise ValueError("poly_decay: max_epochs, power must be > 0 and base_lr >= 0")

    def schedule(epoch, lr=None):
        return base_lr * max(1.0 - float(epoch) / max_epochs, 0.0) ** power
    return schedule
