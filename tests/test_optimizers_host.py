"""CPU tests of the optimizer surface: optimizers.SGD / RMSprop / Adam with clipping, what Model.compile stores, the
float64 oracle of the update rules (tests/optim_oracle.py) on hand-computed steps, LearningRateScheduler and poly_decay.
No device code runs here."""
import ctypes
import re

import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi, graph as G
from dl3_amd.callbacks import LearningRateScheduler, poly_decay
from dl3_amd.optimizers import SGD, Adam, RMSprop, compile_optimizer
from tests import optim_oracle as PO


@pytest.fixture(scope="module")
def model():
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone="mobilenetv2")


# ------------------------------------------------------------------------------------------------------ the classes
def test_keras_defaults_and_config_round_trips():
    assert SGD().get_config() == dict(lr=0.01, momentum=0.0, decay=0.0, nesterov=False)
    assert RMSprop().get_config() == dict(lr=0.001, rho=0.9, epsilon=1e-7, decay=0.0)
    assert Adam().get_config() == dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0, amsgrad=False)
    for o in (SGD(lr=0.007, momentum=0.9, decay=1e-4, nesterov=True, clipnorm=2.0),
              RMSprop(lr=3e-4, rho=0.95, epsilon=1e-6, decay=1e-3, clipvalue=0.5),
              Adam(lr=7e-4, epsilon=1e-8, decay=1e-6, clipnorm=1.0, clipvalue=0.25)):
        back = type(o).from_config(o.get_config())
        assert type(back) is type(o) and back.get_config() == o.get_config()
        assert type(o).__name__ + "(" in repr(o) and "lr=" in repr(o)
    # clipnorm / clipvalue appear only when set
    assert "clipnorm" not in SGD().get_config() and "clipvalue" not in RMSprop().get_config()
    assert SGD(clipnorm=2).get_config()["clipnorm"] == 2.0 and "clipvalue" not in SGD(clipnorm=2).get_config()
    assert Adam(clipvalue=0.5).get_config()["clipvalue"] == 0.5
    # the tf.keras spelling
    assert SGD(learning_rate=0.3).lr == 0.3 and RMSprop(learning_rate=0.2).lr == 0.2 and Adam(learning_rate=0.1).lr == 0.1


@pytest.mark.parametrize("make", [
    lambda: SGD(lr=-1), lambda: SGD(momentum=-0.1), lambda: SGD(decay=-1), lambda: RMSprop(lr=-1),
    lambda: RMSprop(rho=1.5), lambda: RMSprop(decay=-1), lambda: RMSprop(epsilon=-1), lambda: Adam(beta_1=1.0),
    lambda: SGD(clipnorm=0), lambda: SGD(clipnorm=-1), lambda: RMSprop(clipvalue=0), lambda: Adam(clipvalue=-2.0),
    lambda: Adam(amsgrad=True), lambda: Adam(amsgrad=True, clipnorm=1.0)])
def test_bad_arguments_raise_value_error(make):
    with pytest.raises(ValueError):
        make()


@pytest.mark.parametrize("cls", [SGD, RMSprop, Adam])
def test_unknown_keyword_raises_type_error(cls):
    with pytest.raises(TypeError):
        cls(momentun=0.9)


# ------------------------------------------------------------------------------------------------------ compile
def test_compile_stores_rule_and_clip_settings_beside_the_hyper_parameters(model):
    s = SGD(lr=0.007, momentum=0.9, decay=1e-4, nesterov=True, clipnorm=2.0)
    model.compile(optimizer=s)
    c = model._compiled
    assert c["rule"] == "sgd" and c["clipnorm"] == 2.0 and c["clipvalue"] is None and c["optimizer_object"] is s
    assert c["optimizer"] == dict(lr=0.007, momentum=0.9, decay=1e-4, nesterov=True)
    assert model._opt_desc() == dict(rule="sgd", hyper=c["optimizer"], clipnorm=2.0, clipvalue=None)
    assert model._opt_desc()["hyper"] is c["optimizer"]      # _set_lr on the compiled dict reaches the next step
    model.compile(optimizer=RMSprop(rho=0.95, clipvalue=0.5))
    c = model._compiled
    assert c["rule"] == "rmsprop" and c["clipnorm"] is None and c["clipvalue"] == 0.5
    assert c["optimizer"] == dict(lr=0.001, rho=0.95, epsilon=1e-7, decay=0.0)
    a = Adam(lr=7e-4, epsilon=1e-8, decay=1e-6, clipnorm=1.0)
    model.compile(optimizer=a)
    c = model._compiled
    assert c["rule"] == "adam" and c["clipnorm"] == 1.0 and c["clipvalue"] is None
    assert c["optimizer"] == dict(lr=7e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=1e-6)   # the five keys, as ever
    for opt in (None, "adam", dict(lr=1e-3), Adam()):
        model.compile(optimizer=opt)
        assert model._compiled["rule"] == "adam" and model._compiled["clipnorm"] is None
        assert model._compiled["clipvalue"] is None


def test_new_rules_are_taken_as_instances_of_this_package_only(model):
    class SGDLike:      # Keras-shaped, not ours
        def get_config(self):
            return dict(lr=0.1, momentum=0.9, decay=0.0, nesterov=False)

    class AdamW2:  # Adam-shaped and accepted — but not with clipping it would silently lose
        def __init__(self, **extra):
            self.extra = extra

        def get_config(self):
            return dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0, amsgrad=False, **self.extra)
    for bad in ("sgd", "rmsprop", "SGD", SGDLike(), AdamW2(clipnorm=1.0), dict(momentum=0.9)):
        with pytest.raises((TypeError, ValueError)):
            model.compile(optimizer=bad)
    assert compile_optimizer(AdamW2())[:1] == ("adam",) and compile_optimizer(AdamW2())[1]["lr"] == 0.002


def test_get_lr_and_set_lr_work_for_every_rule(model):
    for opt, lr in ((SGD(), 0.01), (RMSprop(), 0.001), (Adam(), 0.001), (SGD(lr=0.5), 0.5), (None, 7e-4),
                    (dict(decay=0.1), 7e-4)):
        model.compile(optimizer=opt)
        assert model._get_lr() == lr
        model._set_lr(0.125)
        assert model._get_lr() == 0.125 and model._opt_desc()["hyper"]["lr"] == 0.125
        if opt is not None and not isinstance(opt, dict):
            assert opt.lr == 0.125
    model._compiled = None
    assert model._get_lr() == 7e-4 and model._opt_desc() == dict(rule="adam", hyper={})   # nothing compiled: unchanged


def test_opt_hyper_mirrors_the_header_struct():
    """capi.OptHyper is handed to dl3_opt_step by address: field order and types as in include/dl3.h"""
    src = open(capi.HEADER).read()
    body = re.search(r"typedef struct \{(.*?)\} dl3_opt_hyper;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, want[t]) for n, t in fields] == list(capi.OptHyper._fields_)
    assert ctypes.sizeof(capi.OptHyper) == 4 * len(fields)
    protos = capi.parse_header()
    assert [a for _, a in protos["dl3_opt_step"][1]] == ["p", "g", "s0", "s1", "n", "rule", "hyper", "denom", "sumsq", "stream"]
    assert [a for _, a in protos["dl3_grad_sumsq"][1]] == ["g", "n", "out", "workspace", "workspace_bytes", "stream"]
    assert protos["dl3_grad_sumsq_workspace_bytes"] == ("size_t", [("size_t", "n")])
    assert capi.lib().dl3_grad_sumsq_workspace_bytes(1) >= 8


# ------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_sgd_two_steps_momentum_and_decay():
    """`it` is the count BEFORE the increment: the first step runs at lr, the second at lr / (1 + decay)"""
    p, g = np.array([1.0, -2.0]), np.array([0.5, 4.0])
    p1, m1, _ = PO.keras_step("sgd", p, g, np.zeros(2), None, 0, lr=0.1, momentum=0.9, decay=0.5)
    np.testing.assert_allclose(m1, [-0.05, -0.4], rtol=1e-15)            # v = -lr g
    np.testing.assert_allclose(p1, [0.95, -2.4], rtol=1e-15)
    p2, m2, _ = PO.keras_step("sgd", p1, g, m1, None, 1, lr=0.1, momentum=0.9, decay=0.5)
    lr1 = 0.1 / 1.5
    np.testing.assert_allclose(m2, [0.9 * -0.05 - lr1 * 0.5, 0.9 * -0.4 - lr1 * 4.0], rtol=1e-15)
    np.testing.assert_allclose(m2, [-0.045 - 1.0 / 30, -0.36 - 4.0 / 15], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.95 - 0.045 - 1.0 / 30, -2.4 - 0.36 - 4.0 / 15], rtol=1e-14)
    # the kernel-level form handed the scheduled lr_t gives the same step
    (kp, km), _ = PO.sgd(p1, g, m1, lr1, 0.9)
    np.testing.assert_allclose(kp, p2, rtol=1e-7)
    np.testing.assert_allclose(km, m2, rtol=1e-7)


def test_oracle_sgd_nesterov():
    p, g, m = np.array([1.0]), np.array([2.0]), np.array([-0.5])
    p1, m1, _ = PO.keras_step("sgd", p, g, m, None, 0, lr=0.1, momentum=0.9, nesterov=True)
    v = 0.9 * -0.5 - 0.1 * 2.0                                           # -0.65
    np.testing.assert_allclose(m1, [-0.65], rtol=1e-15)
    np.testing.assert_allclose(p1, [1.0 + 0.9 * v - 0.2], rtol=1e-15)    # 0.215
    np.testing.assert_allclose(p1, [0.215], rtol=1e-12)
    plain, _, _ = PO.keras_step("sgd", p, g, m, None, 0, lr=0.1, momentum=0.9)
    np.testing.assert_allclose(plain, [0.35], rtol=1e-12)


def test_oracle_rmsprop_first_step():
    p, g = np.array([1.0, 1.0]), np.array([3.0, -1e-3])
    p1, a1, _ = PO.keras_step("rmsprop", p, g, np.zeros(2), None, 0, lr=0.01)
    np.testing.assert_allclose(a1, 0.1 * g * g, rtol=1e-12)             # 0.1: 1 - rho evaluated in float64 next to 0.9
    np.testing.assert_allclose(p1, p - 0.01 * g / (np.sqrt(0.1 * g * g) + 1e-7), rtol=1e-12)
    np.testing.assert_allclose(p1[0], 1.0 - 0.01 * 3.0 / (np.sqrt(0.9) + 1e-7), rtol=1e-12)
    # decay on the count before the increment, here too
    p2, _, _ = PO.keras_step("rmsprop", p, g, np.zeros(2), None, 3, lr=0.01, decay=1.0)
    np.testing.assert_allclose(p2 - p, (p1 - p) / 4.0, rtol=1e-12)


def test_oracle_clipnorm_below_equal_and_above_the_threshold():
    g = np.array([3.0, 4.0])                                             # norm 5
    np.testing.assert_array_equal(PO.effective_gradient(g, clipnorm=6.0), g)           # below: untouched
    np.testing.assert_array_equal(PO.effective_gradient(g, clipnorm=5.0), g)           # equal: clips, factor 5/5 = 1
    np.testing.assert_allclose(PO.effective_gradient(g, clipnorm=2.5), [1.5, 2.0], rtol=1e-15)
    # the scale comes first: the norm is that of the SCALED gradient (data-parallel: gs / denom)
    np.testing.assert_allclose(PO.effective_gradient(g, gs=0.5, clipnorm=2.0), [1.2, 1.6], rtol=1e-15)   # norm 2.5 -> 2
    np.testing.assert_allclose(PO.effective_gradient(g, gs=4.0, denom=8.0, clipnorm=3.0), [1.5, 2.0], rtol=1e-15)
    np.testing.assert_allclose(PO.effective_gradient(g, gs=4.0, denom=8.0, clipnorm=2.0), [1.2, 1.6], rtol=1e-15)
    np.testing.assert_array_equal(PO.effective_gradient(np.zeros(3), gs=1.0, denom=0.0, clipnorm=1.0), np.zeros(3))
    # "equal" takes the clipping branch: with norm >= clipnorm it is g * (c / norm), visible where c / norm != 1 exactly
    p1, _, _ = PO.keras_step("sgd", np.zeros(2), g, np.zeros(2), None, 0, lr=1.0, clipnorm=5.0)
    np.testing.assert_array_equal(p1, -g)


def test_oracle_clipvalue_is_applied_after_clipnorm():
    g = np.array([3.0, 4.0, 0.0, -12.0])                                 # norm 13
    ge = PO.effective_gradient(g, clipnorm=6.5, clipvalue=1.75)          # x 0.5 -> [1.5, 2, 0, -6], then the clamp
    np.testing.assert_allclose(ge, [1.5, 1.75, 0.0, -1.75], rtol=1e-15)
    # the other order would clamp first to [1.75, 1.75, 0, -1.75] (norm 3.03 < 6.5) and leave it there
    assert ge[0] == 1.5
    np.testing.assert_allclose(PO.effective_gradient(g, clipvalue=3.5), [3.0, 3.5, 0.0, -3.5], rtol=1e-15)
    p1, m1, v1 = PO.keras_step("adam", np.zeros(4), g, np.zeros(4), np.zeros(4), 0, lr=0.1, epsilon=1e-30, clipnorm=6.5,
                               clipvalue=1.75)
    np.testing.assert_allclose(m1, 0.1 * ge, rtol=1e-12)
    np.testing.assert_allclose(p1, [-0.1, -0.1, 0.0, 0.1], rtol=1e-9, atol=0)    # Adam's first step: lr * sign(g')


# ------------------------------------------------------------------------------------------ LearningRateScheduler
def test_learning_rate_scheduler_both_schedule_forms(model):
    model.compile(optimizer=SGD(lr=0.1, momentum=0.9))
    seen = []

    def two(epoch, lr):
        seen.append((epoch, lr))
        return lr * 0.5
    cb = LearningRateScheduler(two)
    cb.set_model(model)
    cb.on_epoch_begin(0)
    cb.on_epoch_begin(1)
    assert seen == [(0, 0.1), (1, 0.05)] and model._get_lr() == 0.025 and model._compiled["optimizer_object"].lr == 0.025
    logs = {"loss": 1.0}
    cb.on_epoch_end(1, logs)
    assert logs == {"loss": 1.0, "lr": 0.025}
    cb = LearningRateScheduler(lambda epoch: 0.01 * (epoch + 1))         # the one-argument form
    cb.set_model(model)
    cb.on_epoch_begin(2)
    assert model._get_lr() == pytest.approx(0.03, rel=1e-15)
    for rule in (RMSprop(), Adam(), None):
        model.compile(optimizer=rule)
        cb.on_epoch_begin(4)
        assert model._get_lr() == pytest.approx(0.05, rel=1e-15)


@pytest.mark.parametrize("bad", [1, "0.1", None, [0.1]])
def test_learning_rate_scheduler_rejects_a_non_float(model, bad):
    model.compile(optimizer=SGD(lr=0.1))
    cb = LearningRateScheduler(lambda epoch, lr: bad)
    cb.set_model(model)
    with pytest.raises(ValueError):
        cb.on_epoch_begin(0)
    assert model._get_lr() == 0.1
    cb = LearningRateScheduler(lambda epoch, lr: np.float32(0.25))       # numpy floats are floats (Keras 2.2.4)
    cb.set_model(model)
    cb.on_epoch_begin(0)
    assert model._get_lr() == 0.25


def test_poly_decay_values(model):
    s = poly_decay(0.007, 30)
    assert s(0) == 0.007 and s(0, 123.0) == 0.007
    assert s(15) == pytest.approx(0.007 * 0.5 ** 0.9, rel=1e-15)
    assert s(29) == pytest.approx(0.007 * (1.0 / 30) ** 0.9, rel=1e-12)
    assert s(30) == 0.0 and s(31) == 0.0
    assert poly_decay(1.0, 4, power=2.0)(2) == 0.25
    assert all(isinstance(s(e), float) for e in range(31))
    model.compile(optimizer=SGD(lr=0.5))
    cb = LearningRateScheduler(s)
    cb.set_model(model)
    cb.on_epoch_begin(15)
    assert model._get_lr() == pytest.approx(0.007 * 0.5 ** 0.9, rel=1e-15)
    with pytest.raises(ValueError):
        poly_decay(0.1, 0)


def test_utils_star_exports_what_the_references_utils_does():
    ns = {}
    exec("from dl3_amd.utils import *", ns)
    from dl3_amd import callbacks, optimizers
    assert ns["Adam"] is optimizers.Adam and ns["SGD"] is optimizers.SGD and ns["RMSprop"] is optimizers.RMSprop
    assert ns["LearningRateScheduler"] is callbacks.LearningRateScheduler
