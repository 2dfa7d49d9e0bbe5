"""not gpu: the host half of the L2 weight regularisers — the l2 object, the layer keywords,
utils.add_weight_decay, the run-table builder on a dry-lowered engine's slots, the engine key, the header, and the
float64 oracle (tests/l2_oracle.py) against direct numpy sums."""
import math

import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi, graph as G, regularizers as R, utils as U
from dl3_amd.deeplabv3p import Deeplabv3
from dl3_amd.subpixel import Subpixel
from tests import l2_oracle as LO


# ================================================================================================== the l2 object
def test_l2_has_keras_name_default_and_config_round_trip():
    assert U.l2 is R.l2
    r = R.l2()
    assert r.l2 == 0.01 and r.get_config() == {"l1": 0.0, "l2": 0.01}
    q = R.l2.from_config(R.l2(4e-5).get_config())
    assert isinstance(q, R.l2) and q.l2 == 4e-5
    w = np.arange(-3, 4, dtype=np.float32).reshape(7, 1)
    assert R.l2(0.5)(w) == 0.5 * 28.0 and isinstance(R.l2(0.5)(w), float)
    assert R.l2(0.0)(w) == 0.0


@pytest.mark.parametrize("bad", [-1e-9, float("nan"), float("inf"), -float("inf")])
def test_l2_refuses_negative_and_non_finite(bad):
    with pytest.raises(ValueError):
        R.l2(bad)
    with pytest.raises(ValueError):
        R.normal_form({"a/kernel:0": bad})


def test_l2_refuses_what_is_not_a_number_and_l1_configs():
    with pytest.raises(TypeError):
        R.l2("4e-5")
    with pytest.raises(ValueError):
        R.l2.from_config({"l1": 0.1, "l2": 0.0})


# ================================================================================================= layer keywords
def test_layer_keywords_are_stored_and_settable_afterwards():
    G.clear_session()
    a, b = R.l2(1e-4), R.l2(2e-4)
    c = G.Conv2D(8, 1, kernel_regularizer=a, bias_regularizer=b)
    assert c.kernel_regularizer is a and c.bias_regularizer is b
    d = G.DepthwiseConv2D(3, use_bias=False, depthwise_regularizer=a)
    assert d.depthwise_regularizer is a
    n = G.BatchNormalization(gamma_regularizer=a, beta_regularizer=b)
    assert n.gamma_regularizer is a and n.beta_regularizer is b
    s = Subpixel(3, 3, 2, padding="same", kernel_regularizer=a, bias_regularizer=b)
    assert s.kernel_regularizer is a and s.bias_regularizer is b
    plain = G.Conv2D(8, 1)
    assert plain.kernel_regularizer is None and plain.bias_regularizer is None
    plain.kernel_regularizer = b
    assert plain.kernel_regularizer is b
    G.Conv2D(8, 1, activity_regularizer=None, kernel_constraint=None, some_unknown_keyword=3)   # ignored as before
    Subpixel(3, 3, 2, dilation_rate=2, some_unknown_keyword=3)            # Subpixel drops these itself, as before


@pytest.mark.parametrize("foreign", [lambda w: 0.0, "l2", 4e-5, object()])
def test_a_foreign_regulariser_is_a_type_error_at_construction_and_at_compile(foreign):
    G.clear_session()
    for make in (lambda: G.Conv2D(8, 1, kernel_regularizer=foreign), lambda: G.Conv2D(8, 1, bias_regularizer=foreign),
                 lambda: G.DepthwiseConv2D(3, use_bias=False, depthwise_regularizer=foreign),
                 lambda: G.BatchNormalization(gamma_regularizer=foreign),
                 lambda: Subpixel(3, 3, 2, kernel_regularizer=foreign)):
        with pytest.raises(TypeError):
            make()
    m = _model()
    m.compile(optimizer=U.SGD(lr=0.5))
    before = (dict(m._compiled), m._compile_gen, dict(m._collected_trainable))
    m.get_layer("aspp0").kernel_regularizer = foreign   # set afterwards: compile() is the check
    m.get_layer("aspp0").trainable = False
    with pytest.raises(TypeError):
        m.compile(optimizer=U.SGD(lr=0.25))
    # ... and a refused compile() leaves the model as the last good one left it
    assert (dict(m._compiled), m._compile_gen, dict(m._collected_trainable)) == before
    assert m._compiled["rule"] == "sgd" and m._get_lr() == 0.5


def test_activity_regulariser_and_missing_weights_raise():
    G.clear_session()
    for make in (lambda: G.Conv2D(8, 1, activity_regularizer=R.l2(1e-4)),
                 lambda: G.DepthwiseConv2D(3, use_bias=False, activity_regularizer=R.l2(1e-4)),
                 lambda: G.BatchNormalization(activity_regularizer=R.l2(1e-4)),
                 lambda: Subpixel(3, 3, 2, activity_regularizer=R.l2(1e-4))):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(ValueError, match="no bias"):
        G.Conv2D(8, 1, use_bias=False, bias_regularizer=R.l2(1e-4))
    with pytest.raises(ValueError, match="no bias"):
        Subpixel(3, 3, 2, use_bias=False, bias_regularizer=R.l2(1e-4))
    with pytest.raises(ValueError, match="no such weight"):
        G.DepthwiseConv2D(3, use_bias=False, kernel_regularizer=R.l2(1e-4))
    with pytest.raises(ValueError, match="no such weight"):
        G.BatchNormalization(kernel_regularizer=R.l2(1e-4))
    with pytest.raises(ValueError, match="no such weight"):
        G.Conv2D(8, 1, gamma_regularizer=R.l2(1e-4))
    # set after construction: compile() refuses a regulariser that names a weight the layer does not have
    m = _model()
    nobias = next(l for l in m.layers if l.kind == "Conv2D" and not l.cfg["use_bias"])
    nobias.bias_regularizer = R.l2(1e-4)
    with pytest.raises(ValueError, match="does not have"):
        m.compile()
    nobias.bias_regularizer = None
    next(l for l in m.layers if l.kind == "BatchNormalization").kernel_regularizer = R.l2(1e-4)
    with pytest.raises(ValueError, match="does not have"):
        m.compile()


# ============================================================================================== add_weight_decay
def _model(backbone="mobilenetv2"):
    G.clear_session()
    return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone=backbone, OS=16)


def _names(m, kinds, suffix):
    return sorted(n for l in m.layers if l.kind in kinds for n in l.weights if n.endswith(suffix))


@pytest.mark.parametrize("backbone", ["mobilenetv2", "xception"])
def test_add_weight_decay_covers_the_convolution_kernels_by_default(backbone):
    m = _model(backbone)
    kernels = _names(m, ("Conv2D", "Subpixel"), "/kernel:0")
    dws = _names(m, ("DepthwiseConv2D",), "/depthwise_kernel:0")
    biases = _names(m, ("Conv2D", "Subpixel"), "/bias:0")
    bns = _names(m, ("BatchNormalization",), "/gamma:0") + _names(m, ("BatchNormalization",), "/beta:0")
    assert kernels and dws and biases and bns
    assert U.add_weight_decay(m) == len(kernels)
    m.compile()
    assert m._compiled["l2"] == {n: 4e-5 for n in kernels}            # depthwise=0 leaves the depthwise kernels bare
    assert all(l.depthwise_regularizer is None for l in m.layers if l.kind == "DepthwiseConv2D")
    n = U.add_weight_decay(m, l2=1e-4, depthwise=2e-4, bias=3e-4, batchnorm=5e-4)
    assert n == len(kernels) + len(dws) + len(biases) + len(bns)
    m.compile()
    want = dict({k: 1e-4 for k in kernels}, **{k: 2e-4 for k in dws})
    want.update({k: 3e-4 for k in biases})
    want.update({k: 5e-4 for k in bns})
    assert m._compiled["l2"] == want
    assert U.add_weight_decay(m, l2=0.0) == 0                          # 0.0 removes
    m.compile()
    assert m._compiled["l2"] == {}
    assert all(getattr(l, k, None) is None for l in m.layers for k in R.KEYWORDS)
    with pytest.raises(ValueError):
        U.add_weight_decay(m, l2=-1e-5)
    assert "compile()" in U.add_weight_decay.__doc__


# ================================================================================================== table builder
def _dry(monkeypatch, m, **kw):
    """tests/test_host.py::_dry_engine's method: the plan lowered without a GPU, the buffers on the CPU"""
    import torch
    from dl3_amd.engine import Engine
    capi.lib()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return Engine(m, batch=2, training=True, device="cpu", **kw)


def _check_table(e, kind, table):
    runs, coef, tiles = R.build_runs(e.slots, R.normal_form(table), kind)
    wr, wc, wt = LO.expected_table(e.slots, table, kind)
    assert runs.dtype == np.int64 and coef.dtype == np.float32
    assert runs.tolist() == wr and coef.tolist() == wc and tiles == wt
    n = e.n_param if kind == "p" else e.state.numel()
    prev_end, t = 0, 0
    for (first, length, tile0), c in zip(runs.tolist(), coef.tolist()):
        assert length >= 1 and first >= prev_end and first + length <= n    # ascending, disjoint, inside the arena
        assert tile0 == t and c > 0
        t += -(-length // R.TILE)
        prev_end = first + length
    assert t == tiles
    covered = np.zeros(n, bool)
    covered[LO.run_index([r[:2] for r in runs.tolist()])] = True
    for name, (k, off, size, _, _) in e.slots.items():
        if k == kind:
            assert covered[off:off + size].all() == (table.get(name, 0) > 0), name
            if table.get(name, 0) <= 0:
                assert not covered[off:off + size].any(), name                # a bare weight is on no run
    return runs, coef, tiles


def test_run_table_on_a_dry_engine_merges_neighbours_and_sends_frozen_layers_to_the_state_table(monkeypatch):
    m = _model()
    U.add_weight_decay(m, l2=4e-5, batchnorm=4e-5)
    frozen = m.get_layer("aspp0")
    frozen.trainable = False
    m.compile()
    table = m._compiled["l2"]
    e = _dry(monkeypatch, m, l2=table)
    assert e.l2 == R.normal_form(table)
    runs_p, _, _ = _check_table(e, "p", table)
    runs_s, _, _ = _check_table(e, "s", table)
    # a convolution kernel and the gamma / beta of the BatchNormalization behind it sit side by side with one l: fewer
    # runs than regularised weights
    n_p = sum(1 for n in table if e.slots[n][0] == "p")
    assert 1 <= len(runs_p) < n_p
    # the frozen layer's kernel is in the state arena's table and in no parameter run
    assert e.slots["aspp0/kernel:0"][0] == "s" and len(runs_s) >= 1
    off, size = e.slots["aspp0/kernel:0"][1:3]
    assert any(f <= off and off + size <= f + n for f, n, _ in runs_s.tolist())
    # the engine's own device tables are these
    assert e._l2["arenas"][0]["runs"].numpy().tolist() == runs_p.tolist()
    assert e._l2["arenas"][1]["runs"].numpy().tolist() == runs_s.tolist()
    # two different l on neighbours do not merge
    table2 = dict(table)
    some = sorted((v[1], n) for n, v in e.slots.items() if v[0] == "p" and n in table)[1][1]
    table2[some] = 8e-5
    runs2, coef2, _ = _check_table(e, "p", table2)
    assert len(runs2) > len(runs_p) and 8e-5 in [pytest.approx(c, rel=1e-6) for c in coef2.tolist()]
    with pytest.raises(ValueError, match="does not have"):
        R.build_runs(e.slots, R.normal_form({"no_such_layer/kernel:0": 1e-4}), "p")


def test_an_engine_without_a_table_has_none(monkeypatch):
    e = _dry(monkeypatch, _model())
    assert e.l2 is None and e._l2 is None
    e = _dry(monkeypatch, _model(), l2={})
    assert e.l2 is None and e._l2 is None


# ===================================================================================================== engine key
def test_engine_key_carries_the_table_and_compile_is_the_collection_point():
    m = _model()
    m.compile()
    plain_key, plain_kw = m._engine_key(2, True, {})
    assert "l2" not in plain_kw and sorted(plain_kw) == ["bn_update", "opt_trainable"]
    assert plain_key == (2, True, (), ("compiled", 1))                  # today's key
    U.add_weight_decay(m, l2=0.0)
    m.compile()
    key0, kw0 = m._engine_key(2, True, {})
    assert "l2" not in kw0 and key0[:3] == plain_key[:3]                # an empty table: the plain key and keywords
    assert m._engine_key(2, True, {"l2": {}})[0] == key0
    U.add_weight_decay(m, l2=4e-5)
    assert m._compiled["l2"] == {}                                      # set after compile(): not in force ...
    assert "l2" not in m._engine_key(2, True, {})[1]
    m.compile()                                                         # ... until the next compile()
    key1, kw1 = m._engine_key(2, True, {})
    assert len(m._compiled["l2"]) > 0 and kw1["l2"] == R.normal_form(m._compiled["l2"])
    U.add_weight_decay(m, l2=5e-5)
    m.compile()
    key2, kw2 = m._engine_key(2, True, {})
    assert key1[2] != key2[2] and kw1["l2"] != kw2["l2"]                # two tables, two keys
    hash(key1), hash(key2)
    # an inference engine's key never carries it
    assert m._engine_key(2, False, {}) == ((2, False, ()), {})


# ========================================================================================================= header
def test_header_exports_both_symbols():
    protos = capi.parse_header()
    assert [t for t, _ in protos["dl3_l2_penalty"][1]] == [
        "const float *", "float *", "const long long *", "const float *", "int", "long long", "float", "const float *",
        "double *", "void *", "size_t", "void *"]
    assert protos["dl3_l2_penalty_workspace_bytes"] == ("size_t", [("long long", "tiles")])
    L = capi.lib()
    assert L.dl3_l2_penalty_workspace_bytes(0) == 8 and L.dl3_l2_penalty_workspace_bytes(5) == 40
    assert L.dl3_l2_penalty_workspace_bytes(10 ** 9) == 2048 * 8       # grid-stride beyond one resident wave of workgroups
    assert "l2reg.hip" in open(capi.HEADER.replace("include/dl3.h", "keras-segmentation-deeplab-v3.1_amd/csrc/Makefile")).read()


# ========================================================================================================= oracle
def test_oracle_against_direct_numpy_sums():
    p = np.array([1.0, -2.0, 3.0, 0.5, 7.0, -0.25, 4.0, 9.0], np.float32)
    runs, coef = [(1, 3), (5, 2)], [0.5, 0.125]
    assert LO.penalty(p, runs, coef) == 0.5 * (4 + 9 + 0.25) + 0.125 * (0.0625 + 16)
    g = np.arange(8, dtype=np.float32)
    out, mag = LO.gradient(p, g, runs, coef, gs=0.5)
    want = g.astype(np.float64)
    want[1:4] += 2 * 0.5 * p[1:4] / 0.5
    want[5:7] += 2 * 0.125 * p[5:7] / 0.5
    assert np.array_equal(out, want) and np.array_equal(mag[[0, 4, 7]], [0.0, 4.0, 7.0]) and mag[1] == 1 + 4
    out, _ = LO.gradient(p, g, runs, coef, gs=0.5, denom=4.0)
    assert out[2] == 2 + 2 * 0.5 * 3.0 / 0.125
    assert float(LO.scale(0.5, 0.0)) == float(np.float32(0.5)) / 1e-20
    assert LO.run_index(runs).tolist() == [1, 2, 3, 5, 6]
    rng = np.random.default_rng(5)
    w = {"a": rng.normal(0, 1, (3, 3, 4, 5)).astype(np.float32), "b": rng.normal(0, 1, 7).astype(np.float32)}
    t = {"a": 4e-5, "b": 1e-3}
    direct = sum(float(np.float32(l)) * float((w[n].astype(np.float64) ** 2).sum()) for n, l in t.items())
    assert math.isclose(LO.model_penalty(w, t), direct, rel_tol=1e-14)
    assert math.isclose(LO.model_penalty(w, t), R.l2(float(np.float32(4e-5)))(w["a"]) + R.l2(float(np.float32(1e-3)))(w["b"]),
                        rel_tol=1e-14)
    slots = {"a": ("p", 0, 6, None, None), "b": ("p", 8, 2000, None, None), "c": ("p", 2008, 4, None, None),
             "d": ("s", 0, 5, None, None), "e": ("p", 2012, 3, None, None)}
    runs, coef, tiles = LO.expected_table(slots, {"a": 1e-4, "b": 1e-4, "d": 1e-4, "e": 2e-4}, "p")
    assert runs == [[0, 2008, 0], [2012, 3, 2]] and tiles == 3 and coef == [np.float32(1e-4), np.float32(2e-4)]
    assert LO.expected_table(slots, {"a": 1e-4, "b": 1e-4, "d": 1e-4}, "s") == ([[0, 5, 0]], [np.float32(1e-4)], 1)
