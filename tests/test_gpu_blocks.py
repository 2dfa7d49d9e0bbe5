"""-m gpu: the engine's backward wiring, block by block, at fp32 tolerance.

Every case of tests/block_cases.py — a graph of a few layers that takes ONE branch of the gradient-contribution protocol
(tests/test_block_cases_host.py asserts which) — runs one eager training step on the device and is compared with the
float64 graph walk of tests/graph_ref.py: logits, loss, every trainable gradient, the new moving statistics, and exact
zeros where nothing may be written.  A few hundred rows per BatchNorm channel and three or four layers of depth keep the
problem well conditioned, so the bar is fp32 rounding (2e-4 relative L2, or 4 x the float32 reference's own distance
where that is larger) — a residual gradient added twice, sums reduced against the neighbouring slice's mean or a
missing cB * y half of an addend's gradient are errors of percents."""
import numpy as np
import pytest
import torch

from tests import block_cases as BC
from tests.gpu_util import relerr
from tests.graph_ref import l2
from tests.test_block_cases_host import apply_knobs

pytestmark = pytest.mark.gpu


def _engine(c, monkeypatch, use_graph=False):
    """a fresh model of the case (an engine writes its moving statistics back into the model it belongs to) and its
    engine, lowered under the case's knobs"""
    apply_knobs(monkeypatch, c)
    model = BC.build(c, BC.seed_of(c))
    eng = model._engine(c.B, True, **BC.engine_kw(c, use_graph))
    assert c.pred(eng), (c.name, BC.names(eng.ops_bwd))
    return model, eng


def _state(eng, name):
    kind, off, n, shp, _ = eng.slots[name]
    assert kind == "s"
    return eng._unpad(name, eng.state[off:off + n].cpu().numpy().reshape(shp))


def _assert_zero_outside_the_gradients(eng):
    """the gradient arena outside the logical extent of every trainable tensor — the zero channels of a tensor stored
    wider than it is, the alignment gaps between slots, the tail — holds exact zeros"""
    g = eng.grads.cpu().numpy()
    logical = np.zeros(g.shape, bool)
    for name, (kind, off, n, shp, _) in eng.slots.items():
        if kind != "p":
            continue
        m = np.zeros(shp, bool)
        m[tuple(slice(0, k) for k in eng.hshape[name])] = True
        logical[off:off + n] = m.reshape(-1)
    assert np.isfinite(g).all()
    bad = np.nonzero(~logical & (g != 0))[0]
    assert bad.size == 0, ("written outside a gradient's logical extent", bad[:8], g[bad[:8]])


@pytest.mark.parametrize("c", BC.RUNNABLE, ids=lambda c: c.name)
def test_block_against_the_float64_graph_walk(monkeypatch, c):
    _, data, r64, r32 = BC.prepared(c)
    model, eng = _engine(c, monkeypatch)
    x, labels, sw = data
    eng.set_input(x)
    eng.set_targets(labels, sw)
    eng.fwd_bwd()
    torch.cuda.synchronize()
    el = relerr(eng.logits().reshape(r64.logits.shape), r64.logits)
    loss = float(eng.loss[0].item())
    print("%-24s logits %.2e loss %.2e" % (c.name, el, abs(loss - r64.loss) / abs(r64.loss)), end=" ")
    assert el < 1e-4, el
    assert abs(loss - r64.loss) < 1e-5 * abs(r64.loss), (loss, r64.loss)
    worst, failed, trained = (0.0, None, 0.0), [], 0
    for name, g in r64.grads.items():
        if not eng.trainable(name):
            assert eng.slots[name][0] == "s"     # no slot in the gradient arena at all
            continue
        trained += 1
        got = eng.grad_of(name)
        assert got.shape == g.shape and np.isfinite(got).all(), name
        if np.abs(g).max() < 1e-12:              # structurally zero in float64
            assert np.abs(got).max() < 1e-6, (name, np.abs(got).max())
            continue
        e, bar = l2(got, g), max(2e-4, 4.0 * l2(r32.grads[name], g))
        worst = max(worst, (e, name, bar))
        if e >= bar:
            failed.append((name, e, bar))
    print("| worst gradient %.2e (%s, bar %.1e) of %d tensors" % (worst[0], worst[1], worst[2], trained))
    assert not failed, failed
    assert trained == sum(1 for n in eng.slots if eng.slots[n][0] == "p") and trained > 0
    # moving statistics: updated where the reference updates them, untouched everywhere else
    for l in model.layers:
        if l.kind != "BatchNormalization":
            continue
        mm, mv = _state(eng, l.name + "/moving_mean:0"), _state(eng, l.name + "/moving_variance:0")
        if l.name in r64.new_stats:
            assert relerr(mm, r64.new_stats[l.name][0]) < 1e-5 and relerr(mv, r64.new_stats[l.name][1]) < 1e-5, l.name
        else:
            assert np.array_equal(mm, l.weights[l.name + "/moving_mean:0"]), l.name
            assert np.array_equal(mv, l.weights[l.name + "/moving_variance:0"]), l.name
    assert (c.kw.get("bn_mode") == "frozen") == (not r64.new_stats)
    _assert_zero_outside_the_gradients(eng)


@pytest.mark.parametrize("name", ["ir_res_stacked", "aspp", "decoder"])
def test_block_graph_replay_equals_eager(monkeypatch, name):
    """three calls of the captured plan (eager, capture + replay, replay) compute the bits of three eager calls:
    gradients, loss, logits and the moving statistics of three updates (the dropout step advances alike)"""
    c = BC.BY_NAME[name]
    x, labels, sw = BC.prepared(c)[1]
    got = []
    for use_graph in (False, True):
        model, eng = _engine(c, monkeypatch, use_graph)
        eng.set_input(x)
        eng.set_targets(labels, sw)
        for _ in range(3):
            eng.fwd_bwd()
        torch.cuda.synchronize()
        assert (eng.graph is not None) == use_graph
        got.append((eng.grads.cpu().numpy().copy(), float(eng.loss[0].item()), eng.state.cpu().numpy().copy(),
                    eng.logits().copy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert np.abs(got[0][0]).max() > 0
