"""-m gpu: L2 weight regularisers — dl3_l2_penalty through the C ABI against the float64 restatement in
tests/l2_oracle.py, Engine.l2_penalty on given gradients, and kernel_regularizer=l2(...) / utils.add_weight_decay through
Model.compile, train_on_batch, fit and evaluate against an unregularised twin at the same weights.

The value is accumulated in double from exact squares: at most n additions and one product per tile and lane, each rounding
at 2**-53 of a partial sum of non-negative terms — |out[0] - fsum| <= n * 2**-52 * fsum (n: the elements on the runs).
The gradient addend is counted as tests/test_gpu_optimizers.py counts the effective gradient, relative to the magnitude
|g| + |(2 l w) / sc| of the one sum an element is made of:
  (2 l) * w                               1   (2 * l is exact)
  sc = gs / max(denom, 1e-20)            +1   (the denom forms only)
  the quotient by sc                      1   (exact for sc == 1, counted all the same)
  g + addend                              1
so 3 roundings, 4 in the denom forms.  Behind it the step multiplies by sc and applies the rule: SGD without momentum adds
g' * sc (1), lr * g' (1) and p + v (1): 6 (7) from the weight's point of view, on |w| + lr * (|g| sc + |2 l w|).
The reported loss is the float data loss plus the double penalty, added in double on the host: against the twin's loss
(the same float, the step being deterministic) plus the oracle's penalty it is off by the penalty's own bound and a few
double operations (_assert_loss)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import l2_oracle as LO
from tests import ops_oracle as OO
from tests import optim_oracle as PO
from tests.gpu_util import dev, host, ptr, release

pytestmark = pytest.mark.gpu

f32 = np.float32
BIG = 1048576 + 777   # test_gpu_optimizers.NS's last: 1025 tiles of 1024 elements — still ONE trip of the 2048-workgroup grid
LONG = 5 * 1048576 + 777   # 5121 tiles: the grid-stride path, three trips for the first workgroups, two for the rest
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, BIG]
SCALES = {"plain": (0.5, None), "denom": (0.5, 1234.0), "denom_zero": (0.5, 0.0)}   # test_gpu_optimizers.SCALES


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    return capi.lib()


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for fam in sorted(OO.RATIOS):
        print("\nworst error / bound, %-22s %.3f" % (fam, OO.RATIOS[fam]), end="")
    print()


# ========================================================================================================== C ABI
def _layout(name):
    """-> (runs [(first, length)], n): gaps between the runs, the first run at an offset > 0, the last run ending at n"""
    if name == "one":          # S = 1
        return [(8, 1025)], 8 + 1025
    if name == "eight":        # every length of the issue once; starts 4-aligned and not (the quad path and the scalar one)
        lengths, gaps = LENGTHS, [4, 3, 1, 4, 7, 8, 2, 6]   # (the long run starts aligned)
    elif name == "long":       # 2 + 5121 + 1 + 1 + 2 = 5127 tiles on 2048 workgroups: every workgroup takes a second tile, the
        # first 1031 a third; a run boundary inside the later trips; the long run 4-aligned, the last one not
        lengths, gaps = [1025, LONG, 3, 1024, 1500], [4, 7, 2, 3, 2]
    else:                      # S = 300
        lengths, gaps = [[1, 3, 4, 5, 1023, 1024, 1025, 17, 2048, 4100][i % 10] for i in range(300)], [1, 4, 7, 8, 3]
    runs, at = [], 0
    for i, n in enumerate(lengths):
        at += gaps[i % len(gaps)]
        runs.append((at, n))
        at += n
    return runs, at


def _table(runs):
    out, t = np.zeros((len(runs), 3), np.int64), 0
    for s, (first, n) in enumerate(runs):
        out[s] = (first, n, t)
        t += -(-n // LO.TILE)
    return out, t


_CASES = {}


def _case(name):
    """arena, gradients, coefficients and the oracle's value of a layout, computed once.  p outside the runs is NaN: an
    element read there would turn the value into NaN"""
    if name not in _CASES:
        runs, n = _layout(name)
        rng = np.random.default_rng(2301 + len(runs))
        idx = LO.run_index(runs)
        p = np.full(n, np.nan, f32)
        p[idx] = (rng.normal(0, 1, idx.size) * 10.0 ** rng.uniform(-4, 1, idx.size)).astype(f32)
        g = rng.normal(0, 1e-3, n).astype(f32)
        coef = (10.0 ** rng.uniform(-5, -2, len(runs))).astype(f32)
        if len(runs) > 2:
            coef[1] = 0.0            # l = 0 is a valid coefficient: the run counts nothing
        _CASES[name] = dict(runs=runs, n=n, idx=idx, p=p, g=g, coef=coef, want=LO.penalty(p, runs, coef))
    return _CASES[name]


def _f64(value, n):
    return torch.full((n,), value, dtype=torch.float64, device="cuda")


def _penalty_call(L, c, mode, lead, scale=None):
    """one dl3_l2_penalty launch as the engine issues it; mode: "value" (g = NULL) or a key of SCALES (scale: another
    (grad_scale, denom)); g lives in a sentinel-guarded buffer that holds values on the runs only; lead = 1 puts p and g one
    float past a 16-byte boundary (the scalar path).  -> (out[2], g on the runs or None)"""
    from dl3_amd import capi
    runs, n, idx = c["runs"], c["n"], c["idx"]
    tab, tiles = _table(runs)
    tab_d = torch.from_numpy(tab).cuda()
    coef_d = dev(c["coef"])
    pb = np.concatenate([np.full(lead, np.nan, f32), c["p"], np.full(3, np.nan, f32)])
    pd = dev(pb)
    assert pd.data_ptr() % 16 == 0
    gd = None
    gs, denom = scale or SCALES.get(mode, (1.0, None))
    if mode != "value":
        gb = OO.guard_buffer(n, 1, lead=lead)
        gb[lead + idx] = 0.0 if mode == "denom_zero" else c["g"][idx]
        gd = dev(gb)
    dd = None if denom is None else dev(np.array([denom], f32))
    need = int(L.dl3_l2_penalty_workspace_bytes(tiles))
    assert need == 8 * min(tiles, 2048)
    ws = _f64(float("nan"), need // 8 + 3)
    out = _f64(float("nan"), 4)      # [guard, value, value as float, guard]
    capi.call("dl3_l2_penalty", ptr(pd, lead), None if gd is None else ptr(gd, lead), tab_d.data_ptr(), ptr(coef_d),
              len(runs), tiles, gs, None if dd is None else ptr(dd), out.data_ptr() + 8, ws.data_ptr(), need,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[3])                                  # exactly two doubles are written
    assert np.isnan(ws.cpu().numpy()[need // 8:]).all()                       # nothing behind the promised workspace
    assert np.array_equal(host(pd).view(np.uint32), pb.view(np.uint32))       # p is never written
    got = None
    if gd is not None:
        hb = host(gd)
        OO.assert_guard(hb, lead + idx)                                       # g off the runs: the sentinel, bit for bit
        got = hb[lead + idx]
    del tab_d
    release()
    return o[1:3].copy(), got


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("mode", ["value", "plain", "denom", "denom_zero"])
@pytest.mark.parametrize("layout", ["one", "eight", "many", "long"])
def test_l2_penalty_follows_the_oracle(L, layout, mode, lead):
    """S = 1, 8 and 300 runs with gaps, and five runs of 5127 tiles in all (the grid has 2048 workgroups: the only layout
    whose workgroups take a second and a third tile); value-only (g = NULL) and the three scale forms; 16-byte aligned and
    one float off.  Two launches give the same bits."""
    c = _case(layout)
    tiles = _table(c["runs"])[1]
    assert (tiles > 2 * 2048) == (layout == "long") and (layout == "long" or tiles <= 2048)
    (a, ga), (b, gb) = _penalty_call(L, c, mode, lead), _penalty_call(L, c, mode, lead)
    want, n = c["want"], c["idx"].size
    err, bound = abs(float(a[0]) - want), n * 2.0 ** -52 * want
    print("l2 value %s/%s/lead %d: S %d, n %d, value %.17g, err %.3e, bound %.3e" % (layout, mode, lead, len(c["runs"]), n,
                                                                                  a[0], err, bound))
    assert want > 0 and err <= bound
    assert a[1] == float(f32(a[0]))                                           # out[1]: out[0] rounded once to float
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if mode == "value":
        assert ga is None
        return
    gs, denom = SCALES[mode]
    g = np.zeros(c["n"], f32) if mode == "denom_zero" else c["g"]
    ref, mag = LO.gradient(np.nan_to_num(c["p"]), g, c["runs"], c["coef"], gs, denom)
    OO.assert_elementwise(ga, ref[c["idx"]], mag[c["idx"]], 3 + (denom is not None), "l2_penalty gradient")
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    if mode == "plain":   # the addend is there: without it the bound fails by orders of magnitude
        assert np.abs(ga.astype(np.float64) - g[c["idx"]]).max() > 1e3 * 2 * 3 * OO.U * mag[c["idx"]].max()


def test_l2_penalty_scale_one_divides_exactly(L):
    """sc == 1: the quotient is exact, so g == fl(g0 + fl(2 l w)) bit for bit"""
    c = _case("one")
    _, got = _penalty_call(L, c, "plain", 0, scale=(1.0, None))
    idx = c["idx"]
    want = (c["g"][idx] + (f32(2.0) * c["coef"][0]) * c["p"][idx]).astype(f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("bare", [False, True])
def test_l2_penalty_without_runs_writes_zeros(L, bare):
    """S == 0: out = {0, 0}; bare: without coefficients and without a workspace, which the call does not look at then"""
    from dl3_amd import capi
    out, ws = _f64(float("nan"), 4), _f64(float("nan"), 4)
    t = dev(np.ones(8, f32))
    tab = torch.zeros(3, dtype=torch.int64, device="cuda")
    capi.call("dl3_l2_penalty", ptr(t), ptr(t), tab.data_ptr(), None if bare else ptr(t), 0, 0, 1.0, None, out.data_ptr() + 8,
              None if bare else ws.data_ptr(), 0 if bare else 8, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[3]) and o[1] == 0.0 and o[2] == 0.0
    assert np.array_equal(host(t), np.ones(8, f32)) and np.isnan(ws.cpu().numpy()).all()


def test_l2_penalty_refusals_write_nothing(L):
    c = _case("one")
    tab, tiles = _table(c["runs"])
    tab_d = torch.from_numpy(tab).cuda()
    pd, gd, cd = dev(np.nan_to_num(c["p"])), dev(np.full(c["n"], 7.0, f32)), dev(c["coef"])
    need = int(L.dl3_l2_penalty_workspace_bytes(tiles))
    ws, out = _f64(-3.0, need // 8 + 1), _f64(-1.0, 3)
    P, G, T, C, O, W = ptr(pd), ptr(gd), tab_d.data_ptr(), ptr(cd), out.data_ptr(), ws.data_ptr()
    assert L.dl3_l2_penalty(P, G, T, C, -1, tiles, 1.0, None, O, W, need, None) == -1          # S < 0
    assert L.dl3_l2_penalty(None, G, T, C, 1, tiles, 1.0, None, O, W, need, None) == -1        # no arena
    assert L.dl3_l2_penalty(P, G, T, C, 1, tiles, 1.0, None, None, W, need, None) == -1        # no result
    assert L.dl3_l2_penalty(P, G, None, C, 1, tiles, 1.0, None, O, W, need, None) == -1        # no table
    assert L.dl3_l2_penalty(P, G, None, C, 0, 0, 1.0, None, O, W, need, None) == -1            # ... also without runs
    assert L.dl3_l2_penalty(P, G, T, None, 1, tiles, 1.0, None, O, W, need, None) == -1        # no coefficients
    assert L.dl3_l2_penalty(P, G, T, C, 1, tiles, 1.0, None, O + 4, W, need, None) == -1       # misaligned result
    assert L.dl3_l2_penalty(P, G, T, C, 1, tiles, 1.0, None, O, W + 4, need, None) == -1       # misaligned workspace
    assert L.dl3_l2_penalty(P, G, T, C, 1, 0, 1.0, None, O, W, need, None) == -1               # fewer tiles than runs
    assert L.dl3_l2_penalty(P, G, T, C, 1, tiles, 0.0, None, O, W, need, None) == -1           # a scale it cannot divide by
    for short_ptr, short_bytes in ((W, need - 8), (W, 0), (None, need)):
        assert L.dl3_l2_penalty(P, G, T, C, 1, tiles, 1.0, None, O, short_ptr, short_bytes, None) == -3   # DL3_EWORKSPACE
        assert b"workspace" in L.dl3_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1.0).all() and (ws.cpu().numpy() == -3.0).all()
    assert (host(gd) == 7.0).all()                                                             # nothing was launched


# ========================================================================================================== engine
SHAPE, CLASSES, B = (64, 64, 3), 3, 2
DECAY = dict(l2=1e-3, depthwise=5e-4, bias=2e-3, batchnorm=1e-4)   # every keyword on, four different l


def _model(head="deeplab", decay=None, optimizer=None, loss=None, freeze=(), metrics=None):
    """MobileNetV2 64x64x3, 3 classes, the oracle's initial weights (seed 1); decay: add_weight_decay's keywords"""
    from dl3_amd import utils as U
    from tests.test_gpu_model import _build, _load
    model, params = _build("mobilenetv2", SHAPE, CLASSES, head)
    _load(model, params)
    for name in freeze:
        model.get_layer(name).trainable = False
    if decay is not None:
        U.add_weight_decay(model, **decay)
    model.compile(optimizer=optimizer, loss=loss, metrics=metrics)
    return model


def _batches(n, b=B, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x = rng.integers(0, 256, (b,) + SHAPE).astype(f32)
        y = rng.integers(0, CLASSES + 1, (b, SHAPE[0] * SHAPE[1], 1)).astype(f32)
        sw = ((y[..., 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2])).astype(f32)
        out.append((x, y, sw))
    return out


def _np64(t, n=None):
    torch.cuda.synchronize()
    return t[:n].cpu().numpy().astype(np.float64)


def _arena_l(eng, table):
    """per element of the parameter arena: the float l the device holds (0 off the regularised weights)"""
    lam = np.zeros(eng.n_param, np.float64)
    for name, l in table.items():   # noqa: E741
        kind, off, size = eng.slots[name][:3]
        if kind == "p":
            lam[off:off + size] = float(f32(l))
    return lam


def _host_penalty(eng, table):
    """the oracle's penalty of the weights resident on the engine (both arenas)"""
    hp, hs = eng.params.cpu().numpy(), eng.state.cpu().numpy()
    w = {n: (hp if eng.slots[n][0] == "p" else hs)[eng.slots[n][1]:eng.slots[n][1] + eng.slots[n][2]] for n in table}
    return LO.model_penalty(w, table), sum(a.size for a in w.values())


def _assert_loss(got, twin, pen, n, what):
    """got = float data loss + double penalty against twin + the oracle's penalty: the penalty's own bound (n elements) and
    a few double operations — the addition; the two arenas' sum; under fit the batch-size-weighted mean (4 in all)"""
    err, bound = abs(got - (twin + pen)), n * 2.0 ** -52 * pen + 4 * 2.0 ** -52 * abs(twin + pen)
    print("%s: loss %.12f = twin %.9f + penalty %.12f, err %.3e, bound %.3e" % (what, got, twin, pen, err, bound))
    assert pen > 1e-6 * abs(twin), "the penalty is too small for this check to see it"
    assert err <= bound


@pytest.mark.parametrize("frozen", [False, True])
def test_engine_penalty_on_given_gradients(frozen):
    """Engine.l2_penalty on a gradient arena filled by hand (zeros on the slots' padding, as a backward pass leaves them)
    against the oracle over the whole arena; frozen: a regularised layer the optimizer does not update sits in the state
    arena — its weights add to the value, and nothing outside the parameter runs is touched"""
    from dl3_amd import regularizers as R
    model = _model(decay=DECAY, freeze=("aspp0",) if frozen else ())
    table = model._compiled["l2"]
    eng = model._engine(B, True, dropout=False, use_graph=False)
    assert eng.l2 == R.normal_form(table) and ("aspp0/kernel:0" in table)
    assert (eng.slots["aspp0/kernel:0"][0] == "s") == frozen and (eng._l2["arenas"][1] is not None) == frozen
    n = eng.n_param
    live = np.zeros(eng.grads.numel(), bool)
    for name, (kind, off, size, _, _) in eng.slots.items():
        if kind == "p":
            live[off:off + size] = True
    rng = np.random.default_rng(33)
    g = np.where(live, rng.normal(0, 1e-3, live.size), 0.0).astype(f32)
    g[eng.tail:] = [5.0, 6.0, 7.0, 8.0]                                         # the arena's tail is not the penalty's
    eng.grads.copy_(torch.from_numpy(g).cuda())
    dummy = eng.dummy_grad.clone()
    p = eng.params.cpu().numpy()
    eng.l2_penalty(0.5)
    torch.cuda.synchronize()
    got, out = eng.grads.cpu().numpy(), eng._l2["out"].cpu().numpy()
    runs_p, coef_p, _ = LO.expected_table(eng.slots, table, "p")
    runs_p = [r[:2] for r in runs_p]
    ref, mag = LO.gradient(p[:n], g[:n], runs_p, coef_p, 0.5)
    idx = LO.run_index(runs_p)
    OO.assert_elementwise(got[idx], ref[idx], mag[idx], 3, "l2 engine gradient")
    off_runs = np.ones(g.size, bool)
    off_runs[idx] = False
    assert np.array_equal(got[off_runs].view(np.uint32), g[off_runs].view(np.uint32))     # bare weights, gaps, the tail
    assert not got[:n][~live[:n]].any()                                                    # the padding stays exactly zero
    assert np.array_equal(eng.dummy_grad.cpu().numpy(), dummy.cpu().numpy())               # a frozen layer's throw-away slot
    assert np.array_equal(eng.params.cpu().numpy().view(np.uint32), p.view(np.uint32))
    want, cnt = _host_penalty(eng, table)
    # ... which is the penalty of the layers' own host weights, whatever the arenas' layout
    by_layer = {n: w for l in model.layers for n, w in l.weights.items() if n in table}
    assert sorted(by_layer) == sorted(table) and abs(LO.model_penalty(by_layer, table) - want) <= 2.0 ** -50 * want
    want = LO.model_penalty(by_layer, table)
    val = float(out[0]) + float(out[2])
    print("engine penalty (frozen %s): %.15g, oracle %.15g, state share %.6g" % (frozen, val, want, out[2]))
    assert abs(val - want) <= cnt * 2.0 ** -52 * want
    assert out[1] == float(f32(out[0])) and out[3] == float(f32(out[2]))
    assert (out[2] > 0) == frozen
    if frozen:   # the state arena's share is the frozen kernel's penalty
        k = model.get_layer("aspp0").weights["aspp0/kernel:0"]
        share = LO.model_penalty({"aspp0/kernel:0": k}, {"aspp0/kernel:0": table["aspp0/kernel:0"]})
        assert abs(float(out[2]) - share) <= k.size * 2.0 ** -52 * share
    assert eng.l2_value(table) == val                                                      # the evaluation form: same tables


# =========================================================================================================== model
def test_train_on_batch_sgd_step_and_loss_against_the_twin():
    """SGD(lr, momentum=0): w' = w - lr * (g_twin + 2 l w) within 6 roundings (the file's docstring); the loss is the
    twin's plus the oracle's penalty of the pre-step weights; lazy_loss=True gives the same number"""
    from dl3_amd.optimizers import SGD
    lr = 0.05
    (x, y, sw), = _batches(1)
    twin = _model(optimizer=SGD(lr=lr, momentum=0.0))
    lt = twin.train_on_batch(x, y, sw, dropout=False)
    gt = _np64(twin._active.grads, twin._active.n_param)
    losses = []
    for lazy in (False, True):
        model = _model(decay=DECAY, optimizer=SGD(lr=lr, momentum=0.0))
        table = model._compiled["l2"]
        eng = model._engine(B, True, dropout=False)
        n = eng.n_param
        before = _np64(eng.params, n)
        pen, cnt = _host_penalty(eng, table)
        loss = model.train_on_batch(x, y, sw, dropout=False, lazy_loss=lazy)
        assert model._active is eng and eng.iteration == 1
        if lazy:
            from dl3_amd.engine import LazyLoss
            assert isinstance(loss, LazyLoss)
        losses.append(float(loss))
        _assert_loss(losses[-1], lt, pen, cnt, "train_on_batch lazy=%s" % lazy)
        lam, lr32 = _arena_l(eng, table), float(f32(lr))
        add = 2.0 * lam * before
        OO.assert_elementwise(_np64(eng.params, n), before - lr32 * (gt + add), np.abs(before) + lr32 * (np.abs(gt) + np.abs(add)),
                              6, "l2 sgd step")
        OO.assert_elementwise(_np64(eng.grads, n), gt + add, np.abs(gt) + np.abs(add), 3, "l2 model gradient")
        mag = np.abs(before) + lr32 * (np.abs(gt) + np.abs(add))
        assert np.any(np.abs(_np64(eng.params, n) - (before - lr32 * gt)) > 100 * 12 * OO.U * mag)   # the addend is visible
    assert losses[0] == losses[1]
    assert np.any(np.abs(_np64(eng.params, n) - _np64(twin._active.params, n)) > 0)


def test_clipnorm_sees_the_gradient_of_the_total_loss():
    """a clip level between the data gradient's norm d and the total gradient's: l is chosen so that the penalty's gradient
    has norm 3 d — the total norm is then between 2 d and 4 d — and clipnorm = 1.5 d.  The regularised model's update has
    norm lr * clipnorm (test_train_on_batch_clipnorm_limits_the_applied_update's check); the twin at the same level is not
    clipped: its update has norm lr * d."""
    from dl3_amd.optimizers import SGD
    (x, y, sw), = _batches(1, seed=11)
    probe = _model(optimizer=SGD(lr=0.0))       # a step that moves nothing: measures the data gradient's norm
    probe.train_on_batch(x, y, sw, dropout=False)
    e0 = probe._active
    n = e0.n_param
    d = float(np.linalg.norm(_np64(e0.grads, n)))
    wn = math.sqrt(sum(float((w.astype(np.float64) ** 2).sum()) for l in probe.layers if l.kind == "Conv2D"
                       for k, w in l.weights.items() if k.endswith("/kernel:0")))
    assert d > 0 and wn > 0
    l, lr, c = 1.5 * d / wn, 0.1, 1.5 * d   # noqa: E741
    model = _model(decay=dict(l2=l), optimizer=SGD(lr=lr, clipnorm=c))
    twin = _model(optimizer=SGD(lr=lr, clipnorm=c))
    upd = []
    for m in (model, twin):
        eng = m._engine(B, True, dropout=False)
        before = _np64(eng.params, n)
        m.train_on_batch(x, y, sw, dropout=False)
        assert m._active is eng
        upd.append(float(np.linalg.norm(_np64(eng.params, n) - before)))
    total = float(np.linalg.norm(_np64(model._active.grads, n)))
    print("clipnorm: data gradient norm %.6g, l %.4g, total norm %.6g, c %.6g; update norm / (lr c) - 1 = %.3e (regularised), "
          "twin update / (lr d) - 1 = %.3e" % (d, l, total, c, upd[0] / (lr * c) - 1, upd[1] / (lr * d) - 1))
    assert 1.9 * d <= total <= 4.1 * d
    assert abs(upd[0] - lr * c) <= 1e-5 * lr * c
    assert abs(upd[1] - lr * d) <= 1e-5 * lr * d      # the twin moved by lr * |g|: below the level, not clipped


def test_world_of_one_data_parallel_step():
    """Model.distribute() with an RCCL communicator of one rank (every launch of the N-rank step on one GPU).  Against the
    data-parallel TWIN (the external_nnz engine, no regulariser) the arena after the step holds g_twin + (2 l w) / sc — 4
    roundings, sc = c0 / count finished on the device — and the weights follow within 7; the loss is the twin's plus the
    penalty ONCE.  Against the single-process step: the two regularised steps differ by what their twins' data gradients
    differ (the denom form differentiates sum / c0 and multiplies by c0 / count) plus the counted roundings of both, 7 + 6."""
    from dl3_amd.optimizers import SGD
    from dl3_amd.parallel import DataParallel
    assert int(os.environ.get("WORLD_SIZE", "1")) == 1
    lr = 0.05
    (x, y, sw), = _batches(1, seed=13)

    def run(mode, decay):
        model = _model(decay=decay, optimizer=SGD(lr=lr, momentum=0.0))
        dp, kw = None, dict(dropout=False)
        if mode == "rccl":
            dp = DataParallel().attach_single_rank_rccl()
            model.distribute(dp)
        elif mode == "tail":
            kw["external_nnz"] = True
        eng = model._engine(B, True, **dict(kw, external_nnz=True) if mode != "plain" else kw)
        before = _np64(eng.params, eng.n_param)
        pen, cnt = _host_penalty(eng, model._compiled["l2"]) if decay else (0.0, 0)
        loss = model.train_on_batch(x, y, sw, **kw)
        assert model._active is eng and eng.external_nnz == (mode != "plain") and eng.iteration == 1
        torch.cuda.synchronize()
        res = dict(loss=loss, before=before, pen=pen, cnt=cnt, eng=eng, model=model, p=eng.params.cpu().numpy(),
                   g=eng.grads.cpu().numpy())
        if dp is not None:
            dp.close()
        return res

    tw, rccl, ptw, plain = run("tail", None), run("rccl", DECAY), run("plain", None), run("plain", DECAY)
    eng = rccl["eng"]
    n, table = eng.n_param, rccl["model"]._compiled["l2"]
    count = float(tw["g"][eng.tail])
    assert count > 0 and rccl["g"][eng.tail] == tw["g"][eng.tail]
    sc = float(LO.scale(eng.nnz_host, count))
    gt, before = tw["g"][:n].astype(np.float64), rccl["before"]
    add = 2.0 * _arena_l(eng, table) * before
    OO.assert_elementwise(rccl["g"][:n], gt + add / sc, np.abs(gt) + np.abs(add) / sc, 4, "l2 data-parallel gradient")
    lr32 = float(f32(lr))
    mag = np.abs(before) + lr32 * (np.abs(gt) * sc + np.abs(add))
    OO.assert_elementwise(rccl["p"][:n], before - lr32 * (gt * sc + add), mag, 7, "l2 data-parallel step")
    _assert_loss(rccl["loss"], tw["loss"], rccl["pen"], rccl["cnt"], "world of one")
    # the single-process step
    assert np.array_equal(plain["before"], before)
    gp = ptw["g"][:n].astype(np.float64)
    err = np.abs(rccl["p"][:n].astype(np.float64) - plain["p"][:n].astype(np.float64))
    bound = lr32 * np.abs(gt * sc - gp) + 2 * (7 + 6) * OO.U * np.maximum(mag, np.abs(before) + lr32 * (np.abs(gp) + np.abs(add)))
    print("data-parallel against single-process step: worst error / bound %.3f; data gradients differ by %.3e of their norm"
          % (OO.worst_ratio(err, bound), np.linalg.norm(gt * sc - gp) / np.linalg.norm(gp)))
    assert np.all(err <= bound)
    assert np.linalg.norm(gt * sc - gp) <= 1e-3 * np.linalg.norm(gp)     # (the twins do compute the same gradient)
    _assert_loss(plain["loss"], ptw["loss"], plain["pen"], plain["cnt"], "single process")
    assert plain["pen"] == rccl["pen"]


@pytest.mark.parametrize("head", ["deeplab", "subpixel"])
def test_three_adam_steps_under_graph_replay_follow_the_float64_replay(head):
    """three steps on three batches — eager, capture, replay — with Adam.  The data gradient of each step comes from an
    unregularised twin ENGINE that is handed the regularised model's weights and moving statistics before the step and
    takes a step of lr = 0 on the same batch; the arena then holds g_twin + 2 l w within 3 roundings of |g_twin| + |2 l w|,
    and the weights follow optim_oracle.keras_step in float64 fed that arena (the sum just checked: where g_twin and 2 l w
    cancel, Adam's m / sqrt(v) would magnify the sum's own rounding past any bar) — with test_engine_opt_step_follows_the_
    oracle_on_given_gradients' bar for Adam: 1e-4 of the summed step sizes plus one rounding of the weight per step.  The
    penalty launches are not in the plan: the recorded launches are the twin's."""
    from dl3_amd.optimizers import SGD, Adam
    hyper = dict(lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.1)
    model = _model(head, decay=DECAY, optimizer=Adam(**hyper))
    twin = _model(head, optimizer=SGD(lr=0.0))
    table = model._compiled["l2"]
    eng, te = model._engine(B, True, dropout=False), twin._engine(B, True, dropout=False)
    n = eng.n_param
    assert te.n_param == n and te.l2 is None and eng.l2
    lam = _arena_l(eng, table)
    p0 = _np64(eng.params, n)
    p, m, v, steps, gts = p0.copy(), np.zeros(n), np.zeros(n), np.zeros(n), []
    for it, (x, y, sw) in enumerate(_batches(3, seed=17)):
        te.params.copy_(eng.params)
        te.state.copy_(eng.state)
        te.dirty = True
        w = _np64(eng.params, n)
        pen, cnt = _host_penalty(eng, table)
        lt = twin.train_on_batch(x, y, sw, dropout=False)
        assert twin._active is te
        gt = _np64(te.grads, n)
        loss = model.train_on_batch(x, y, sw, dropout=False)
        assert model._active is eng
        _assert_loss(loss, lt, pen, cnt, "%s step %d" % (head, it))
        add = 2.0 * lam * w
        OO.assert_elementwise(_np64(eng.grads, n), gt + add, np.abs(gt) + np.abs(add), 3, "l2 model gradient")
        gts.append(gt)
        q, m, v = PO.keras_step("adam", p, _np64(eng.grads, n), m, v, it, **hyper)
        steps += np.abs(q - p)
        p = q
    assert eng.iteration == 3 and eng.graph is not None, "the step was never captured"
    assert [r[0] for r in eng.ops_fwd] == [r[0] for r in te.ops_fwd] and [r[0] for r in eng.ops_bwd] == [r[0] for r in te.ops_bwd]
    assert not any("l2" in r[0] for r in eng.ops_prep + eng.ops_fwd + eng.ops_bwd)
    err = np.abs(_np64(eng.params, n) - p)
    bound = 3 * 6e-8 * np.maximum(np.abs(p), np.abs(p0)) + 1e-4 * steps
    print("%s adam replay: worst error / bound %.3f" % (head, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
    # and the penalty is in it: the replay of the twin's gradients alone ends elsewhere
    q, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for it, gt in enumerate(gts):
        q, m, v = PO.keras_step("adam", q, gt, m, v, it, **hyper)
    assert np.any(np.abs(q - p) > 1e2 * bound)


def test_evaluation_and_validation_report_the_penalty_once():
    """evaluate(device=True), evaluate(device=False), evaluate_generator and val_loss of fit(validation_data=): the twin's
    number plus the penalty; Jaccard and accuracy are the twin's.  SGD(lr=0): the weights do not move during fit, the moving
    statistics move alike in both models."""
    from dl3_amd.optimizers import SGD
    from dl3_amd import utils as U
    (x, y, sw), = _batches(1, b=4, seed=19)
    metrics = [U.Jaccard, U.sparse_accuracy_ignoring_last_label]
    res = {}
    for name, decay in (("twin", None), ("reg", dict(DECAY))):
        model = _model(decay=decay, optimizer=SGD(lr=0.0), metrics=metrics)
        r = dict(dev=model.evaluate(x, y, batch_size=3, sample_weight=sw, device=True),       # batches of 3 and 1
                 host=model.evaluate(x, y, batch_size=2, sample_weight=sw),
                 gen=model.evaluate_generator([(x[:2], y[:2], sw[:2]), (x[2:], y[2:], sw[2:])]))
        if decay:
            r["pen"], r["cnt"] = _host_penalty(model._active, model._compiled["l2"])
        hist = model.fit(x, y, batch_size=2, epochs=1, sample_weight=sw, validation_data=(x, y, sw))
        r["hist"] = hist.history
        res[name] = r
    t, r = res["twin"], res["reg"]
    for k in ("dev", "host", "gen"):
        _assert_loss(r[k][0], t[k][0], r["pen"], r["cnt"], "evaluate %s" % k)
        assert r[k][1:] == t[k][1:]
    _assert_loss(r["hist"]["val_loss"][0], t["hist"]["val_loss"][0], r["pen"], r["cnt"], "val_loss")
    _assert_loss(r["hist"]["loss"][0], t["hist"]["loss"][0], r["pen"], r["cnt"], "History loss")
    for k in ("val_Jaccard", "val_sparse_accuracy_ignoring_last_label"):
        assert r["hist"][k] == t["hist"][k]


def test_off_is_off():
    """add_weight_decay(model, l2=0.0) + compile(): three steps bit for bit those of a model that never saw a regulariser,
    on the plain engine key, without a penalty table"""
    from dl3_amd import utils as U
    off, plain = _model(decay=dict(l2=0.0)), _model()
    once = _model(decay=dict(l2=4e-5))
    assert U.add_weight_decay(once, l2=0.0) == 0
    once.compile()
    assert off._engine_key(B, True, {}) == plain._engine_key(B, True, {})
    assert once._engine_key(B, True, {})[0][:3] == plain._engine_key(B, True, {})[0][:3]
    for x, y, sw in _batches(3, seed=23):
        la, lb, lc = off.train_on_batch(x, y, sw), plain.train_on_batch(x, y, sw), once.train_on_batch(x, y, sw)
        assert la == lb == lc
    torch.cuda.synchronize()
    for name in ("params", "state", "adam_m", "adam_v", "grads"):
        a, b, c = (getattr(m._active, name).cpu().numpy().view(np.uint32) for m in (off, plain, once))
        assert np.array_equal(a, b) and np.array_equal(a, c), name
    assert off._active.l2 is None and off._active._l2 is None and once._active._l2 is None
    assert off.evaluate(x, y, sample_weight=sw, device=True) == plain.evaluate(x, y, sample_weight=sw, device=True)
    assert not off._active._l2_eval


def test_focal_loss_with_a_regulariser():
    """the penalty is independent of the loss tail: one step with utils.sparse_focal_crossentropy, loss = twin + penalty"""
    from dl3_amd import utils as U
    (x, y, sw), = _batches(1, seed=29)
    twin = _model(loss=U.sparse_focal_crossentropy(2.0, (0.5, 1.0, 2.0)))
    model = _model(decay=DECAY, loss=U.sparse_focal_crossentropy(2.0, (0.5, 1.0, 2.0)))
    eng = model._engine(B, True, dropout=False)
    pen, cnt = _host_penalty(eng, model._compiled["l2"])
    lt = twin.train_on_batch(x, y, sw, dropout=False)
    loss = model.train_on_batch(x, y, sw, dropout=False)
    assert model._active is eng and eng.focal is not None and eng.l2
    _assert_loss(loss, lt, pen, cnt, "focal")


def test_device_feed_equals_the_host_array_path():
    """fit_generator(device_feed=True) on a regularised model returns the losses of fit_generator over the float arrays
    utils.prepare_targets builds on the host, bit for bit (test_gpu_focal's check): the fed loop runs the same penalty
    launches between its replayed step and the optimizer"""
    from dl3_amd import utils as U
    rng = np.random.default_rng(31)
    raw = []
    for _ in range(2):
        img = rng.integers(0, 256, (B,) + SHAPE, dtype=np.uint8)
        lab = rng.integers(0, CLASSES, (B, SHAPE[0], SHAPE[1]), dtype=np.uint8)
        lab[rng.uniform(size=lab.shape) < 0.1] = 255
        raw.append((img, lab))
    fed, plain, twin = _model(decay=DECAY), _model(decay=DECAY), _model()
    got = list(fed.fit_generator(raw, steps_per_epoch=2, device_feed=True, n_classes=CLASSES))
    arrays = [(img.astype(f32),) + tuple(U.prepare_targets(lab, CLASSES)) for img, lab in raw]
    want = list(plain.fit_generator(arrays, steps_per_epoch=2))
    bare = list(twin.fit_generator(arrays, steps_per_epoch=2))
    assert len(got) == 2 and np.isfinite(got).all()
    assert [float(v) for v in got] == [float(v) for v in want], (got, want)
    assert got[0] > bare[0] + 1.0 and fed._active.l2 and fed._active.iteration == 2      # (the penalty is about 7.2)
