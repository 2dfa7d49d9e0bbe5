"""Hard-example mining on the device (csrc/mine.hip): the per-pixel loss of the three training forms
through the C ABI against the float64 oracle under the project's yardstick, the radix selection bit for bit against
numpy, and the mined training step at model level — schedule under hipGraph replay, the twin model stepped on w', the
ramp across engines, mining off, evaluation untouched, a world of one."""
import os

import numpy as np
import pytest
import torch

from tests import mine_oracle as M
from tests.gpu_util import call, dev, empty, host

pytestmark = pytest.mark.gpu

f32 = np.float32


# ---------------------------------------------------------------------------------------------------- per-pixel loss
def _targets(rng, shape, C):
    """labels 0..C (C = void, about one in C + 1) and weights in [0.5, 2) with a fifth of them zero"""
    t = rng.integers(0, C + 1, shape).astype(f32)
    w = (rng.uniform(0.5, 2.0, shape) * (rng.random(shape) > 0.2)).astype(f32)
    return t, w


def _plain_cases():
    for M_ in (1, 257, 4099):
        for C in (2, 21, 32):
            yield "plain", (1, 1, M_, C), None, C


def _bilinear_cases():
    yield "bilinear", (2, 5, 5, 21), (33, 33), 21
    yield "bilinear", (1, 9, 7, 3), (65, 49), 3


def _shuffle_cases():
    for r in (4, 8):
        for C in (3, 21):
            yield "shuffle", (1, 8, 8, C * r * r), r, C
    yield "shuffle", (2, 3, 13, 21 * 16), 4, 21   # an odd width; the tile (34 pixels at C = 21, r = 4) still holds the row
    # widths that are no multiple of the tile: more than one tile per row and a ragged last one
    yield "shuffle", (1, 2, 13, 21 * 64), 8, 21   # tile of 9 pixels: tiles of 9 and 4
    yield "shuffle", (2, 2, 40, 21 * 16), 4, 21   # tile of 34 pixels: tiles of 34 and 6


def _device_v(form, x, shape, t, w, C):
    xd, td = dev(x), dev(t)
    wd = dev(w) if w is not None else None
    wp = wd.data_ptr() if wd is not None else None
    v = empty(t.size)
    if form == "plain":
        call("dl3_pixel_xent_plain", xd.data_ptr(), td.data_ptr(), wp, v.data_ptr(), t.size, C)
    elif form == "bilinear":
        N, Hi, Wi, _ = x.shape
        call("dl3_pixel_xent_bilinear", xd.data_ptr(), td.data_ptr(), wp, v.data_ptr(), N, Hi, Wi, shape[0], shape[1], C)
    else:
        N, H, W, _ = x.shape
        call("dl3_pixel_xent_shuffle", xd.data_ptr(), td.data_ptr(), wp, v.data_ptr(), N, H, W, C, shape)
    return host(v)


def _yardstick(vd, v64, v32):
    """(device distance, float32-oracle distance): the largest per-pixel distance from the float64 oracle"""
    return float(np.abs(vd.astype(np.float64) - v64).max()), float(np.abs(v32.astype(np.float64) - v64).max())


@pytest.mark.parametrize("cases", [_plain_cases, _bilinear_cases, _shuffle_cases], ids=["plain", "bilinear", "shuffle"])
def test_pixel_loss_against_the_float64_oracle(cases):
    """v of one form over all its shapes, with and without weights: v == 0 exactly where w == 0 or the label is void
    (and nowhere else), and the form's largest per-pixel distance from the float64 oracle is at most 2x the float32
    oracle's own.  Measured ratios (MI355X): see DESIGN.md §15."""
    rng = np.random.default_rng(11)
    dd = od = 0.0
    form = None
    for form, xs, shape, C in cases():
        x = (rng.standard_normal(xs) * 3).astype(f32)
        z = M.E.full_logits(form, x, shape)
        t, w = _targets(rng, z.shape[:-1], C)
        for weights in (w, None):
            vd = _device_v(form, x, shape, t, weights, C)
            assert vd.shape == (t.size,) and np.isfinite(vd).all() and (vd >= 0).all()
            zero = (t.reshape(-1) >= C) | ((weights.reshape(-1) == 0) if weights is not None else False)
            assert np.array_equal(vd == 0, zero), (form, xs, "v == 0 exactly where w == 0 or the label is void")
            assert not np.signbit(vd).any()
            v64 = M.pixel_v(form, x, shape, t, weights, np.float64)
            v32 = M.pixel_v(form, x, shape, t, weights, np.float32)
            d, o = _yardstick(vd, v64, v32)
            print("pixel loss %-8s %-18s %s: device %.3e, float32 oracle %.3e" % (
                form, xs, "weighted" if weights is not None else "plain   ", d, o))
            dd, od = max(dd, d), max(od, o)
    print("pixel loss %s: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2)" % (form, dd, od, dd / od))
    assert dd <= 2 * od


# ---------------------------------------------------------------------------------------------------------- selection
SIZES = (1, 63, 257, 65539, 1048583)


def _values(kind, N, rng):
    if kind == "exponential":
        return rng.exponential(1.0, N).astype(f32)
    if kind == "quantised":
        return (rng.integers(0, 7, N) * f32(0.375)).astype(f32)          # 7 distinct values, 0 among them
    if kind == "zeros":
        return np.zeros(N, f32)
    if kind == "equal":
        return np.full(N, f32(1.25))
    if kind == "half_zeros":
        return (rng.exponential(1.0, N) * (rng.random(N) < 0.5)).astype(f32)
    if kind == "low_byte":                                               # equal in the upper 24 bits
        return (np.uint32(0x3F8A5C00) | rng.integers(0, 256, N).astype(np.uint32)).view(f32)
    if kind == "inf_denormal":
        v = rng.exponential(1.0, N).astype(f32)
        v[rng.random(N) < 0.3] = f32(np.inf)
        den = rng.random(N) < 0.3
        v[den] = rng.integers(1, 1 << 23, int(den.sum())).astype(np.uint32).view(f32)   # denormals
        return v
    raise ValueError(kind)


KINDS = ("exponential", "quantised", "zeros", "equal", "half_zeros", "low_byte", "inf_denormal")


def _p_for(k, N):
    """a float32 p in (0, 1] with trunc(fl(p * fl32(N))) == k (S = 0: pct = p)"""
    if k >= N:
        return 1.0
    p = f32((k + 0.5) / N)
    for _ in range(64):
        got = M.schedule_k(p, 0, 0, N)
        if got == k:
            return float(p)
        p = np.nextafter(p, f32(1) if got < k else f32(0))
    raise AssertionError("no float32 p gives k = %d of %d" % (k, N))


class _Selector:
    def __init__(self, v, w):
        self.N = v.size
        self.v, self.w = dev(v), (dev(w) if w is not None else None)
        nws = int(M_lib().dl3_topk_workspace_bytes(self.N))
        assert nws > 0
        self.nws = nws
        self.ws = torch.full((nws // 4 + 2,), -1, dtype=torch.int32, device="cuda")   # the call zeroes what it uses
        self.k = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        self.tau, self.nnz, self.wout = empty(4), empty(4), empty(self.N)
        self.step = torch.zeros(1, dtype=torch.int64, device="cuda")

    def run(self, p, S, s=None):
        if s is not None:
            self.step.fill_(int(s))
        self.wout.fill_(float("nan"))
        call("dl3_topk_threshold", self.v.data_ptr(), self.N, float(p), int(S), self.step.data_ptr() if s is not None else None,
             self.ws.data_ptr(), self.nws, self.k.data_ptr(), self.tau.data_ptr())
        call("dl3_mine_weights", self.v.data_ptr(), self.w.data_ptr() if self.w is not None else None, self.tau.data_ptr(),
             self.k.data_ptr(), self.wout.data_ptr(), self.nnz.data_ptr(), self.ws.data_ptr(), self.N)
        torch.cuda.synchronize()
        assert int(self.ws[-1].item()) == -1 and int(self.ws[-2].item()) == -1, "wrote past the workspace"
        return int(self.k[0].item()), host(self.tau)[:1].copy(), host(self.wout).copy(), float(self.nnz[0].item())


def M_lib():
    from dl3_amd import capi
    return capi.lib()


def _check(sel, v, w, p, S, s, what):
    k, tau, wout, nnz = sel.run(p, S, s)
    ko, tauo, wo, no = M.mine(v, w, p, S, 0 if s is None else s)
    assert k == ko, (what, "k", k, ko)
    assert tau.view(np.uint32)[0] == np.asarray([tauo], f32).view(np.uint32)[0], (what, "tau", tau, tauo)
    assert nnz == float(no), (what, "n'", nnz, no)
    assert np.array_equal(wout.view(np.uint32), wo.view(np.uint32)), (what, "w'", int((wout != wo).sum()))
    return k, tau, wout, nnz


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_selection_equals_numpy_bit_for_bit(N, kind):
    """tau, k, n' and every w' against np.partition on the same v, for k in {0, 1, 2, N/2, count(v > 0),
    count(v > 0) + 1, N} (set through p with S = 0); two runs are identical"""
    rng = np.random.default_rng(N * 31 + KINDS.index(kind))
    v = _values(kind, N, rng)
    w = rng.uniform(0.5, 2.0, N).astype(f32)
    sel = _Selector(v, w)
    pos = int((v > 0).sum())
    ks = sorted({min(N, max(0, k)) for k in (0, 1, 2, N // 2, pos, pos + 1, N)})
    for k in ks:
        p = _p_for(k, N)
        assert M.schedule_k(p, 0, 0, N) == k
        a = _check(sel, v, w, p, 0, None, (N, kind, k))
        b = sel.run(p, 0, None)
        assert a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), "two runs differ"


def test_selection_without_weights_and_the_ramp():
    """a null weights pointer means w = 1; the schedule reads the device counter: s in {0, S/2, S, S + 7}, and a case
    in which the float32 roundings of the schedule decide k (tests/test_mine_host.py)"""
    N = 65539
    rng = np.random.default_rng(5)
    v = _values("half_zeros", N, rng)
    sel = _Selector(v, None)
    S = 10
    seen = []
    for s in (0, S // 2, S, S + 7):
        seen.append(_check(sel, v, None, 0.25, S, s, ("ramp", s))[0])
    assert seen == [N, M.schedule_k(0.625, 0, 0, N), M.schedule_k(0.25, 0, 0, N), M.schedule_k(0.25, 0, 0, N)]
    assert seen[0] > seen[1] > seen[2]
    v2 = _values("exponential", 1000, rng)
    sel2 = _Selector(v2, None)
    assert _check(sel2, v2, None, 0.1, 3, 2, "float32 roundings")[0] == 399


# -------------------------------------------------------------------------------------------------------- model level
SHAPE, CLASSES, B = (64, 64, 3), 3, 2
P, S = 0.25, 4


def _batches(n, b=B, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x = rng.integers(0, 256, (b,) + SHAPE).astype(f32)
        y = rng.integers(0, CLASSES + 1, (b, SHAPE[0] * SHAPE[1], 1)).astype(f32)
        sw = ((y[..., 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2]) * (rng.random(y.shape[:2]) > 0.1)).astype(f32)
        out.append((x, y, sw))
    return out


def _model(backbone, head, loss):
    from tests.test_gpu_model import _build, _load
    model, params = _build(backbone, SHAPE, CLASSES, head)
    _load(model, params)
    model.compile(optimizer=None, loss=loss)
    return model


def _weights(model):
    eng = model._active
    torch.cuda.synchronize()
    return eng.params.cpu().numpy().copy(), eng.state.cpu().numpy().copy()


@pytest.mark.parametrize("backbone,head", [("mobilenetv2", "deeplab"), ("mobilenetv2", "original"),
                                           ("mobilenetv2", "subpixel"), ("xception", "original")])
def test_mined_step_follows_the_oracle_and_equals_the_twin_on_mined_weights(backbone, head):
    """four steps with p = .25, S = 4 — eager, capture, two replays: k and n' follow the oracle's schedule at every step;
    the recorded mask is the oracle's selection of the recorded v bit for bit; v agrees with the oracle's evaluation of
    Engine.logits() under the yardstick; loss and updated weights equal, bit for bit, a twin model stepped without mining
    on sample_weight = w' (same initial weights, seed and step, hence the same dropout mask)."""
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    mined = _model(backbone, head, U.sparse_crossentropy_top_k(P, S))
    twin = _model(backbone, head, U.sparse_crossentropy_ignoring_last_label)
    N = B * SHAPE[0] * SHAPE[1]
    ks, dd, od = [], 0.0, 0.0
    for s, (x, y, sw) in enumerate(_batches(4)):
        loss = mined.train_on_batch(x, y, sw)
        eng = mined._active
        assert eng.mining == (P, S)
        v, w2, tau, k, n = eng.mining_record()
        ko, tauo, wo, no = M.mine(v, sw, P, S, s)
        assert (k, n) == (ko, no), (s, k, ko, n, no)
        assert f32(tau) == tauo and np.array_equal(w2.view(np.uint32), wo.view(np.uint32))
        ks.append(k)
        # v against the oracle's evaluation of this step's logits
        z = eng.logits()
        v64 = M.pixel_v("plain", z, None, y, sw, np.float64)
        v32 = M.pixel_v("plain", z, None, y, sw, np.float32)
        d = float(np.abs(v.astype(np.float64) - v64).max())
        o = float(np.abs(v32.astype(np.float64) - v64).max())
        dd, od = max(dd, d), max(od, o)
        # the twin: today's step on the mined weights
        loss2 = twin.train_on_batch(x, y, w2.reshape(sw.shape))
        assert loss == loss2, (s, loss, loss2)
        (pa, sa), (pb, sb) = _weights(mined), _weights(twin)
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb), (s, "weights differ from the twin's")
    assert mined._active.graph is not None and twin._active.graph is not None, "the step was never captured"
    names = [r[0] for r in mined._active.ops_fwd]
    assert "dl3_count_nonzero" not in names and sum(n in Engine.MINING_OPS for n in names) == 3
    assert ks == [M.schedule_k(P, S, s, N) for s in range(4)] and ks[0] == N and len(set(ks)) == 4
    print("%s/%s: k %s; v device / float32-oracle distance %.3e / %.3e = %.2f" % (backbone, head, ks, dd, od, dd / od))
    assert dd <= 2 * od


def test_ramp_continues_across_engines():
    """5 samples at batch size 2 through fit_generator — batches of 2, 2 and 1, engines of B = 2 and B = 1 (Model.fit
    itself drops a ragged tail): the B = 1 engine adopts the step counter, so its k is the schedule's at s = 2, and the
    second epoch goes on at s = 3, 4, 5"""
    from dl3_amd import utils as U
    model = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_top_k(P, S))
    (x, y, sw), = _batches(1, b=5)
    gen = [(x[i:i + 2], y[i:i + 2], sw[i:i + 2]) for i in (0, 2, 4)]
    HW = SHAPE[0] * SHAPE[1]
    for epoch in range(2):
        model.fit_generator(gen, steps_per_epoch=3, epochs=1)
        engs = {e.B: e for e in model._engines.values() if e.training}
        assert sorted(engs) == [1, 2]
        s0 = 3 * epoch
        assert engs[2].mining_record()[3] == M.schedule_k(P, S, s0 + 1, 2 * HW)
        assert engs[1].mining_record()[3] == M.schedule_k(P, S, s0 + 2, HW)
        assert int(engs[1].mine_step.item()) == s0 + 3 == engs[1].iteration


def test_ramp_continues_across_a_recompile_with_the_same_optimizer():
    """compile() again with the same optimizer object keeps the optimizer's clock (graph.Model.compile) and, beside it,
    the mining step counter: the first step of the new engine mines at s = 2; a new optimizer object starts over"""
    from dl3_amd import utils as U
    from dl3_amd.optimizers import Adam
    from tests.test_gpu_model import _build, _load
    model, params = _build("mobilenetv2", SHAPE, CLASSES, "deeplab")
    _load(model, params)
    opt = Adam(lr=7e-4)
    N = B * SHAPE[0] * SHAPE[1]
    batches = _batches(4)
    model.compile(optimizer=opt, loss=U.sparse_crossentropy_top_k(P, S))
    for x, y, sw in batches[:2]:
        model.train_on_batch(x, y, sw)
    first = model._active
    model.compile(optimizer=opt, loss=U.sparse_crossentropy_top_k(P, S))
    model.train_on_batch(*batches[2])
    eng = model._active
    assert eng is not first and eng.iteration == 3 and int(eng.mine_step.item()) == 3
    assert eng.mining_record()[3] == M.schedule_k(P, S, 2, N)
    model.compile(optimizer=Adam(lr=7e-4), loss=U.sparse_crossentropy_top_k(P, S))
    model.train_on_batch(*batches[3])
    assert model._active.iteration == 1 and model._active.mining_record()[3] == N


def test_mining_off_is_the_plain_loss():
    """p = 1.0: weights and loss bit-identical to the plain loss, and no mining launch in the lowered plan"""
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    a = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_top_k(1.0, 4))
    b = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_ignoring_last_label)
    for x, y, sw in _batches(3):
        assert a.train_on_batch(x, y, sw) == b.train_on_batch(x, y, sw)
    (pa, sa), (pb, sb) = _weights(a), _weights(b)
    assert np.array_equal(pa, pb) and np.array_equal(sa, sb)
    ea, eb = a._active, b._active
    assert ea.mining is None
    assert [r[0] for r in ea.ops_fwd] == [r[0] for r in eb.ops_fwd] and [r[0] for r in ea.ops_bwd] == [r[0] for r in eb.ops_bwd]
    assert not any(r[0] in Engine.MINING_OPS for r in ea.ops_fwd + ea.ops_bwd)
    with pytest.raises(ValueError):
        ea.mining_record()


def test_evaluation_is_not_mined():
    from dl3_amd import utils as U
    a = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_top_k(P, S))
    b = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_ignoring_last_label)
    (x, y, sw), = _batches(1, b=4, seed=9)
    ra = a.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    rb = b.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    assert ra == rb and np.isfinite(ra).all()
    assert np.array_equal(a.predict(x[:2]), b.predict(x[:2]))


def test_world_of_one_mined_step():
    """Model.distribute() with an RCCL communicator of one rank, mined: each rank mines its own shard and its n' rides in
    the arena tail where count(w != 0) rides today.  Bit for bit the single-process data-parallel engine (external_nnz,
    no communicator): losses, weights and every step's record.  Against the plain single-process engine the first step's
    record — v, w', tau, k, n' — is bit-identical too (same forward pass); its loss agrees to fp32 rounding only, because
    the data-parallel engine scales by c0 / count instead of 1 / count (tests/test_gpu_parallel.py)."""
    from dl3_amd import utils as U
    from dl3_amd.parallel import DataParallel
    assert int(os.environ.get("WORLD_SIZE", "1")) == 1
    batches = _batches(4)

    def run(mode):
        model = _model("mobilenetv2", "deeplab", U.sparse_crossentropy_top_k(P, S))
        dp, kw = None, dict(dropout=False)
        if mode == "rccl":
            dp = DataParallel().attach_single_rank_rccl()
            assert dp.rccl_ranks() == 1
            model.distribute(dp)
        elif mode == "tail":
            kw["external_nnz"] = True
        losses, recs = [], []
        for x, y, sw in batches:
            losses.append(model.train_on_batch(x, y, sw, **kw))
            recs.append(model._active.mining_record())
        eng = model._active
        assert eng.graph is not None and eng.external_nnz == (mode != "plain") and eng.mining == (P, S)
        w = _weights(model)
        if dp is not None:
            dp.close()
        return losses, recs, w

    lp, rp, _ = run("plain")
    lt, rt, wt = run("tail")
    lr, rr, wr = run("rccl")
    assert lt == lr and np.array_equal(wt[0], wr[0]) and np.array_equal(wt[1], wr[1])
    for a, b in zip(rt, rr):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    a, b = rp[0], rr[0]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert abs(lp[0] - lr[0]) < 2e-6 * abs(lp[0])
    N = B * SHAPE[0] * SHAPE[1]
    assert [r[3] for r in rr] == [M.schedule_k(P, S, s, N) for s in range(4)]
