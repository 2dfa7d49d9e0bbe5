"""The focal loss on the device (csrc/losstail.hip): the four forms through the C ABI against the float64
oracle under the project's yardstick (the fold form against today's fold kernel: both use __expf), the cross-entropy
half bit for bit against today's loss kernels, the refusals, and the training step at model level — loss against the
oracle on Engine.logits() under hipGraph replay, the plan, gamma = 0, evaluation untouched, a world of one, the device
feed."""
import os

import numpy as np
import pytest
import torch

from oracle import dl3_oracle as O
from tests import focal_oracle as F
from tests import ops_oracle as OO
from tests.gpu_util import Guarded, assert_bands, assert_untouched, call, dev, host, stream
from tests.test_gpu_mine import _shuffle_cases

pytestmark = pytest.mark.gpu

f32 = np.float32
ENTRY = {"plain": "dl3_focal_xent", "bilinear": "dl3_upsample_focal_xent", "bilinear_fold": "dl3_upsample_focal_xent_fold",
         "shuffle": "dl3_shuffle_focal_xent"}
TODAY = {"plain": "dl3_softmax_xent", "bilinear": "dl3_upsample_softmax_xent",
         "bilinear_fold": "dl3_upsample_softmax_xent_fold", "shuffle": "dl3_shuffle_softmax_xent"}


def _lib():
    from dl3_amd import capi
    return capi.lib()


class _Case:
    """one case of one form on the device: inputs, and guarded outputs for the gradient and the loss partials.
    form 'plain': x [B,1,HW,C]; 'bilinear' / 'bilinear_fold': x [N,Hi,Wi,C], shape (Ho, Wo); 'shuffle': x [N,H,W,C*r*r],
    shape r"""

    def __init__(self, form, x, shape, t, w, C):
        self.form, self.C, self.xs, self.shape = form, C, x.shape, shape
        L = _lib()
        N = x.shape[0]
        if form == "plain":
            M = t.size
            self.dims, self.ng, self.P = (M, C), M * C, L.dl3_rows_partials(M)
        elif form in ("bilinear", "bilinear_fold"):
            Hi, Wi, (Ho, Wo) = x.shape[1], x.shape[2], shape
            self.dims = (N, Hi, Wi, Ho, Wo, C)
            fold = form == "bilinear_fold"
            self.ng = N * Ho * (Wi if fold else Wo) * C
            self.P = L.dl3_xent_fold_partials(N, Ho) if fold else L.dl3_rows_partials(N * Ho * Wo)
        else:
            self.dims = (N, x.shape[1], x.shape[2], C, shape)
            self.ng, self.P = x.size, L.dl3_shuffle_xent_partials(N, x.shape[1], x.shape[2], C, shape)
        assert self.P >= 1
        self.x, self.t = dev(x), dev(t)
        self.w = dev(w) if w is not None else None
        self.wp = self.w.data_ptr() if w is not None else None
        self.nnz = dev(np.array([t.size if w is None else int((w != 0).sum()), 0, 0, 0], f32))
        self.pool = []
        self.g = Guarded(self.pool, "gradient", self.ng)
        self.part = Guarded(self.pool, "loss partials", self.P)
        self.loss = Guarded(self.pool, "loss", 1)

    def _out(self):
        call("dl3_reduce_partials", self.part.p, self.P, 1, self.loss.p)
        assert_bands(self.pool)
        return dict(g=host(self.g.t).copy(), part=host(self.part.t).copy(), loss=float(host(self.loss.t)[0]))

    def focal(self, gamma, alpha):
        for g in self.pool:
            g.t.fill_(float("nan"))
        a = dev(alpha) if alpha is not None else None
        call(ENTRY[self.form], self.x.data_ptr(), self.t.data_ptr(), self.wp, self.nnz.data_ptr(),
             a.data_ptr() if a is not None else None, float(gamma), self.g.p, self.part.p, *self.dims)
        return self._out()

    def today(self):
        for g in self.pool:
            g.t.fill_(float("nan"))
        probs = (None,) if self.form in ("plain", "bilinear") else ()
        call(TODAY[self.form], self.x.data_ptr(), self.t.data_ptr(), self.wp, self.nnz.data_ptr(), *probs, self.g.p,
             self.part.p, *self.dims)
        return self._out()

    def full(self, g):
        """the device gradient at the full resolution [B,HW,C] (the shuffle form writes u's layout)"""
        if self.form == "shuffle":
            g = O.phase_shift(g.reshape(self.xs), self.shape)
        return g.reshape(self.xs[0], -1, self.C)


def _targets(rng, B, HW, C, void=False):
    """labels uniform in 0..C (C = void), weights in [0.5, 2) with a fifth of them zero; void: every label void"""
    t = rng.integers(0, C + 1, (B, HW)).astype(f32)
    if void:
        t[:] = C
    w = (rng.uniform(0.5, 2.0, (B, HW)) * (rng.random((B, HW)) > 0.2)).astype(f32)
    return t, w


def _plain_cases():
    for B, HW in ((1, 1), (2, 257), (3, 4099)):
        for C in (2, 21, 32):
            yield "plain", (B, 1, HW, C), None, C, False
    yield "plain", (2, 1, 257, 21), None, 21, True


def _bilinear_cases():
    yield "bilinear", (2, 5, 5, 21), (33, 33), 21, False
    yield "bilinear", (1, 9, 7, 3), (65, 49), 3, False
    yield "bilinear", (2, 5, 5, 21), (33, 33), 21, True


def _shuffle_all():
    for form, xs, r, C in _shuffle_cases():
        yield form, xs, r, C, False
    yield "shuffle", (1, 8, 8, 21 * 16), 4, 21, True


def _fold_cases():
    # the two shapes of test_gpu_ops_edges::test_upsample_softmax_xent_fold_capped_rows: without prefetch and second trips
    # of the workgroups (4200 rows > 4096); the prefetching variant
    yield "bilinear_fold", (70, 2, 2, 3), (60, 4), 3, False
    yield "bilinear_fold", (3, 3, 5, 4), (110, 101), 4, False
    yield "bilinear_fold", (2, 5, 5, 21), (33, 33), 21, False


def _hw(form, xs, shape):
    if form == "plain":
        return xs[1] * xs[2]
    if form == "shuffle":
        return xs[1] * shape * xs[2] * shape
    return shape[0] * shape[1]


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("cases", [_plain_cases, _bilinear_cases, _shuffle_all], ids=["plain", "bilinear", "shuffle"])
def test_forms_against_the_float64_oracle(cases):
    """every shape of one form, gamma in {0.5, 2}, alpha null and uniform in [0.5, 2], with and without weights, one
    all-void case: loss and dlogits at most 2x as far from the float64 oracle as the float32 yardstick is (the largest
    distance over the form's cases, per quantity); dlogits exactly zero where w = 0 or the label is void; everything
    finite; two runs bit-identical; guard bands untouched.  Measured ratios (MI355X): DESIGN.md §18."""
    rng = np.random.default_rng(29)
    qs = ("loss", "dlogits")
    dd, od = dict.fromkeys(qs, 0.0), dict.fromkeys(qs, 0.0)
    form = None
    for form, xs, shape, C, void in cases():
        x = (rng.standard_normal(xs) * 3).astype(f32)
        B, HW = xs[0], _hw(form, xs, shape)
        t, w = _targets(rng, B, HW, C, void)
        alpha = rng.uniform(0.5, 2.0, C).astype(f32)
        for weights in (w, None):
            ch = _Case(form, x, shape, t, weights, C)
            for gamma in (0.5, 2.0):
                for al in (None, alpha):
                    d = ch.focal(gamma, al)
                    r64 = F.evaluate(form, x, shape, t, weights, gamma, al, np.float64)
                    r32 = F.evaluate(form, x, shape, t, weights, gamma, al, np.float32)
                    what = (form, xs, "weighted" if weights is not None else "plain", gamma, "alpha" if al is not None else "",
                            "void" if void else "")
                    g = ch.full(d["g"])
                    assert np.isfinite(g).all() and np.isfinite(d["part"]).all() and np.isfinite(d["loss"]), what
                    zero = (t >= C) | ((weights == 0) if weights is not None else False)
                    assert (g[zero] == 0).all(), (what, "dlogits == 0 where w = 0 or the label is void")
                    if void:
                        assert d["loss"] == 0.0 and (g == 0).all()
                    elif not zero.all():
                        assert np.abs(g[~zero]).max() > 0
                    got = dict(loss=d["loss"], dlogits=g)
                    for q in qs:
                        a, b = _dist(got[q], r64[q]), _dist(r32[q], r64[q])
                        print("%-8s %-18s %-8s gamma %.1f %-5s %-4s %-7s device %.3e, float32 oracle %.3e" % (what + (q, a, b)))
                        dd[q], od[q] = max(dd[q], a), max(od[q], b)
                    e = ch.focal(gamma, al)
                    assert np.array_equal(d["g"].view(np.uint32), e["g"].view(np.uint32)), (what, "two runs differ")
                    assert np.array_equal(d["part"].view(np.uint32), e["part"].view(np.uint32)) and d["loss"] == e["loss"]
    for q in qs:
        print("focal %s %s: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2)" % (
            form, q, dd[q], od[q], dd[q] / od[q] if od[q] else 0.0))
    for q in qs:
        assert dd[q] <= 2 * od[q], (form, q, dd[q], od[q])


@pytest.mark.parametrize("case", list(_fold_cases()), ids=["capped-rows", "prefetch", "33x33x21"])
def test_fold_form_against_todays_fold_kernel(case):
    """this kernel family uses __expf, so it is measured against the parent's kernel: on the same inputs d_focal (the focal
    xfold, gamma = 2, random alpha, against the float64 focal gradient folded with ops_oracle.resize_bwd_cols) is at most
    2 d_ce (today's dl3_upsample_softmax_xent_fold against the float64 cross-entropy gradient folded the same way), each
    divided by its reference's largest absolute value; then dl3_resize_bilinear_bwd_rows on it is finite and bit-identical
    over two runs.  Measured ratios (MI355X): DESIGN.md §18."""
    form, xs, shape, C, _ = case
    rng = np.random.default_rng(31)
    x = (rng.standard_normal(xs) * 3).astype(f32)
    N, Hi, Wi, (Ho, Wo) = xs[0], xs[1], xs[2], shape
    t, w = _targets(rng, N, Ho * Wo, C)
    alpha = rng.uniform(0.5, 2.0, C).astype(f32)
    ch = _Case(form, x, shape, t, w, C)
    want_pref = (Wi * C) % 4 == 0 and (Wo * C) % 4 == 0
    assert want_pref == (xs == (3, 3, 5, 4)), "the shapes take the variants the test says"

    def folded(gamma, al):
        r = F.evaluate("bilinear", x, shape, t, w, gamma, al, np.float64)
        return OO.resize_bwd_cols(r["dlogits"].reshape(N, Ho, Wo, C), Wi, Wo)[0], r["loss"]

    d = ch.focal(2.0, alpha)
    e = ch.focal(2.0, alpha)
    assert np.isfinite(d["g"]).all() and np.array_equal(d["g"].view(np.uint32), e["g"].view(np.uint32)) and d["loss"] == e["loss"]
    assert np.array_equal(d["part"].view(np.uint32), e["part"].view(np.uint32))
    ref, loss = folded(2.0, alpha)
    d_focal = _dist(d["g"].reshape(ref.shape), ref) / np.abs(ref).max()
    c = ch.today()
    ref_ce, loss_ce = folded(0.0, None)
    d_ce = _dist(c["g"].reshape(ref_ce.shape), ref_ce) / np.abs(ref_ce).max()
    print("fold %s -> %s: d_focal %.3e, d_ce %.3e, ratio %.2f (bound 2); loss %.7f against %.7f, today's %.7f against %.7f" % (
        xs, shape, d_focal, d_ce, d_focal / d_ce, d["loss"], loss, c["loss"], loss_ce))
    assert d_focal <= 2 * d_ce
    # the loss: the relative distance of today's kernel from its own oracle, doubled, and no less than 2e-6 (the bound of
    # the comparison of two float32 sums elsewhere in this file)
    assert abs(d["loss"] - loss) <= max(2 * abs(c["loss"] - loss_ce) / loss_ce, 2e-6) * loss
    # the y half on the folded rows
    ch.focal(2.0, alpha)
    outs = []
    for _ in range(2):
        pool = []
        dx = Guarded(pool, "dx", N * Hi * Wi * C)
        call("dl3_resize_bilinear_bwd_rows", ch.g.p, dx.p, C, N, Hi, Wi, Ho, C, 0)
        assert_bands(pool)
        outs.append(host(dx.t).copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def _pin_cases():
    for cases in (_plain_cases, _bilinear_cases, _shuffle_all, _fold_cases):
        for c in cases():
            yield c


def test_gamma_zero_is_todays_kernel_bit_for_bit():
    """gamma = 0 and alpha null: the gradient of each of the four forms equals today's counterpart bit for bit (compared as
    uint32) and the loss partials' sum agrees to 2e-6 relative; alpha == 1 as an array equals alpha null bit for bit"""
    rng = np.random.default_rng(37)
    for form, xs, shape, C, void in _pin_cases():
        x = (rng.standard_normal(xs) * 3).astype(f32)
        t, w = _targets(rng, xs[0], _hw(form, xs, shape), C, void)
        for weights in (w, None):
            ch = _Case(form, x, shape, t, weights, C)
            a = ch.focal(0.0, None)
            b = ch.today()
            what = (form, xs, shape, "weighted" if weights is not None else "plain")
            assert np.array_equal(a["g"].view(np.uint32), b["g"].view(np.uint32)), (what, "the cross-entropy half differs")
            sa, sb = a["part"].astype(np.float64).sum(), b["part"].astype(np.float64).sum()
            assert abs(sa - sb) <= 2e-6 * max(abs(sb), 1.0), (what, sa, sb)
            one = ch.focal(0.0, np.ones(C, f32))
            assert np.array_equal(one["g"].view(np.uint32), a["g"].view(np.uint32)), (what, "alpha == 1 differs from null")
            assert np.array_equal(one["part"].view(np.uint32), a["part"].view(np.uint32))
            for gamma in (2.0, 0.5):
                two, ones = ch.focal(gamma, None), ch.focal(gamma, np.ones(C, f32))
                assert np.array_equal(two["g"].view(np.uint32), ones["g"].view(np.uint32))
                assert np.array_equal(two["part"].view(np.uint32), ones["part"].view(np.uint32))


def test_more_than_32_classes_and_a_bad_gamma_are_refused():
    L = _lib()
    s = stream()
    x, t = np.zeros((1, 2, 2, 33 * 4), f32), np.zeros((1, 16), f32)
    dims = {"plain": lambda C: (16, C), "bilinear": lambda C: (1, 2, 2, 4, 4, C), "bilinear_fold": lambda C: (1, 2, 2, 4, 4, C),
            "shuffle": lambda C: (1, 2, 2, C, 2)}
    xd, td = dev(x), dev(t)
    nnz = dev(np.array([16, 0, 0, 0], f32))
    for form, name in ENTRY.items():
        pool = []
        g, part = Guarded(pool, "gradient", 16 * 33), Guarded(pool, "loss partials", 64)
        fn = getattr(L, name)
        assert fn(xd.data_ptr(), td.data_ptr(), None, nnz.data_ptr(), None, 2.0, g.p, part.p, *dims[form](33), s) == -4, form
        for gamma in (-1.0, float("nan"), float("inf")):
            assert fn(xd.data_ptr(), td.data_ptr(), None, nnz.data_ptr(), None, gamma, g.p, part.p, *dims[form](3), s) == -1, (
                form, gamma)
        torch.cuda.synchronize()
        assert_untouched(pool)
        assert fn(xd.data_ptr(), td.data_ptr(), None, nnz.data_ptr(), None, 2.0, g.p, part.p, *dims[form](3), s) == 0, form
        assert_bands(pool)


# -------------------------------------------------------------------------------------------------------- model level
SHAPE, CLASSES, B = (64, 64, 3), 3, 2
GAMMA, ALPHA = 2.0, (0.5, 1.0, 2.0)


def _batches(n, b=B, seed=7):
    """different labels every step"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x = rng.integers(0, 256, (b,) + SHAPE).astype(f32)
        y = rng.integers(0, CLASSES + 1, (b, SHAPE[0] * SHAPE[1], 1)).astype(f32)
        sw = ((y[..., 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2]) * (rng.random(y.shape[:2]) > 0.1)).astype(f32)
        out.append((x, y, sw))
    return out


def _model(head, loss, classes=CLASSES):
    from tests.test_gpu_model import _build, _load
    model, params = _build("mobilenetv2", SHAPE, classes, head)
    _load(model, params)
    model.compile(optimizer=None, loss=loss)
    return model


def _weights(model):
    eng = model._active
    torch.cuda.synchronize()
    return [a.cpu().numpy().copy() for a in (eng.params, eng.state, eng.adam_m, eng.adam_v)]


def _names(eng):
    return [r[0] for r in eng.ops_fwd], [r[0] for r in eng.ops_bwd]


@pytest.mark.parametrize("head", ["deeplab", "original", "subpixel"])
def test_step_follows_the_oracle_under_graph_replay(head):
    """three steps with new labels each — eager, capture, replay: the returned loss against the oracle's evaluation of
    Engine.logits() under the yardstick; the plan holds exactly one FOCAL_OPS launch and none of today's loss family: the
    fold entry with dl3_resize_bilinear_bwd_rows on the bilinear heads, the shuffle entry without dl3_phase_shift in the
    backward list on the Subpixel head"""
    from dl3_amd import head as H
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    model = _model(head, U.sparse_focal_crossentropy(GAMMA, ALPHA))
    dd = od = 0.0
    losses = []
    for s, (x, y, sw) in enumerate(_batches(3)):
        loss = model.train_on_batch(x, y, sw)
        eng = model._active
        assert eng.focal == (GAMMA, ALPHA) and eng.mining is None and eng.jaccard is None
        z = eng.logits()
        r64 = F.evaluate("plain", z, None, y, sw, GAMMA, ALPHA, np.float64)
        r32 = F.evaluate("plain", z, None, y, sw, GAMMA, ALPHA, np.float32)
        a, b = abs(loss - r64["loss"]), abs(r32["loss"] - r64["loss"])
        print("%s step %d loss %.9f, oracle %.9f: device %.3e, float32 oracle %.3e" % (head, s, loss, r64["loss"], a, b))
        dd, od = max(dd, a), max(od, b)
        losses.append(loss)
    eng = model._active
    assert eng.graph is not None, "the step was never captured"
    assert len(set(losses)) == 3 and np.isfinite(losses).all()
    fwd, bwd = _names(eng)
    today = [e[0] for e in H.KERNELS["loss"].values()]
    assert sum(n in Engine.FOCAL_OPS for n in fwd + bwd) == 1 and not any(n in today for n in fwd + bwd)
    assert fwd.count("dl3_count_nonzero") == 1 and fwd.count("dl3_reduce_partials") >= 1
    if head == "subpixel":
        assert "dl3_shuffle_focal_xent" in fwd and "dl3_phase_shift" not in bwd
    else:
        assert "dl3_upsample_focal_xent_fold" in fwd and "dl3_resize_bilinear_bwd_rows" in bwd
    print("%s loss: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2)" % (head, dd, od, dd / od if od else 0.0))
    assert dd <= 2 * od


def test_off_is_the_plain_loss_on_changes_the_step_and_evaluation_is_untouched():
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    off = _model("deeplab", U.sparse_focal_crossentropy(0.0, None))
    on = _model("deeplab", U.sparse_focal_crossentropy(2.0))
    twin = _model("deeplab", U.sparse_crossentropy_ignoring_last_label)
    (x, y, sw), = _batches(1, b=4, seed=9)
    ra = on.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    rb = twin.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    assert ra == rb and np.isfinite(ra).all()
    assert np.array_equal(on.predict(x[:2]), twin.predict(x[:2]))
    for s, (x, y, sw) in enumerate(_batches(3)):
        la, lb, lc = off.train_on_batch(x, y, sw), twin.train_on_batch(x, y, sw), on.train_on_batch(x, y, sw)
        assert la == lb
        if s == 0:
            assert lc != lb and 0 < lc < lb      # (1 - q)^2 < 1 at every pixel
    for wa, wb, wc in zip(_weights(off), _weights(twin), _weights(on)):
        assert np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
    assert not np.array_equal(_weights(on)[0], _weights(twin)[0])
    ea, eb = off._active, twin._active
    assert ea.focal is None and _names(ea) == _names(eb)
    assert not any(n in Engine.FOCAL_OPS for n in _names(ea)[0] + _names(ea)[1])


def test_refusals_at_the_engine():
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    model = _model("deeplab", U.sparse_focal_crossentropy(GAMMA, ALPHA))
    with pytest.raises(ValueError, match="separate losses"):
        Engine(model, batch=1, training=True, focal=(GAMMA, ALPHA), mining=(0.25, 0))
    with pytest.raises(ValueError, match="separate losses"):
        Engine(model, batch=1, training=True, focal=(GAMMA, ALPHA), jaccard=0.5)
    with pytest.raises(ValueError, match="class weights"):
        Engine(model, batch=1, training=True, focal=(GAMMA, (1.0, 2.0)))
    wide = _model("deeplab", U.sparse_focal_crossentropy(GAMMA), classes=33)
    with pytest.raises(ValueError, match="32 classes"):
        wide.train_on_batch(np.zeros((1,) + SHAPE, f32), np.zeros((1, SHAPE[0] * SHAPE[1], 1), f32))


def test_world_of_one_focal_step():
    """Model.distribute() with an RCCL communicator of one rank and the focal loss: bit for bit the single-process
    data-parallel engine (external_nnz, no communicator) over two steps — losses, weights, optimizer state; against the
    plain single-process engine the first loss agrees to fp32 rounding (the data-parallel engine scales by c0 / count)"""
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    from dl3_amd.parallel import DataParallel
    assert int(os.environ.get("WORLD_SIZE", "1")) == 1
    batches = _batches(2)

    def run(mode):
        model = _model("deeplab", U.sparse_focal_crossentropy(GAMMA, ALPHA))
        dp, kw = None, dict(dropout=False)
        if mode == "rccl":
            dp = DataParallel().attach_single_rank_rccl()
            assert dp.rccl_ranks() == 1
            model.distribute(dp)
        elif mode == "tail":
            kw["external_nnz"] = True
        losses = [model.train_on_batch(x, y, sw, **kw) for x, y, sw in batches]
        eng = model._active
        assert eng.external_nnz == (mode != "plain") and eng.focal == (GAMMA, ALPHA)
        assert sum(n in Engine.FOCAL_OPS for n in _names(eng)[0]) == 1
        w = _weights(model)
        if dp is not None:
            dp.close()
        return losses, w

    lp, _ = run("plain")
    lt, wt = run("tail")
    lr, wr = run("rccl")
    assert lt == lr and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(wt, wr))
    assert abs(lp[0] - lr[0]) < 2e-6 * abs(lp[0])


def test_device_feed_equals_the_host_array_path():
    """fit_generator(device_feed=True) over 5 samples at batch size 2 — batches of 2, 2 and 1 (the feed takes one batch size
    per call, so the single image is a second call) — returns the losses of fit_generator over the float arrays
    utils.prepare_targets builds on the host, bit for bit"""
    from dl3_amd import utils as U
    rng = np.random.default_rng(23)
    raw = []
    for b in (2, 2, 1):
        img = rng.integers(0, 256, (b,) + SHAPE, dtype=np.uint8)
        lab = rng.integers(0, CLASSES, (b, SHAPE[0], SHAPE[1]), dtype=np.uint8)
        lab[rng.uniform(size=lab.shape) < 0.1] = 255
        raw.append((img, lab))
    a = _model("deeplab", U.sparse_focal_crossentropy(GAMMA, ALPHA))
    got = list(a.fit_generator(raw[:2], steps_per_epoch=2, device_feed=True, n_classes=CLASSES))
    got += list(a.fit_generator(raw[2:], steps_per_epoch=1, device_feed=True, n_classes=CLASSES))
    b = _model("deeplab", U.sparse_focal_crossentropy(GAMMA, ALPHA))
    arrays = [(img.astype(f32),) + tuple(U.prepare_targets(lab, CLASSES)) for img, lab in raw]
    want = list(b.fit_generator(arrays[:2], steps_per_epoch=2)) + list(b.fit_generator(arrays[2:], steps_per_epoch=1))
    assert len(got) == 3 and np.isfinite(got).all()
    assert [float(v) for v in got] == [float(v) for v in want], (got, want)
    engs = {e.B: e for e in a._engines.values() if e.training}
    assert sorted(engs) == [1, 2] and all(e.focal == (GAMMA, ALPHA) for e in engs.values()) and engs[1].iteration == 3
