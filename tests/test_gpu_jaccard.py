"""The soft-Jaccard loss on the device (csrc/jaccard.hip): sums, coefficient table, L_J and the gradient of
both forms through the C ABI against the float64 oracle under the project's yardstick, the cross-entropy half bit for bit
against today's loss kernels, and the training step at model level — the record and the loss against the oracle on
Engine.logits() under hipGraph replay, lambda = 0, evaluation untouched, the device feed."""
import numpy as np
import pytest
import torch

from tests import jaccard_oracle as J
from tests.gpu_util import Guarded, assert_bands, call, dev, host

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -12345.0


def _lib():
    from dl3_amd import capi
    return capi.lib()


def _f64(n):
    """n doubles and two sentinels behind them"""
    t = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    t[n:] = SENTINEL
    return t


class _Chain:
    """the three launches of one case through the C ABI, and the fold of the loss partials"""

    def __init__(self, form, x, shape, t, w, C, lam):
        self.form, self.C, self.lam = form, C, float(lam)
        self.B = B = x.shape[0]
        self.HW = HW = t.size // B
        self.dimsv = (B, HW, C) if form == "plain" else (B, x.shape[1], x.shape[2], shape[0], shape[1], C)
        self.x, self.t = dev(x), dev(t)
        self.w = dev(w) if w is not None else None
        self.wp = self.w.data_ptr() if w is not None else None
        self.nnz = dev(np.array([t.size if w is None else int((w != 0).sum()), 0, 0, 0], f32))
        L = _lib()
        self.P, self.LP = L.dl3_jaccard_partials(B, HW), L.dl3_jaccard_loss_partials(B, HW)
        assert self.P >= 1 and self.LP >= B
        self.part, self.sums, self.stats = _f64(B * self.P * 3 * C), _f64(B * C * 3), _f64(4)
        self.pool = []
        self.coef = Guarded(self.pool, "coef", B * C * 2)
        self.dl = Guarded(self.pool, "dlogits", B * HW * C)
        self.lpart = Guarded(self.pool, "loss partials", self.LP + 1)
        self.loss = Guarded(self.pool, "loss", 1)

    def run(self, zero_table=False):
        for g in self.pool:
            g.t.fill_(float("nan"))
        sfx = "plain" if self.form == "plain" else "bilinear"
        call("dl3_jaccard_sums_" + sfx, self.x.data_ptr(), self.t.data_ptr(), self.wp, self.part.data_ptr(), *self.dimsv)
        call("dl3_jaccard_coef", self.part.data_ptr(), self.P, self.B, self.C, self.lam, self.sums.data_ptr(), self.coef.p,
             self.stats.data_ptr(), self.lpart.p + 4 * self.LP)
        if zero_table:
            self.coef.t.zero_()
        name = "dl3_softmax_xent_jaccard" if self.form == "plain" else "dl3_upsample_softmax_xent_jaccard"
        call(name, self.x.data_ptr(), self.t.data_ptr(), self.wp, self.nnz.data_ptr(), self.coef.p, self.lam, self.dl.p,
             self.lpart.p, *self.dimsv)
        call("dl3_reduce_partials", self.lpart.p, self.LP + 1, 1, self.loss.p)
        assert_bands(self.pool)
        for d, n in ((self.part, self.B * self.P * 3 * self.C), (self.sums, self.B * self.C * 3), (self.stats, 4)):
            assert (host(d)[n:] == SENTINEL).all(), "wrote past a double buffer"
        B, HW, C = self.B, self.HW, self.C
        lp = host(self.lpart.t).copy()
        return dict(sums=host(self.sums)[:B * C * 3].reshape(B, C, 3).copy(), coef=host(self.coef.t).reshape(B, C, 2).copy(),
                    lj=float(host(self.stats)[0]), n_legal=float(host(self.stats)[1]), lam_lj=float(host(self.stats)[2]),
                    row=float(lp[self.LP]), ce=float(lp[:self.LP].astype(np.float64).sum()),
                    dlogits=host(self.dl.t).reshape(B, HW, C).copy(), loss=float(host(self.loss.t)[0]))

    def plain_loss_gradient(self):
        """today's kernel on the same inputs: dl3_softmax_xent / dl3_upsample_softmax_xent"""
        pool = []
        g = Guarded(pool, "dlogits", self.B * self.HW * self.C)
        P = _lib().dl3_rows_partials(self.B * self.HW)
        part = Guarded(pool, "partials", P)
        if self.form == "plain":
            call("dl3_softmax_xent", self.x.data_ptr(), self.t.data_ptr(), self.wp, self.nnz.data_ptr(), None, g.p, part.p,
                 self.B * self.HW, self.C)
        else:
            call("dl3_upsample_softmax_xent", self.x.data_ptr(), self.t.data_ptr(), self.wp, self.nnz.data_ptr(), None, g.p,
                 part.p, *self.dimsv)
        assert_bands(pool)
        return host(g.t).reshape(self.B, self.HW, self.C).copy(), float(host(part.t).astype(np.float64).sum())


def _targets(rng, B, HW, C, void=False):
    """labels uniform in 0..C (C = void), a fifth of the weights zero; class C - 1 removed from every image and class 0
    from image 0 (where there is a second image); void: every label void"""
    t = rng.integers(0, C + 1, (B, HW)).astype(f32)
    t[t == C - 1] = C - 2 if C > 2 else C
    if B > 1:
        t[0][t[0] == 0] = C
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


QUANTITIES = ("sums", "coef", "lj", "dlogits")


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("cases", [_plain_cases, _bilinear_cases], ids=["plain", "bilinear"])
def test_forms_against_the_float64_oracle(cases):
    """every shape of one form, with and without weights, lambda = 0.75: Y exact; the sums, the coefficient table, L_J
    and dlogits at most 2x as far from the float64 oracle as the float32 yardstick is (the largest distance over the form's
    cases, per quantity); dlogits exactly zero where u = 0 and the cross-entropy half is zero too; lambda * L_J rides in
    the extra partial row and in the folded loss; with an all-zero table dlogits is today's kernel's bit for bit; two
    runs are bit-identical.  Measured ratios (MI355X): DESIGN.md §16."""
    rng = np.random.default_rng(17)
    lam = 0.75
    dd, od = dict.fromkeys(QUANTITIES, 0.0), dict.fromkeys(QUANTITIES, 0.0)
    form = None
    for form, xs, shape, C, void in cases():
        x = (rng.standard_normal(xs) * 3).astype(f32)
        B = xs[0]
        HW = xs[1] * xs[2] if form == "plain" else shape[0] * shape[1]
        t, w = _targets(rng, B, HW, C, void)
        for weights in (w, None):
            ch = _Chain(form, x, shape, t, weights, C, lam)
            d = ch.run()
            r64 = J.evaluate(form, x, shape, t, weights, lam, np.float64)
            r32 = J.evaluate(form, x, shape, t, weights, lam, np.float32)
            u, _ = J.mask(t, weights, C)
            what = (form, xs, shape, "weighted" if weights is not None else "plain", "void" if void else "")
            assert np.array_equal(d["sums"][..., 2], r64["sums"][..., 2]), (what, "Y is exact")
            assert np.isfinite(d["dlogits"]).all() and np.isfinite(d["coef"]).all() and np.isfinite(d["sums"]).all()
            zero = ~u if weights is not None else (t >= C)
            assert (d["dlogits"][zero] == 0).all(), (what, "dlogits == 0 where u = 0 and the cross-entropy half is zero")
            assert np.array_equal(d["coef"] == 0, np.repeat(r64["sums"][..., 2:] == 0, 2, -1)), (what, "absent classes")
            assert d["n_legal"] == float((r64["sums"][..., 2].sum(0) > 0).sum())
            if void:
                assert d["lj"] == 0.0 and (d["coef"] == 0).all() and (d["sums"] == 0).all() and (d["dlogits"] == 0).all()
            # lambda * L_J: once, in the extra row; the folded loss is the cross-entropy plus it
            assert d["lam_lj"] == float(f32(lam)) * d["lj"] and d["row"] == float(f32(d["lam_lj"]))
            assert abs(d["loss"] - (d["ce"] + d["row"])) <= 4e-7 * max(abs(d["loss"]), 1.0), (what, d["loss"], d["ce"], d["row"])
            assert abs(d["ce"] - r64["ce"]) <= 2e-6 * max(abs(r64["ce"]), 1.0), (what, d["ce"], r64["ce"])
            for q in QUANTITIES:
                a, b = _dist(d[q], r64[q]), _dist(r32[q], r64[q])
                if q == "sums":   # I and S (Y is exact)
                    a, b = _dist(d[q][..., :2], r64[q][..., :2]), _dist(r32[q][..., :2], r64[q][..., :2])
                print("%-8s %-16s %-8s %-8s %-4s %-7s device %.3e, float32 oracle %.3e" % (what + (q, a, b)))
                dd[q], od[q] = max(dd[q], a), max(od[q], b)
            # the cross-entropy half, pinned: an all-zero table leaves today's gradient, bit for bit
            z = ch.run(zero_table=True)
            g0, ce0 = ch.plain_loss_gradient()
            assert np.array_equal(z["dlogits"].view(np.uint32), g0.view(np.uint32)), (what, "cross-entropy half differs")
            assert abs(z["ce"] - ce0) <= 2e-6 * max(abs(ce0), 1.0)
            # two runs
            e = ch.run()
            for k in ("sums", "coef", "dlogits"):
                assert np.array_equal(d[k].view(np.uint8), e[k].view(np.uint8)), (what, k, "two runs differ")
            assert (d["lj"], d["loss"], d["ce"]) == (e["lj"], e["loss"], e["ce"])
    for q in QUANTITIES:
        print("jaccard %s %s: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2)" % (
            form, q, dd[q], od[q], dd[q] / od[q] if od[q] else 0.0))
    for q in QUANTITIES:
        assert dd[q] <= 2 * od[q], (form, q, dd[q], od[q])


def test_more_than_32_classes_and_bad_arguments_are_refused():
    from dl3_amd import capi
    ch = _Chain("plain", np.zeros((1, 1, 4, 3), f32), None, np.zeros((1, 4), f32), None, 3, 1.0)
    L = capi.lib()
    s = torch.cuda.current_stream().cuda_stream
    assert L.dl3_jaccard_sums_plain(ch.x.data_ptr(), ch.t.data_ptr(), None, ch.part.data_ptr(), 1, 4, 33, s) == -4
    assert L.dl3_softmax_xent_jaccard(ch.x.data_ptr(), ch.t.data_ptr(), None, ch.nnz.data_ptr(), ch.coef.p, 1.0, ch.dl.p,
                                      ch.lpart.p, 1, 4, 33, s) == -4
    for lam in (-1.0, float("nan"), float("inf")):
        assert L.dl3_jaccard_coef(ch.part.data_ptr(), ch.P, 1, 3, lam, ch.sums.data_ptr(), ch.coef.p, ch.stats.data_ptr(),
                                  None, s) == -1
    assert L.dl3_jaccard_partials(0, 4) == 0 and L.dl3_jaccard_loss_partials(1, 0) == 0
    torch.cuda.synchronize()
    assert_bands(ch.pool)


# -------------------------------------------------------------------------------------------------------- model level
SHAPE, CLASSES, B = (64, 64, 3), 3, 2
LAM = 0.5


def _batches(n, b=B, seed=7):
    """different labels every step; class 2 is absent from image 0 of step 1"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n):
        x = rng.integers(0, 256, (b,) + SHAPE).astype(f32)
        y = rng.integers(0, CLASSES + 1, (b, SHAPE[0] * SHAPE[1], 1)).astype(f32)
        if s == 1:
            y[0][y[0] == 2] = 1
        sw = ((y[..., 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2]) * (rng.random(y.shape[:2]) > 0.1)).astype(f32)
        out.append((x, y, sw))
    return out


def _model(head, loss):
    from tests.test_gpu_model import _build, _load
    model, params = _build("mobilenetv2", SHAPE, CLASSES, head)
    _load(model, params)
    model.compile(optimizer=None, loss=loss)
    return model


def _ce32(z, y, sw):
    """the cross-entropy as a float32 evaluation gives it: today's loss kernels keep their partials in float32, so the
    yardstick forms the per-pixel terms l * w / nnz in float32 and adds them in float32, in index order"""
    from tests import eval_oracle as E
    z = np.asarray(z, f32).reshape(y.shape[0], -1, z.shape[-1])
    ell = E.pixel_loss(z, y.reshape(y.shape[0], -1), f32)
    w = np.asarray(sw, f32).reshape(ell.shape)
    inv = f32(1) / f32(max(int((w != 0).sum()), 1))
    return float(np.cumsum((ell * w * inv).reshape(-1), dtype=f32)[-1])


def _weights(model):
    eng = model._active
    torch.cuda.synchronize()
    return [a.cpu().numpy().copy() for a in (eng.params, eng.state, eng.adam_m, eng.adam_v)]


@pytest.mark.parametrize("head", ["deeplab", "original", "subpixel"])
def test_step_follows_the_oracle_under_graph_replay(head):
    """three steps with different labels — eager, capture, replay: the record (sums, table, L_J, cross-entropy) and the
    returned loss against the oracle's evaluation of Engine.logits() under the yardstick; the tables of steps 2 and 3
    follow the new labels (a frozen argument would repeat step 1's)"""
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    model = _model(head, U.sparse_crossentropy_jaccard(LAM))
    qs = ("sums", "coef", "lj", "ce", "loss")
    dd, od = dict.fromkeys(qs, 0.0), dict.fromkeys(qs, 0.0)
    tables = []
    for s, (x, y, sw) in enumerate(_batches(3)):
        loss = model.train_on_batch(x, y, sw)
        eng = model._active
        assert eng.jaccard == LAM and eng.mining is None
        sums, coef, lj, ce = eng.jaccard_record()
        z = eng.logits()
        r64 = J.evaluate("plain", z, None, y, sw, LAM, np.float64)
        r32 = J.evaluate("plain", z, None, y, sw, LAM, np.float32)
        assert np.array_equal(sums[..., 2], r64["sums"][..., 2]), (s, "Y follows this step's labels")
        # the cross-entropy and the returned loss are float32 sums on the device: so are the yardstick's
        got = dict(sums=sums[..., :2], coef=coef, lj=lj, ce=ce, loss=loss)
        ce32 = _ce32(z, y, sw)
        y32 = dict(sums=r32["sums"][..., :2], coef=r32["coef"], lj=r32["lj"], ce=ce32,
                   loss=float(f32(f32(ce32) + f32(f32(LAM) * f32(r32["lj"])))))
        y64 = dict(sums=r64["sums"][..., :2], coef=r64["coef"], lj=r64["lj"], ce=r64["ce"], loss=r64["loss"])
        for q in qs:
            a, b = _dist(got[q], y64[q]), _dist(y32[q], y64[q])
            print("%s step %d %-5s device %.3e, float32 oracle %.3e" % (head, s, q, a, b))
            dd[q], od[q] = max(dd[q], a), max(od[q], b)
        assert 0 < lj < 1 and abs(loss - (ce + LAM * lj)) <= 4e-7 * loss
        tables.append(coef)
    assert (tables[1][0, 2] == 0).all() and (tables[0][0, 2] != 0).all() and (tables[2][0, 2] != 0).all()
    assert not np.array_equal(tables[0], tables[2])
    eng = model._active
    assert eng.graph is not None, "the step was never captured"
    names = [r[0] for r in eng.ops_fwd]
    assert sum(n in Engine.JACCARD_OPS for n in names) == 3 and names.count("dl3_count_nonzero") == 1
    # this loss's admission rule: a bilinear head is read as `bilinear`, the Subpixel head (fused by today's loss) as `plain`
    assert eng.head.form == ("shuffle" if head == "subpixel" else "bilinear")
    form = "bilinear" if head != "subpixel" else "plain"
    assert eng.loss_head.form == form and ("dl3_phase_shift" in names) == (head == "subpixel")
    assert "dl3_jaccard_sums_" + form in names and not any(n.endswith("xent_fold") or n.startswith("dl3_shuffle") for n in names)
    for q in qs:
        print("%s %s: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2)" % (
            head, q, dd[q], od[q], dd[q] / od[q] if od[q] else 0.0))
    for q in qs:
        assert dd[q] <= 2 * od[q], (head, q, dd[q], od[q])


def test_weight_zero_is_the_plain_loss():
    """jaccard_weight = 0: loss, weights and optimizer state bit-identical to the plain loss, the same plan, no record"""
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    a = _model("deeplab", U.sparse_crossentropy_jaccard(0.0))
    b = _model("deeplab", U.sparse_crossentropy_ignoring_last_label)
    for x, y, sw in _batches(3):
        assert a.train_on_batch(x, y, sw) == b.train_on_batch(x, y, sw)
    for wa, wb in zip(_weights(a), _weights(b)):
        assert np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
    ea, eb = a._active, b._active
    assert ea.jaccard is None
    assert [r[0] for r in ea.ops_fwd] == [r[0] for r in eb.ops_fwd] and [r[0] for r in ea.ops_bwd] == [r[0] for r in eb.ops_bwd]
    assert not any(r[0] in Engine.JACCARD_OPS for r in ea.ops_fwd + ea.ops_bwd)
    with pytest.raises(ValueError):
        ea.jaccard_record()


def test_the_term_changes_the_step_and_evaluation_is_untouched():
    from dl3_amd import utils as U
    a = _model("deeplab", U.sparse_crossentropy_jaccard(LAM))
    b = _model("deeplab", U.sparse_crossentropy_ignoring_last_label)
    (x, y, sw), = _batches(1, b=4, seed=9)
    ra = a.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    rb = b.evaluate(x, y, batch_size=2, sample_weight=sw, device=True)
    assert ra == rb and np.isfinite(ra).all()
    assert np.array_equal(a.predict(x[:2]), b.predict(x[:2]))
    la, lb = a.train_on_batch(x[:2], y[:2], sw[:2]), b.train_on_batch(x[:2], y[:2], sw[:2])
    _, _, lj, ce = a._active.jaccard_record()
    assert abs(ce - lb) <= 1e-6 * lb and abs(la - (lb + LAM * lj)) <= 1e-6 * la and la > lb
    assert not np.array_equal(_weights(a)[0], _weights(b)[0])


def test_refusals_at_the_engine():
    from dl3_amd import utils as U
    from dl3_amd.engine import Engine
    from tests.test_gpu_model import _build, _load
    model = _model("deeplab", U.sparse_crossentropy_jaccard(LAM))
    with pytest.raises(ValueError, match="mining"):
        Engine(model, batch=1, training=True, jaccard=LAM, mining=(0.25, 0))
    with pytest.raises(ValueError, match="data-parallel"):
        Engine(model, batch=1, training=True, jaccard=LAM, external_nnz=True)
    wide, params = _build("mobilenetv2", SHAPE, 33, "deeplab")
    wide.compile(optimizer=None, loss=U.sparse_crossentropy_jaccard(LAM))
    with pytest.raises(ValueError, match="32 classes"):
        wide.train_on_batch(np.zeros((1,) + SHAPE, f32), np.zeros((1, SHAPE[0] * SHAPE[1], 1), f32))


def test_device_feed_over_batches_of_2_2_1():
    """fit_generator(device_feed=True) over batches of 2, 2 and then 1 (the feed takes one batch size per call, so the
    single image is a second call): engines of B = 2 and B = 1 carry the term and share the optimizer's clock; the last
    batch's record against the float64 oracle on its logits (the feed's balanced weights reach the term as the mask of
    the non-void pixels)"""
    from dl3_amd import utils as U
    rng = np.random.default_rng(23)
    batches = []
    for b in (2, 2, 1):
        img = rng.integers(0, 256, (b,) + SHAPE, dtype=np.uint8)
        lab = rng.integers(0, CLASSES, (b, SHAPE[0], SHAPE[1]), dtype=np.uint8)
        lab[rng.uniform(size=lab.shape) < 0.1] = 255
        batches.append((img, lab))
    model = _model("deeplab", U.sparse_crossentropy_jaccard(LAM))
    losses = model.fit_generator(batches[:2], steps_per_epoch=2, device_feed=True, n_classes=CLASSES)
    losses += model.fit_generator(batches[2:], steps_per_epoch=1, device_feed=True, n_classes=CLASSES)
    assert len(losses) == 3 and np.isfinite(losses).all()
    engs = {e.B: e for e in model._engines.values() if e.training}
    assert sorted(engs) == [1, 2] and all(e.jaccard == LAM for e in engs.values())
    eng = engs[1]
    assert eng.iteration == 3
    sums, coef, lj, ce = eng.jaccard_record()
    y = np.where(batches[2][1] == 255, CLASSES, batches[2][1]).reshape(1, -1).astype(f32)
    z = eng.logits()
    r64 = J.evaluate("plain", z, None, y, None, LAM, np.float64)
    assert np.array_equal(sums[..., 2], r64["sums"][..., 2])
    # one batch, one image: no yardstick statistics here, the bound comes from the format — a float32 p is within 2^-22 of
    # its value (expf and the normalisation, an ulp each), so are the sums of such terms, J = I / U within twice that,
    # and L_J, a mean of J <= 1, within 2^-21 absolute
    rel = np.abs(sums[..., :2] - r64["sums"][..., :2]) / r64["sums"][..., :2]
    print("device feed: sums relative %.3e, L_J %.9f against %.9f" % (rel.max(), lj, r64["lj"]))
    assert rel.max() <= 2.0 ** -22 and abs(lj - r64["lj"]) <= 2.0 ** -21
    assert np.array_equal(coef, J.coefficients(sums)[0].astype(f32))      # the table is the recorded sums' own
    assert abs(float(losses[2]) - (ce + LAM * lj)) <= 4e-7 * float(losses[2])
