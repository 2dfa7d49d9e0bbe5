"""-m gpu: the kernels that decode the output head's class scores, at every class-count instantiation (C in 1, 8, 9, 24,
25, 32: both sides of each MAXC bucket of csrc/common.h DL3_DISPATCH_MAXC, the single class and the full row), on logits
centred on 0 and on logits far below 0, where a pad register that reads 0 instead of being masked would show.  The cases,
their inputs and the references are tests/head_class_cases.py; tests/test_head_class_cases_host.py shows without a GPU
that the table reaches every compiled <MAXC, variant> and that a zero pad in the maximum and the sum misses the margins
used here.

No tolerance is new.  Each family is held to the rule its own test file states:
  * training loss tails (test_gpu_focal.py's rule, which its gamma = 0 case shares with them), focal tails, soft-Jaccard,
    mining front: per quantity, the largest distance from the float64 oracle over the form's cases is at most twice the
    float32 oracle's own largest distance over the same cases; both numbers of every case are printed.
  * evaluation tail, CRF unary: the same factor per input (per image / per call), bit equality with the float32 oracle
    where its distance is 0 (tests/test_gpu_crf_unary.py _compare).
  * fold forms (__expf): the constants of test_gpu_ops.py test_xent_fold_and_rows, and for the focal twin the rule of
    test_gpu_focal.py test_fold_form_against_todays_fold_kernel.
  * integers (nnz, counts, confusion, Y, the exact-zero pattern of gradients and of v) exactly; masks equal to the
    existing kernels' bit for bit and to float64 wherever it is decidable.
  * every float output inside guard bands that must not change; two runs bit-identical.

Measured worst ratios (MI355X): DESIGN.md §9, §10, §15, §16, §18."""
import numpy as np
import pytest
import torch

from oracle import dl3_oracle as O
from tests import head_class_cases as H
from tests import ops_oracle as OO
from tests.gpu_util import Guarded, assert_bands, call, dev, host, relerr, release

pytestmark = pytest.mark.gpu

f32 = np.float32


def _lib():
    from dl3_amd import capi
    return capi.lib()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Worst:
    """per quantity: the largest device distance and the largest float32-oracle distance over a form's cases"""

    def __init__(self, family, form):
        self.family, self.form = family, form
        self.dd, self.od = dict.fromkeys(H.QUANTITIES[family], 0.0), dict.fromkeys(H.QUANTITIES[family], 0.0)
        self.at = dict.fromkeys(H.QUANTITIES[family], "")

    def add(self, what, got, r64, r32):
        for q in H.QUANTITIES[self.family]:
            a, b = H.distance(q, got[q], r64[q]), H.distance(q, r32[q], r64[q])
            print("%-90s %-8s device %.3e, float32 oracle %.3e" % (what, q, a, b))
            if a > self.dd[q]:
                self.dd[q], self.at[q] = a, what
            self.od[q] = max(self.od[q], b)

    def check(self):
        for q in H.QUANTITIES[self.family]:
            print("head classes %s %s %s: device / float32-oracle distance = %.3e / %.3e = %.2f (bound 2), worst at %s" % (
                self.family, self.form, q, self.dd[q], self.od[q], self.dd[q] / self.od[q] if self.od[q] else 0.0, self.at[q]))
        for q in H.QUANTITIES[self.family]:
            assert self.dd[q] <= 2 * self.od[q], (self.family, self.form, q, self.dd[q], self.od[q], self.at[q])


def _focal_case(case, x, t, w):
    from tests.test_gpu_focal import _Case
    form, shape = H.oracle_form(case)
    return _Case("bilinear_fold" if case.form == "fold" else form, x, shape, t, w, case.C)


def _check_partials(case):
    L = _lib()
    if case.form == "plain":
        assert L.dl3_rows_partials(case.dims[0] * case.dims[1]) > 1
    elif case.form == "shuffle" and case.family in ("xent", "focal"):
        N, Hh, W, r = case.dims
        assert L.dl3_shuffle_xent_partials(N, Hh, W, case.C, r) == N * Hh * 2   # tiles of 8 and 5 pixels at every C
    elif case.form == "shuffle":
        N, Hh, W, r = case.dims
        P = L.dl3_eval_tail_shuffle_partials(N, Hh, W, case.C, r)
        assert P == Hh * len(H.tiles(W, H.shuffle_pb(W, case.C, r))) and P > Hh   # every row takes more than one tile


# ----------------------------------------------------------------------- training loss tails and focal tails, unfused
def _loss_tail_group(family, form):
    worst = _Worst(family, form)
    for case in H.group(family, form):
        _check_partials(case)
        C = case.C
        for x, t, w, kw, r64, r32 in H.runs(case):
            what = H.describe(case, w, kw)
            ch = _focal_case(case, x, t, w)
            run = (lambda: ch.focal(kw["gamma"], kw["alpha"])) if family == "focal" else ch.today
            d = run()
            g = ch.full(d["g"])
            assert np.isfinite(g).all() and np.isfinite(d["part"]).all() and np.isfinite(d["loss"]), what
            zero = H.is_void(t, C) | ((w == 0) if w is not None else False)
            assert (g[zero] == 0).all(), (what, "dlogits == 0 where w = 0 or the label is void")
            if C > 1:
                assert np.abs(g[~zero]).max() > 0, what
            else:
                assert not g.any(), (what, "one class: p = 1 is outside the clip interval, no gradient")
            worst.add(what, dict(loss=d["loss"], dlogits=g), r64, r32)
            e = run()
            assert np.array_equal(_bits(d["g"]), _bits(e["g"])), (what, "two runs differ")
            assert np.array_equal(_bits(d["part"]), _bits(e["part"])) and d["loss"] == e["loss"], what
        release()
    worst.check()


@pytest.mark.parametrize("form", ["plain", "bilinear", "shuffle"])
def test_loss_tails(form):
    """dl3_softmax_xent, dl3_upsample_softmax_xent, dl3_shuffle_softmax_xent"""
    _loss_tail_group("xent", form)


@pytest.mark.parametrize("form", ["plain", "bilinear", "shuffle"])
def test_focal_tails(form):
    """dl3_focal_xent, dl3_upsample_focal_xent, dl3_shuffle_focal_xent: gamma in {0.5, 2}, alpha null and per class; one
    case per form whose void pixels are 255 and -1"""
    _loss_tail_group("focal", form)


# -------------------------------------------------------------------------------------------------------- fold forms
def _rows_to_source(ch, N, Hi, Wi, Ho, C):
    """dl3_resize_bilinear_bwd_rows on the fold kernel's output, twice"""
    outs = []
    for _ in range(2):
        pool = []
        dx = Guarded(pool, "dx", N * Hi * Wi * C)
        call("dl3_resize_bilinear_bwd_rows", ch.g.p, dx.p, C, N, Hi, Wi, Ho, C, 0)
        assert_bands(pool)
        outs.append(host(dx.t).copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(_bits(outs[0]), _bits(outs[1]))
    return outs[0]


def _unfused_source_gradient(case, x, t, w, kw):
    """the unfused form of the same family, then dl3_resize_bilinear_bwd"""
    N, Hi, Wi, Ho, Wo = case.dims
    C = case.C
    un = _focal_case(case._replace(form="bilinear"), x, t, w)
    d = un.focal(kw["gamma"], kw["alpha"]) if case.family == "focal" else un.today()
    pool = []
    dx = Guarded(pool, "dx", N * Hi * Wi * C)
    call("dl3_resize_bilinear_bwd", un.g.p, C, dx.p, C, N, Hi, Wi, Ho, Wo, C, 0, None, 0)
    assert_bands(pool)
    return host(dx.t).copy(), d


def _set_pref(monkeypatch, case):
    if case.pref_env is None:
        monkeypatch.delenv("DL3_XENT_PREF", raising=False)
    else:
        monkeypatch.setenv("DL3_XENT_PREF", case.pref_env)


def test_loss_tail_fold_form(monkeypatch):
    """dl3_upsample_softmax_xent_fold in <24> and <32>, prefetching and not: the rule of test_gpu_ops.py
    test_xent_fold_and_rows — loss within 1e-5 of the float64 oracle, the gradient through dl3_resize_bilinear_bwd_rows
    within 1e-4 of the oracle's (relative to its largest element) and within 1e-5 of the unfused pair of kernels, and the
    two variants bit-identical on the same input"""
    N, Hi, Wi, Ho, Wo = H.BILINEAR
    seen = {}
    for case in H.group("xent", "fold"):
        C = case.C
        x, t, w = H.inputs(case)
        for ww in (w, None):
            what = H.describe(case, ww, {})
            tape = O.Tape()
            lo = x.astype(np.float64)
            up = O.resize_bilinear_tf1(lo, Ho, Wo, tape=tape)
            wd = np.ones(t.shape) if ww is None else ww.astype(np.float64)
            _, dl_ref, _ = O.loss_sparse_xent_ignoring_last_label(up.reshape(1, -1, C), t.reshape(1, -1), wd.reshape(1, -1))
            # the loss by tests/ops_oracle.py, which clips at the contract's float32 constants 1e-7f and 1 - 1e-7f (the
            # double constants of oracle/dl3_oracle.py differ from them by 19 % of -log(1 - 1e-7): all there is at C = 1)
            loss_ref = H.reference("xent", "bilinear", x, (Ho, Wo), t, ww, np.float64)["loss"]
            dlo_ref = tape.backward(up, dl_ref.reshape(up.shape))[id(lo)]
            ch = _focal_case(case, x, t, ww)
            _set_pref(monkeypatch, case)
            d = ch.today()
            e = ch.today()
            assert np.isfinite(d["g"]).all() and np.array_equal(_bits(d["g"]), _bits(e["g"])), (what, "two runs differ")
            assert np.array_equal(_bits(d["part"]), _bits(e["part"])), what
            dlo = _rows_to_source(ch, N, Hi, Wi, Ho, C)
            monkeypatch.delenv("DL3_XENT_PREF", raising=False)
            dlo2, _ = _unfused_source_gradient(case, x, t, ww, {})
            dlo, dlo2 = dlo.reshape(dlo_ref.shape), dlo2.reshape(dlo_ref.shape)
            lsum = float(d["part"].astype(np.float64).sum())
            print("%-80s loss %.3e (1e-5) | source gradient: oracle %.3e (1e-4), unfused kernels %.3e (1e-5)" % (
                what, abs(lsum - loss_ref) / abs(loss_ref), relerr(dlo, dlo_ref), relerr(dlo, dlo2)))
            assert abs(lsum - loss_ref) < 1e-5 * abs(loss_ref), what
            assert relerr(dlo, dlo_ref) < 1e-4, what
            assert relerr(dlo, dlo2) < 1e-5, what
            if C == 1:
                assert not d["g"].any()
            seen.setdefault((C, case.kind, ww is None), {})[case.variant] = (d["g"], d["part"])
        release()
    pairs = 0
    for key, v in seen.items():
        if len(v) == 2:   # rows that request their operands one row ahead == rows that request their own
            assert np.array_equal(_bits(v["pref"][0]), _bits(v["nopref"][0])), key
            assert np.array_equal(_bits(v["pref"][1]), _bits(v["nopref"][1])), key
            pairs += 1
    assert pairs == 3 * 2 * 2   # C = 8, 24, 32


def test_focal_tail_fold_form(monkeypatch):
    """dl3_upsample_focal_xent_fold in <24> and <32>, prefetching and not: the rule of test_gpu_focal.py
    test_fold_form_against_todays_fold_kernel (gamma = 2, per-class alpha; d_focal <= 2 d_ce on the same input, the loss
    within the doubled distance of today's kernel and no less than 2e-6), the source gradient against the unfused kernels
    by the 1e-5 of test_xent_fold_and_rows, the two variants bit-identical"""
    from tests import focal_oracle as F
    N, Hi, Wi, Ho, Wo = H.BILINEAR
    seen = {}
    worst = (0.0, "")
    missed = []
    for case in H.group("focal", "fold"):
        C = case.C
        x, t, w = H.inputs(case)
        alpha = H.alpha(case)
        for ww in (w, None):
            what = H.describe(case, ww, {})

            def folded(gamma, al):
                r = F.evaluate("bilinear", x, (Ho, Wo), t, ww, gamma, al, np.float64)
                return OO.resize_bwd_cols(r["dlogits"].reshape(N, Ho, Wo, C), Wi, Wo)[0], r["loss"]

            ch = _focal_case(case, x, t, ww)
            _set_pref(monkeypatch, case)
            c = ch.today()
            d = ch.focal(2.0, alpha)
            e = ch.focal(2.0, alpha)
            assert np.isfinite(d["g"]).all() and np.array_equal(_bits(d["g"]), _bits(e["g"])) and d["loss"] == e["loss"], what
            assert np.array_equal(_bits(d["part"]), _bits(e["part"])), what
            dlo = _rows_to_source(ch, N, Hi, Wi, Ho, C)
            monkeypatch.delenv("DL3_XENT_PREF", raising=False)
            dlo2, _ = _unfused_source_gradient(case, x, t, ww, dict(gamma=2.0, alpha=alpha))
            ref, loss = folded(2.0, alpha)
            ref_ce, loss_ce = folded(0.0, None)
            if C == 1:   # no gradient at all (p = 1 is outside the clip interval): bit equality
                assert not ref.any() and not ref_ce.any() and not d["g"].any() and not c["g"].any(), what
                d_focal = d_ce = 0.0
            else:
                d_focal = H.distance("dlogits", d["g"].reshape(ref.shape), ref) / np.abs(ref).max()
                d_ce = H.distance("dlogits", c["g"].reshape(ref_ce.shape), ref_ce) / np.abs(ref_ce).max()
                assert d_focal <= 2 * d_ce, (what, d_focal, d_ce)
                worst = max(worst, (d_focal / d_ce, what))
            print("%-80s d_focal %.3e, d_ce %.3e, ratio %.2f (bound 2); loss %.7f against %.7f, today's %.7f against %.7f; "
                  "source gradient against the unfused kernels %.3e (1e-5)" % (
                      what, d_focal, d_ce, d_focal / d_ce if d_ce else 0.0, d["loss"], loss, c["loss"], loss_ce, relerr(dlo, dlo2)))
            if not abs(d["loss"] - loss) <= max(2 * abs(c["loss"] - loss_ce) / loss_ce, 2e-6) * loss:
                missed.append((what, d["loss"], loss))
            assert relerr(dlo, dlo2) < 1e-5, what
            seen.setdefault((C, case.kind, case.void, ww is None), {})[case.variant] = (d["g"], d["part"])
        release()
    print("head classes focal fold: worst d_focal / d_ce = %.2f (bound 2) at %s" % worst)
    for m in missed:
        print("head classes focal fold MISS loss %s: device %.6e float64 %.6e" % m)
    pairs = 0
    for key, v in seen.items():
        if len(v) == 2:
            assert np.array_equal(_bits(v["pref"][0]), _bits(v["nopref"][0])), key
            assert np.array_equal(_bits(v["pref"][1]), _bits(v["nopref"][1])), key
            pairs += 1
    assert pairs == 3 * 2 * 2
    assert not missed, missed


# ----------------------------------------------------------------------------------------------------- soft-Jaccard
@pytest.mark.parametrize("form", ["plain", "bilinear"])
def test_jaccard(form):
    """dl3_jaccard_sums_* in <8>, <24>, <32>, dl3_jaccard_coef and dl3_*softmax_xent_jaccard: the assertions of
    test_gpu_jaccard.py test_forms_against_the_float64_oracle"""
    from tests import jaccard_oracle as J
    from tests.test_gpu_jaccard import _Chain
    worst = _Worst("jaccard", form)
    lam = H.LAMBDA
    for case in H.group("jaccard", form):
        C = case.C
        oform, shape = H.oracle_form(case)
        for x, t, w, kw, r64, r32 in H.runs(case):
            what = H.describe(case, w, kw)
            ch = _Chain(oform, x, shape, t, w, C, lam)
            d = ch.run()
            u, _ = J.mask(t, w, C)
            assert np.array_equal(d["sums"][..., 2], r64["sums"][..., 2]), (what, "Y is exact")
            assert np.isfinite(d["dlogits"]).all() and np.isfinite(d["coef"]).all() and np.isfinite(d["sums"]).all(), what
            zero = ~u if w is not None else H.is_void(t, C)
            assert (d["dlogits"][zero] == 0).all(), (what, "dlogits == 0 where u = 0 and the cross-entropy half is zero")
            assert np.array_equal(d["coef"] == 0, np.repeat(r64["sums"][..., 2:] == 0, 2, -1)), (what, "absent classes")
            assert d["n_legal"] == float((r64["sums"][..., 2].sum(0) > 0).sum()), what
            assert d["lam_lj"] == float(f32(lam)) * d["lj"] and d["row"] == float(f32(d["lam_lj"])), what
            assert abs(d["loss"] - (d["ce"] + d["row"])) <= 4e-7 * max(abs(d["loss"]), 1.0), (what, d["loss"], d["ce"], d["row"])
            assert abs(d["ce"] - r64["ce"]) <= 2e-6 * max(abs(r64["ce"]), 1.0), (what, d["ce"], r64["ce"])
            worst.add(what, d, r64, r32)
            z = ch.run(zero_table=True)
            g0, ce0 = ch.plain_loss_gradient()
            assert np.array_equal(_bits(z["dlogits"]), _bits(g0)), (what, "cross-entropy half differs")
            assert abs(z["ce"] - ce0) <= 2e-6 * max(abs(ce0), 1.0), what
            e = ch.run()
            for k in ("sums", "coef", "dlogits"):
                assert np.array_equal(_bits(d[k]), _bits(e[k])), (what, k, "two runs differ")
            assert (d["lj"], d["loss"], d["ce"]) == (e["lj"], e["loss"], e["ce"]), what
        release()
    worst.check()


# ----------------------------------------------------------------------------------------------------- mining front
def _device_v(case, x, t, w):
    C = case.C
    xd, td = dev(x), dev(t)
    wd = dev(w) if w is not None else None
    wp = wd.data_ptr() if wd is not None else None
    pool = []
    v = Guarded(pool, "v", t.size)
    if case.form == "plain":
        call("dl3_pixel_xent_plain", xd.data_ptr(), td.data_ptr(), wp, v.p, t.size, C)
    elif case.form == "bilinear":
        N, Hi, Wi, Ho, Wo = case.dims
        call("dl3_pixel_xent_bilinear", xd.data_ptr(), td.data_ptr(), wp, v.p, N, Hi, Wi, Ho, Wo, C)
    else:
        N, Hh, W, r = case.dims
        call("dl3_pixel_xent_shuffle", xd.data_ptr(), td.data_ptr(), wp, v.p, N, Hh, W, C, r)
    assert_bands(pool)
    return host(v.t).copy()


@pytest.mark.parametrize("form", ["plain", "bilinear", "shuffle"])
def test_mining_front(form):
    """dl3_pixel_xent_*: the assertions of test_gpu_mine.py test_pixel_loss_against_the_float64_oracle"""
    worst = _Worst("mine", form)
    for case in H.group("mine", form):
        _check_partials(case)
        C = case.C
        for x, t, w, kw, r64, r32 in H.runs(case):
            what = H.describe(case, w, kw)
            vd = _device_v(case, x, t, w)
            assert vd.shape == (t.size,) and np.isfinite(vd).all() and (vd >= 0).all(), what
            zero = H.is_void(t, C).reshape(-1) | ((w.reshape(-1) == 0) if w is not None else False)
            if C > 1:
                assert np.array_equal(vd == 0, zero), (what, "v == 0 exactly where w == 0 or the label is void")
            else:   # one class: p = 1 is clipped to 1 - 1e-7, every pixel that counts has the same small positive loss
                assert (vd[zero] == 0).all() and (vd[~zero] > 0).all(), what
            assert not np.signbit(vd).any(), what
            worst.add(what, dict(v=vd), r64, r32)
            assert np.array_equal(_bits(vd), _bits(_device_v(case, x, t, w))), (what, "two runs differ")
        release()
    worst.check()


# -------------------------------------------------------------------------------------------------- evaluation tail
class _IntGuard:
    """a device buffer of n elements of dtype between two runs of 16 sentinel elements (64 or 128 bytes: the payload
    keeps the 16-byte alignment the 16-byte variant asks of the mask)"""
    PAD = 16

    def __init__(self, n, dtype, fill, sentinel):
        self.n, self.sentinel = n, sentinel
        self.full = torch.full((n + 2 * self.PAD,), sentinel, dtype=dtype, device="cuda")
        self.t = self.full[self.PAD:self.PAD + n]
        self.t.fill_(fill)
        self.p = self.t.data_ptr()

    def intact(self):
        edge = torch.cat([self.full[:self.PAD], self.full[self.PAD + self.n:]])
        return bool((edge == self.sentinel).all())


def _device_tail(case, x, t, w, conf):
    L = _lib()
    C, (N, HW) = case.C, H.pixels(case)
    dx, dl = dev(x), dev(t)
    dw = dev(w) if w is not None else None
    if case.form == "bilinear":
        Nn, Hi, Wi, Ho, Wo = case.dims
        P, tail = L.dl3_eval_tail_bilinear_partials(N, Hi, Wi, Ho, Wo, C), (N, Hi, Wi, Ho, Wo, C)
    elif case.form == "shuffle":
        Nn, Hh, W, r = case.dims
        P, tail = L.dl3_eval_tail_shuffle_partials(N, Hh, W, C, r), (N, Hh, W, C, r)
    else:
        P, tail = L.dl3_eval_tail_plain_partials(N, HW, C), (N, HW, C)
    assert P > 0, case.id
    bufs = dict(part=_IntGuard(N * P, torch.float64, float("nan"), -12345.0), loss_sum=_IntGuard(N, torch.float64, float("nan"), -12345.0),
                nnz=_IntGuard(N, torch.int32, -1, -77), counts=_IntGuard(N * 3 * C, torch.int32, -1, -77),
                mask=_IntGuard(N * HW, torch.int32, -1, -77))
    if case.variant == "vec4":   # the launcher's condition for the 16-byte variant, beside Wo % 4 == 0
        assert dl.data_ptr() % 16 == 0 and (dw is None or dw.data_ptr() % 16 == 0) and bufs["mask"].p % 16 == 0
    call("dl3_eval_tail_" + case.form, dx.data_ptr(), dl.data_ptr(), dw.data_ptr() if dw is not None else None,
         bufs["part"].p, bufs["loss_sum"].p, bufs["nnz"].p, bufs["counts"].p, conf.data_ptr(), bufs["mask"].p, *tail)
    torch.cuda.synchronize()
    bad = [k for k, b in bufs.items() if not b.intact()]
    assert not bad, "wrote outside its output: %s" % bad
    out = {k: b.t.cpu().numpy().copy() for k, b in bufs.items()}
    out["counts"] = out["counts"].reshape(N, 3, C)
    return out


def _existing_mask(case, x):
    from tests.test_gpu_eval import _existing_mask as existing
    d = case.dims
    N, HW = H.pixels(case)
    if case.form == "bilinear":
        return existing("bilinear", x, (d[1], d[2], d[3], d[4]), case.C, N, d[3], d[4]).reshape(N, HW)
    if case.form == "shuffle":
        return existing("shuffle", x, (d[1], d[2], d[3]), case.C, N, d[1] * d[3], d[2] * d[3]).reshape(N, HW)
    return existing("plain", x, None, case.C, N, 1, HW).reshape(N, HW)


@pytest.mark.parametrize("form", ["plain", "bilinear", "shuffle"])
def test_evaluation_tail(form):
    """dl3_eval_tail_*: the assertions of test_gpu_eval.py test_eval_tail_operator; the bilinear form in its scalar and
    its 16-byte variant"""
    from tests import eval_oracle as EO
    worst = (0.0, "")
    missed = []
    for case in H.group("eval", form):
        _check_partials(case)
        C, (N, HW) = case.C, H.pixels(case)
        existing = None
        for x, t, w, kw, r64, r32 in H.runs(case):
            what = H.describe(case, w, kw)
            tau = 32.0 * 2.0 ** -24 * float(np.abs(r64["logits"]).max())
            unsure = (r64["margin"] <= tau).reshape(N, HW)
            assert unsure.mean() <= 1e-3, what
            conf = torch.zeros(C, C, dtype=torch.int64, device="cuda")
            a = _device_tail(case, x, t, w, conf)
            conf1 = conf.cpu().numpy().copy()
            b = _device_tail(case, x, t, w, conf)
            conf2 = conf.cpu().numpy().copy()
            mask = a["mask"].reshape(N, HW)
            if existing is None:
                existing = _existing_mask(case, x)
            assert np.array_equal(mask, existing), (what, "mask differs from the resize / phase-shift + argmax kernels")
            assert np.array_equal(mask[~unsure], r64["mask"].reshape(N, HW)[~unsure]), what
            assert np.array_equal(a["counts"], O.seg_counts(mask, t, C)), what
            ww = np.ones_like(t) if w is None else w
            assert np.array_equal(a["nnz"], (ww != 0).sum(1)), what
            cm = EO.confusion(mask, t, C)
            assert np.array_equal(conf1, cm) and np.array_equal(conf2, 2 * cm), what
            for n in range(N):
                ref = r64["loss_sum"][n]
                d_dev = abs(a["loss_sum"][n] - ref) / abs(ref)
                d_f32 = abs(float(r32["loss_sum"][n]) - ref) / abs(ref)
                print("%-80s image %d: loss_sum device %.3e float32-oracle %.3e ratio %.2f" % (
                    what, n, d_dev, d_f32, d_dev / max(d_f32, 1e-300)))
                if not d_dev <= 2.0 * d_f32:
                    missed.append((what, n, d_dev, d_f32))
                worst = max(worst, (d_dev / d_f32, what))
            for k in ("loss_sum", "nnz", "counts", "mask", "part"):
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, "two runs differ")
        release()
    print("head classes eval %s loss_sum: worst device / float32-oracle distance = %.2f (bound 2) at %s; %d images miss" % (
        (form,) + worst + (len(missed),)))
    for m in missed:
        print("head classes eval %s MISS %s image %d: device %.3e float32-oracle %.3e" % ((form,) + m))
    assert not missed, missed


# -------------------------------------------------------------------------------------------------------- CRF unary
def _device_unary(case, x, scale, clip):
    C, (B, HW) = case.C, H.pixels(case)
    dx = dev(x)
    pool = []
    U = Guarded(pool, "U", B, C, HW)
    if case.form == "bilinear":
        Nn, Hi, Wi, Ho, Wo = case.dims
        call("dl3_crf_unary_bilinear", dx.data_ptr(), U.p, B, Hi, Wi, Ho, Wo, C, scale, clip)
    elif case.form == "shuffle":
        Nn, Hh, W, r = case.dims
        call("dl3_crf_unary_shuffle", dx.data_ptr(), U.p, B, Hh, W, C, r, scale, clip)
    else:
        call("dl3_crf_unary_plain", dx.data_ptr(), 0, U.p, B, HW, C, scale, clip)
    assert_bands(pool)
    return host(U.t).copy()


@pytest.mark.parametrize("form", ["plain", "bilinear", "shuffle"])
def test_crf_unary(form):
    """dl3_crf_unary_* in <8>, <24>, <32>, scale in {0, 0.5} x clip in {0, 1e-5}: _compare of test_gpu_crf_unary.py"""
    from tests.test_gpu_crf_unary import _compare
    worst = (0.0, 0.0, 0.0, "")
    for case in H.group("unary", form):
        _check_partials(case)
        for x, t, w, kw, r64, r32 in H.runs(case):
            what = H.describe(case, w, kw)
            got = _device_unary(case, x, kw["scale"], kw["clip"])
            r = _compare(what, got, r64["U"], r32["U"])
            print("%-90s U device %.3e, float32 oracle %.3e, ratio %.2f" % (what, r[1], r[2], r[0]))
            worst = max(worst, r + (what,))
            assert np.array_equal(_bits(got), _bits(_device_unary(case, x, kw["scale"], kw["clip"]))), (what, "two runs differ")
        release()
    print("head classes unary %s U: worst device %.3e against float32-oracle %.3e (ratio %.2f, bound 2) at %s" % (
        (form,) + worst[1:3] + (worst[0], worst[3])))
