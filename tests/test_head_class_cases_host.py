"""The case table of tests/test_gpu_head_classes.py (tests/head_class_cases.py), checked without a GPU, so that a failure
of the device test points at the device and not at the input:
  (a) the table reaches every (entry point, MAXC, variant) the sources define, on both sides of each bucket edge, and the
      launch rules it restates are the sources';
  (b) the references alone satisfy each family's existing condition on the new inputs;
  (c) the float32 oracle is finite on the 'negative' kind and its distance from float64 is a usable yardstick;
  (d) a deliberately wrong oracle — the row padded to MAXC with a logit of 0 that takes part in the maximum and the sum —
      misses the float64 result by more than the margin the device test allows, for every family: a device test this
      mutation passed would not have caught the slip it exists for."""
import os
import re

import numpy as np
import pytest

from tests import head_class_cases as H
from tests import eval_oracle as E
from tests import ops_oracle as OO

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "keras-segmentation-deeplab-v3.1_amd",
                    "csrc")
_RUNS = {}


def _runs(case):
    """the references of one case, computed once for the whole file"""
    if case.id not in _RUNS:
        _RUNS[case.id] = list(H.runs(case))
    return _RUNS[case.id]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _groups():
    return [(f, form) for f in H.FAMILIES for form in H.ENTRY[f]]


# ------------------------------------------------------------------------------------------------------ (a) coverage
def test_the_restated_launch_rules_are_the_sources():
    m = re.search(r"#define DL3_DISPATCH_MAXC\(C, M\)(.*?)while \(0\)", _src("common.h"), re.S)
    body = re.sub(r"[\\\s]+", " ", m.group(1))
    assert re.findall(r"\(C\) <= (\d+)", body) == ["8", "24"] and re.findall(r"M\((\d+)\)", body) == ["8", "24", "32"]
    for C in range(1, 33):
        assert H.dispatch_maxc(C) == (8 if C <= 8 else 24 if C <= 24 else 32)
    assert "constexpr int kHeadMaxC = 32;" in _src("tailmath.h")
    for entry, (fname, text, rule, defined) in H.KERNELS.items():
        src = _src(fname)
        assert 'extern "C" int %s(' % entry in src, entry
        assert text in src, (entry, text)
    # the kernels with one register row for every C take it from kHeadMaxC
    for fname, n in (("losstail.hip", 1), ("jaccard.hip", 1), ("misc.hip", 0)):
        assert _src(fname).count("constexpr int MAXC = kHeadMaxC;") == n, fname
    # a form of the training loss tail has one kernel body and one launcher, whatever the pixel term: the duplicate that
    # the focal loss once was (csrc/focal.hip, a copy of every kernel) does not come back
    tail = _src("losstail.hip")
    assert not os.path.exists(os.path.join(CSRC, "focal.hip"))
    for body in ("row_kernel", "fold_kernel", "shuffle_kernel"):
        assert len(re.findall(r"__global__[^;{]*\bvoid %s\(" % body, tail)) == 1, body
        assert len(re.findall(r"^template <class Term, [^>]*class\.\.\. TermArgs>\n__global__[^;{]*\bvoid %s\(" % body, tail,
                              re.M)) == 1, body
    # the two-bucket choices of the fold and the shuffle launcher, as two_bucket_maxc restates them
    assert tail.count("if (C <= 24) { if (pref) DL3_FOLD(24, true); else DL3_FOLD(24, false); }") == 1
    assert tail.count("else { if (pref) DL3_FOLD(32, true); else DL3_FOLD(32, false); }") == 1
    assert tail.count("if (C <= 24) DL3_SHUFFLE(24); else DL3_SHUFFLE(32);") == 1
    assert "(fold_kernel<Term, MAXC_, PREF_, TermArgs...>)" in tail and "(shuffle_kernel<Term, MAXC_, TermArgs...>)" in tail
    assert "(row_kernel<Term, UPSAMPLE, TermArgs...>)" in tail
    # the fold launcher's prefetch condition, as fold_prefetches restates it
    assert tail.count("constexpr int kPrefFloats = 12, kPrefPixels = 2;") == 1
    assert re.sub(r"\s+", " ", tail).count(
        "const bool pref = (long)Wi * C <= 256L * kPrefFloats && Wo <= 256 * kPrefPixels && (Wi * C) % 4 == 0 && "
        "((long)Wo * C) % 4 == 0 && aligned16(logits_lo) && !(pe && atoi(pe) == 0);") == 1
    assert tail.count('getenv("DL3_XENT_PREF")') == 1
    assert "const bool vec = (Wo % 4 == 0) && aligned16(labels)" in _src("evaltail.hip")
    # the tile rules
    assert "int pb = (int)((48u << 10) / ((size_t)C * (r * r + 1) * sizeof(float)));" in _src("tailmath.h")
    assert "subpixel_tile_pixels(W, C, r, (1024 + r * r - 1) / (r * r))" in _src("tailmath.h")
    assert tail.count("const int PB = subpixel_tile_pixels(W, C, r, 8);") == 2   # the launcher, and the partials it sizes


def test_the_table_reaches_every_kernel_the_sources_define():
    defined = {(e, m, v) for e, (_, _, _, pairs) in H.KERNELS.items() for m, v in pairs}
    reached = {}
    for c in H.ALL:
        for k in H.kernels(c):
            assert k[1] == H.KERNELS[k[0]][2](c.C)
            reached.setdefault(k, set()).add((c.C, c.kind))
    assert set(reached) <= defined, sorted(set(reached) - defined)
    assert not defined - set(reached), "unreached (entry point, MAXC, variant): %r" % sorted(defined - set(reached))
    # every kernel on the 'negative' kind too, and every entry point at every class count of the sweep: both sides of
    # each bucket edge (8 | 9, 24 | 25), the single class and the full row
    for k, seen in reached.items():
        assert {kind for _, kind in seen} == set(H.KINDS), k
    for e in H.KERNELS:
        cs = {c.C for c in H.ALL if e in H.entries(c)}
        assert cs >= set(H.C_SWEEP), (e, cs)
        by_maxc = {}
        for C in H.C_SWEEP:
            by_maxc.setdefault(H.maxc(e, C), []).append(C)
        if len(by_maxc) == 3:
            assert by_maxc == {8: [1, 8], 24: [9, 24], 32: [25, 32]}, e
        elif len(by_maxc) == 2:
            assert by_maxc == {24: [1, 8, 9, 24], 32: [25, 32]}, e


def test_the_variants_and_tiles_are_what_the_table_says():
    N, Hi, Wi, Ho, Wo = H.BILINEAR
    assert (Hi * 2 ** 24) % Ho and (Wi * 2 ** 24) % Wo, "both scale factors are inexact in float32"
    for c in H.ALL:
        if c.form == "fold":
            assert c.variant == ("pref" if H.fold_prefetches(c.dims[2], c.dims[4], c.C, c.pref_env) else "nopref"), c.id
            if c.C in (1, 9, 25):   # Wi = 7: the rows hold no whole float4s, the non-prefetch variant by itself
                assert not H.fold_prefetches(c.dims[2], c.dims[4], c.C, None)
        if c.family == "eval" and c.form == "bilinear":
            assert c.variant == ("vec4" if c.dims[4] % 4 == 0 else "scalar"), c.id
        if c.form == "shuffle" and c.family in ("xent", "focal"):
            n, h, w, r = c.dims
            assert H.tiles(w, H.subpixel_tile_pixels(w, c.C, r, 8)) == [8, 5], c.id
        elif c.form == "shuffle":
            n, h, w, r = c.dims
            t = H.tiles(w, H.shuffle_pb(w, c.C, r))
            assert len(t) > 1 and t[-1] < t[0], (c.id, t)
            if c.C <= 9:
                assert t == [16, 13], (c.id, t)
            if c.C == 32:
                assert t == [5, 5, 5, 5, 5, 4], (c.id, t)
    # the plain shape: more than one 256-pixel workgroup, the last one ragged
    assert H.PLAIN_HW > 256 and H.PLAIN_HW % 256
    assert (H.BILINEAR[0] * H.BILINEAR[3] * H.BILINEAR[4]) % 256 and H.BILINEAR[3] % 8   # ragged last group / band


# ------------------------------------------------------------------------------------------ (b) reference conditions
@pytest.mark.parametrize("family", H.FAMILIES)
def test_targets_and_logits_are_what_the_table_promises(family):
    for c in H.CASES[family]:
        x, t, w = H.inputs(c)
        B, HW = H.pixels(c)
        assert t.shape == w.shape == (B, HW) and x.shape == H.x_shape(c) and x.dtype == np.float32
        void = H.is_void(t, c.C)
        for b in range(B):
            want = set(range(c.C))
            if family == "jaccard" and B > 1 and b == 0:
                want -= {0}            # the existing generator's property: some class is absent from some image
            assert set(np.unique(t[b][~void[b]]).astype(int)) == want, (c.id, b)
        assert 1 / 9 < (np.arange(HW) % 8 == 5).mean() < 1 / 7 and void.mean() >= (np.arange(HW) % 8 == 5).mean()
        if c.void == "C":
            assert set(np.unique(t[void])) == {float(c.C)}
        else:
            assert set(np.unique(t[void])) == {255.0, -1.0} and family == "focal"
        assert 0.1 < (w == 0).mean() < 0.4 and (w[w != 0] > 0).all()
        if c.kind == "negative":
            form, shape = H.oracle_form(c)
            z = E.full_logits(form, x, shape)
            assert -50 < z.min() and z.max() < -10, (c.id, z.min(), z.max())
            assert np.mean((z > -40) & (z < -20)) > 0.95 or family == "unary"


@pytest.mark.parametrize("family", H.FAMILIES)
def test_the_references_meet_each_familys_own_condition(family):
    from tests import crf_unary_oracle as UO
    for c in H.CASES[family]:
        for x, t, w, kw, r64, r32 in _runs(c):
            what = H.describe(c, w, kw)
            if family == "eval":
                # tests/test_gpu_eval.py: the mask must be decidable — pixels under tau at most 0.1 % (a cap on the input)
                tau = 32.0 * 2.0 ** -24 * float(np.abs(r64["logits"]).max())
                assert (r64["margin"] <= tau).mean() <= 1e-3, what
                assert (r64["loss_sum"] > 0).all(), what
            elif family == "unary":
                # tests/test_gpu_crf_unary.py _compare: positions where the float32 oracle is +inf leave the distance;
                # here no probability underflows, every position is compared
                assert np.isfinite(r32["U"]).all() and np.isfinite(r64["U"]).all(), what
                assert np.abs(r64["U"]).max() > 0 or c.C == 1, what
            elif family in ("xent", "focal", "jaccard"):
                # no pixel on the edge of Keras' clip interval: float32 and float64 decide `inside` alike
                z = np.asarray(r64["logits"], np.float64).reshape(-1, c.C)
                tt = np.where(H.is_void(t, c.C), c.C, t).reshape(-1)
                assert not OO.clip_ambiguous_rows(z, tt).any(), what
            if family == "jaccard" and c.dims[0] > 1:
                assert (r64["sums"][..., 2] == 0).any(), what
    assert UO is not None


# ------------------------------------------------------------------------------------------- (c) the float32 oracle
def _yardsticks(family, form):
    """(case, w, kw) -> {quantity: float32-oracle distance}, and the group's largest per quantity"""
    per, top = [], dict.fromkeys(H.QUANTITIES[family], 0.0)
    for c in H.group(family, form):
        for x, t, w, kw, r64, r32 in _runs(c):
            d = {q: H.distance(q, r32[q], r64[q]) for q in H.QUANTITIES[family]}
            per.append((c, x, t, w, kw, r64, r32, d))
            for q in d:
                top[q] = max(top[q], d[q])
    return per, top


@pytest.mark.parametrize("family,form", _groups(), ids=lambda v: str(v))
def test_float32_oracle_is_finite_and_a_usable_yardstick(family, form):
    per, top = _yardsticks(family, form)
    for c, x, t, w, kw, r64, r32, d in per:
        for q in H.QUANTITIES[family]:
            assert np.isfinite(np.asarray(r32[q], np.float64)).all() and np.isfinite(np.asarray(r64[q], np.float64)).all(), (
                H.describe(c, w, kw), q)
        if family == "eval":      # per image, no fall-back in tests/test_gpu_eval.py: the yardstick must not vanish
            r = np.abs(r32["loss_sum"].astype(np.float64) - r64["loss_sum"]) / np.abs(r64["loss_sum"])
            assert (r > 0).all(), H.describe(c, w, kw)
            # ... nor be a lucky rounding.  A scalar's distance can fall far below what float32 delivers when the oracle's
            # own errors cancel ("a lucky rounding"), and these images have some 200 to 3 700 pixels, not the
            # 4 096 to 263 169 of tests/test_gpu_eval.py.  The rule's factor 2 stands for another summation order, so the
            # yardstick has to be one that its summation dominates: at least twice the root-sum-square of the float32
            # oracle's own per-pixel errors, which is what those errors add up to when they do not cancel.  A condition
            # on the two oracle runs alone; a seed that breaks it is replaced (SALT), the rule stays.
            N = r64["logits"].shape[0]
            lab = t.reshape(r64["logits"].shape[:-1])
            e = (E.pixel_loss(r32["logits"], lab, np.float32).astype(np.float64) - E.pixel_loss(r64["logits"], lab)).reshape(N, -1)
            ww = np.ones_like(e) if w is None else w.reshape(N, -1).astype(np.float64)
            rss = np.sqrt(((ww * e) ** 2).sum(1)) / np.abs(r64["loss_sum"])
            assert (r >= 2.0 * rss).all(), (H.describe(c, w, kw), r, rss)
        # unary: where the distance is 0 (C = 1: U is -log 1 or -log of the mixed 1) the device test falls back to bit
        # equality with the float32 oracle, as _compare of tests/test_gpu_crf_unary.py does
        if family == "unary" and d["U"] == 0.0:
            assert c.C == 1, H.describe(c, w, kw)
    if family not in ("eval", "unary"):   # the families whose rule takes the largest distance over the form's cases
        for q, v in top.items():
            assert v > 0, (family, form, q)


# -------------------------------------------------------------------------------------------------------- (d) teeth
def _wrong_pad(case, x, t, w, kw, maxc):
    """the family's float32 oracle on rows padded to maxc with a logit of 0 that is NOT masked out of the maximum and the
    sum (the pad classes are real classes to it; void labels move out of range so that they stay void)"""
    from tests import crf_unary_oracle as UO
    C = case.C
    form, shape = H.oracle_form(case)
    if case.family == "unary":
        z = (UO.gather_bilinear(x, shape[0], shape[1], np.float32) if form == "bilinear" else
             UO.gather_shuffle(x, shape, np.float32) if form == "shuffle" else np.asarray(x, np.float32))
    else:
        z = E.full_logits(form, x, shape, np.float32)
    zp = np.concatenate([z, np.zeros(z.shape[:-1] + (maxc - C,), np.float32)], -1)
    tp = np.where(H.is_void(t, C), -1, t).astype(np.float32)
    kw = dict(kw)
    if kw.get("alpha") is not None:
        kw["alpha"] = np.concatenate([kw["alpha"], np.ones(maxc - C, np.float32)])
    r = H.reference(case.family, "plain", zp, None, tp, w, np.float32, **kw)
    cut = {"dlogits": lambda a: a[..., :C], "sums": lambda a: a[:, :C], "coef": lambda a: a[:, :C], "U": lambda a: a[:, :C]}
    return {q: cut.get(q, lambda a: a)(r[q]) for q in H.QUANTITIES[case.family]}


@pytest.mark.parametrize("family,form", _groups(), ids=lambda v: str(v))
def test_a_zero_pad_in_the_maximum_and_the_sum_is_caught(family, form):
    per, top = _yardsticks(family, form)
    checked = 0
    for c, x, t, w, kw, r64, r32, d in per:
        m = max(k[1] for k in H.kernels(c))
        if c.kind != "negative" or m <= c.C:
            continue   # an empty pad (C = 8, 24, 32 in their own bucket), or a kernel without a register row (MAXC 0)
        bad = _wrong_pad(c, x, t, w, kw, m)
        for q in H.QUANTITIES[family]:
            if q == "dlogits" and c.C == 1:
                # one class: p = 1 lies outside Keras' clip interval and p (G - p G) vanishes, the gradient is zero
                # whatever the softmax does — the slip shows in the other quantities of the same launch
                assert not np.asarray(r64[q]).any()
                continue
            # the margin of the device test: twice the float32 oracle's distance — of this input for the evaluation
            # tail and the CRF unary, the largest over the form's cases for the other families
            margin = 2.0 * (d[q] if family in ("eval", "unary") else top[q])
            miss = H.distance(q, bad[q], r64[q])
            assert miss > margin, (H.describe(c, w, kw), q, miss, margin)
        checked += 1
    entry_maxc = {H.maxc(e, C) for e in sum((list(H.entries(c)) for c in H.group(family, form)), []) for C in H.C_SWEEP}
    if entry_maxc == {0}:
        assert checked == 0   # dl3_pixel_xent_plain, dl3_eval_tail_plain: a loop over the classes in memory, no pad
    else:
        assert checked > 0, (family, form)
