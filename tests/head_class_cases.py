"""The case table of tests/test_gpu_head_classes.py: the six kernel families that decode the output head's class scores
(csrc/losstail.hip, both of its pixel terms, jaccard.hip, mine.hip, evaltail.hip, crfunary.hip) at every class-count
instantiation, and what a case needs on the host: its seeded inputs and the launch rules of those files restated in
Python.  Importable without a GPU: tests/test_head_class_cases_host.py checks the table here against the sources, the
references' own conditions and a deliberately wrong oracle.

A pixel's logits live in float z[MAXC] (csrc/tailmath.h); MAXC is chosen on the host and every <MAXC, form> pair is its
own compiled kernel.  C_SWEEP sits on both sides of each bucket edge: the pad (classes C..MAXC-1) is empty at C = 8, 24,
32, one register wide behind C = 8 and 24 (C = 9 -> 24 has 15, C = 25 -> 32 has 7), and everything but z[0] at C = 1."""
import zlib
from collections import namedtuple

import numpy as np

C_SWEEP = (1, 8, 9, 24, 25, 32)
KINDS = ("normal", "negative")
NEGATIVE_SHIFT = -30.0   # 'negative': the family's own draw moved so that every real logit lies in roughly [-40, -20]:
#                          a finite, well-conditioned softmax in which a pad logit of 0 is far above every class

# ------------------------------------------------------------------------------------------------ smallest shapes
PLAIN_HW = 257                       # two 256-pixel workgroups, the second with one pixel
BILINEAR = (2, 5, 7, 33, 19)         # (N, Hi, Wi, Ho, Wo): 5/33 and 7/19 are inexact in float32
BILINEAR_VEC = (2, 5, 7, 33, 20)     # Wo % 4 == 0: the evaluation tail's 16-byte variant (a lane owns four pixels)
SHUFFLE_TRAIN = (2, 2, 13, 4)        # (N, H, W, r): the training forms' tile cap of 8 pixels -> tiles of 8 and 5
SHUFFLE_TAIL = (1, 2, 29, 8)         # mining / evaluation / CRF-unary forms: shuffle_pb pixels per tile, see tiles()

# the family's own draw of the logits (standard deviation) and of the weights, as its test file has them
LOGIT_STD = {"xent": 3.0, "focal": 3.0, "jaccard": 3.0, "mine": 3.0, "eval": 1.0, "unary": 4.0}
PER_IMAGE = ("jaccard", "eval", "unary")   # families whose plain form takes [B][HW]: B = 1 and B = 2

# form -> entry point, per family
ENTRY = {
    "xent": {"plain": "dl3_softmax_xent", "bilinear": "dl3_upsample_softmax_xent",
             "fold": "dl3_upsample_softmax_xent_fold", "shuffle": "dl3_shuffle_softmax_xent"},
    "focal": {"plain": "dl3_focal_xent", "bilinear": "dl3_upsample_focal_xent",
              "fold": "dl3_upsample_focal_xent_fold", "shuffle": "dl3_shuffle_focal_xent"},
    "jaccard": {"plain": ("dl3_jaccard_sums_plain", "dl3_softmax_xent_jaccard"),
                "bilinear": ("dl3_jaccard_sums_bilinear", "dl3_upsample_softmax_xent_jaccard")},
    "mine": {"plain": "dl3_pixel_xent_plain", "bilinear": "dl3_pixel_xent_bilinear", "shuffle": "dl3_pixel_xent_shuffle"},
    "eval": {"plain": "dl3_eval_tail_plain", "bilinear": "dl3_eval_tail_bilinear", "shuffle": "dl3_eval_tail_shuffle"},
    "unary": {"plain": "dl3_crf_unary_plain", "bilinear": "dl3_crf_unary_bilinear", "shuffle": "dl3_crf_unary_shuffle"},
}


# ----------------------------------------------------------------------------------- launch rules, restated from csrc/
def dispatch_maxc(C):
    """DL3_DISPATCH_MAXC (csrc/common.h)"""
    return 8 if C <= 8 else 24 if C <= 24 else 32


def two_bucket_maxc(C):
    """the fold and the training shuffle launchers (launch_fold, launch_shuffle) pick by hand: <24> or <32>"""
    return 24 if C <= 24 else 32


# entry point -> (source file, the text of the launcher's choice, rule, the (MAXC, variant) pairs the source defines).
# MAXC 0: the kernel loops over the classes in memory, it has no register row and no pad (listed so that the table's
# coverage names every entry point; there is one kernel to reach).
_D = ((8, ""), (24, ""), (32, ""))
_T = ((24, ""), (32, ""))
_F = ((24, "pref"), (24, "nopref"), (32, "pref"), (32, "nopref"))
_V = tuple((m, v) for m in (8, 24, 32) for v in ("vec4", "scalar"))
KERNELS = {
    "dl3_softmax_xent": ("losstail.hip", "launch_rows<XentTerm, false>(", lambda C: 32, ((32, ""),)),
    "dl3_upsample_softmax_xent": ("losstail.hip", "launch_rows<XentTerm, true>(", lambda C: 32, ((32, ""),)),
    "dl3_upsample_softmax_xent_fold": ("losstail.hip", "launch_fold<XentTerm>(", two_bucket_maxc, _F),
    "dl3_shuffle_softmax_xent": ("losstail.hip", "launch_shuffle<XentTerm>(", two_bucket_maxc, _T),
    "dl3_focal_xent": ("losstail.hip", "launch_rows<FocalTerm, false>(", lambda C: 32, ((32, ""),)),
    "dl3_upsample_focal_xent": ("losstail.hip", "launch_rows<FocalTerm, true>(", lambda C: 32, ((32, ""),)),
    "dl3_upsample_focal_xent_fold": ("losstail.hip", "launch_fold<FocalTerm>(", two_bucket_maxc, _F),
    "dl3_shuffle_focal_xent": ("losstail.hip", "launch_shuffle<FocalTerm>(", two_bucket_maxc, _T),
    "dl3_jaccard_sums_plain": ("jaccard.hip", "DL3_DISPATCH_MAXC(C, DL3_JSUMS)", dispatch_maxc, _D),
    "dl3_jaccard_sums_bilinear": ("jaccard.hip", "DL3_DISPATCH_MAXC(C, DL3_JSUMS)", dispatch_maxc, _D),
    "dl3_softmax_xent_jaccard": ("jaccard.hip", "xent32_jaccard_kernel<false>", lambda C: 32, ((32, ""),)),
    "dl3_upsample_softmax_xent_jaccard": ("jaccard.hip", "xent32_jaccard_kernel<true>", lambda C: 32, ((32, ""),)),
    "dl3_pixel_xent_plain": ("mine.hip", "hipLaunchKernelGGL(pixel_plain_kernel", lambda C: 0, ((0, ""),)),
    "dl3_pixel_xent_bilinear": ("mine.hip", "DL3_DISPATCH_MAXC(C, DL3_PIX_BIL)", dispatch_maxc, _D),
    "dl3_pixel_xent_shuffle": ("mine.hip", "DL3_DISPATCH_MAXC(C, DL3_PIX_SHF)", dispatch_maxc, _D),
    "dl3_eval_tail_plain": ("evaltail.hip", "hipLaunchKernelGGL(eval_plain_kernel", lambda C: 0, ((0, ""),)),
    "dl3_eval_tail_bilinear": ("evaltail.hip", "DL3_DISPATCH_MAXC(C, DL3_EVAL_BIL_VEC)", dispatch_maxc, _V),
    "dl3_eval_tail_shuffle": ("evaltail.hip", "DL3_DISPATCH_MAXC(C, DL3_EVAL_SHF)", dispatch_maxc, _D),
    "dl3_crf_unary_plain": ("crfunary.hip", "DL3_DISPATCH_MAXC(C, DL3_UNARY)", dispatch_maxc, _D),
    "dl3_crf_unary_bilinear": ("crfunary.hip", "DL3_DISPATCH_MAXC(C, DL3_UNARY)", dispatch_maxc, _D),
    "dl3_crf_unary_shuffle": ("crfunary.hip", "DL3_DISPATCH_MAXC(C, DL3_UNARY)", dispatch_maxc, _D),
}


def fold_prefetches(Wi, Wo, C, pref_env):
    """the condition of launch_fold, the launcher of dl3_upsample_softmax_xent_fold and its focal twin (kPrefFloats = 12,
    kPrefPixels = 2; the test's device buffers are 16-byte aligned): pref_env is DL3_XENT_PREF, None when unset"""
    return (Wi * C <= 256 * 12 and Wo <= 256 * 2 and (Wi * C) % 4 == 0 and (Wo * C) % 4 == 0
            and not (pref_env is not None and int(pref_env) == 0))


def subpixel_tile_pixels(W, C, r, cap):
    """csrc/tailmath.h: pixels of one LDS tile"""
    return min((48 << 10) // (C * (r * r + 1) * 4), cap, W)


def shuffle_pb(W, C, r):
    return subpixel_tile_pixels(W, C, r, (1024 + r * r - 1) // (r * r))


def tiles(W, pb):
    """the tile widths of one row"""
    return [min(pb, W - x0) for x0 in range(0, W, pb)]


# ------------------------------------------------------------------------------------------------------ the cases
# family, form: ENTRY;  dims: plain (B, HW), bilinear (N, Hi, Wi, Ho, Wo), shuffle (N, H, W, r);  kind: KINDS;
# void: how a void pixel is written, "C" or "255/-1" (focal only: include/dl3.h, every label outside 0..C-1 is void);
# variant: the kernel variant the launcher's condition gives the case ("" where the entry point has one kernel per MAXC);
# pref_env: the value DL3_XENT_PREF has during the case (None: unset);  salt: added to the seed (a case that broke a
# reference-only condition gets another seed, never another bound)
Case = namedtuple("Case", "id family form dims C kind void variant pref_env salt")


def entries(case):
    e = ENTRY[case.family][case.form]
    return e if isinstance(e, tuple) else (e,)


def maxc(entry, C):
    return KERNELS[entry][2](C)


def kernels(case):
    """the (entry point, MAXC, variant) triples the case launches"""
    return [(e, maxc(e, case.C), case.variant if any(v for _, v in KERNELS[e][3]) else "") for e in entries(case)]


# cases whose first seed broke a reference-only condition of tests/test_head_class_cases_host.py (b)
SALT = {
    # a pixel on the edge of Keras' clip interval, where float32 and float64 decide the gradient differently
    "jaccard-bilinear-2x5x7x33x19-C9-negative": 1,
    # the evaluation tail, whose rule holds every image to twice ITS OWN yardstick: seeds at which the float32 oracle's
    # loss_sum is a lucky rounding (closer to float64 than twice the root-sum-square of its own per-pixel errors, condition
    # (c) of the host file) or at which more than 0.1 % of the pixels are undecidable; the smallest salt that meets both
    "eval-plain-1x257-C8-normal": 2, "eval-plain-1x257-C8-negative": 1, "eval-plain-2x257-C8-negative": 4,
    "eval-plain-1x257-C9-normal": 2, "eval-plain-1x257-C9-negative": 1, "eval-plain-2x257-C9-negative": 1,
    "eval-plain-2x257-C24-normal": 2, "eval-plain-2x257-C24-negative": 1, "eval-plain-2x257-C25-negative": 1,
    "eval-plain-2x257-C32-normal": 2,
    "eval-bilinear-2x5x7x33x20-C8-normal-vec4": 1, "eval-bilinear-2x5x7x33x19-C8-negative-scalar": 22,
    "eval-bilinear-2x5x7x33x20-C8-negative-vec4": 28, "eval-bilinear-2x5x7x33x20-C9-normal-vec4": 1,
    "eval-bilinear-2x5x7x33x19-C9-negative-scalar": 4, "eval-bilinear-2x5x7x33x20-C9-negative-vec4": 15,
    "eval-bilinear-2x5x7x33x20-C24-negative-vec4": 18, "eval-bilinear-2x5x7x33x19-C25-negative-scalar": 22,
    "eval-bilinear-2x5x7x33x20-C25-negative-vec4": 4, "eval-bilinear-2x5x7x33x20-C32-normal-vec4": 1,
    "eval-bilinear-2x5x7x33x19-C32-negative-scalar": 7, "eval-bilinear-2x5x7x33x20-C32-negative-vec4": 2,
    "eval-shuffle-1x2x29x8-C9-negative": 1, "eval-shuffle-1x2x29x8-C25-normal": 1, "eval-shuffle-1x2x29x8-C32-normal": 1,
}


def _mk(family, form, dims, C, kind, void="C", variant="", pref_env=None):
    cid = "%s-%s-%s-C%d-%s" % (family, form, "x".join(map(str, dims)), C, kind)
    if void != "C":
        cid += "-void255"
    if variant:
        cid += "-" + variant
    return Case(cid, family, form, tuple(dims), C, kind, void, variant, pref_env, SALT.get(cid, 0))


def _family_cases(family):
    out = []
    for form in ENTRY[family]:
        for C in C_SWEEP:
            for kind in KINDS:
                if form == "plain":
                    for B in ((1, 2) if family in PER_IMAGE else (1,)):
                        out.append(_mk(family, form, (B, PLAIN_HW), C, kind))
                elif form == "bilinear":
                    if family == "eval":
                        out.append(_mk(family, form, BILINEAR, C, kind, variant="scalar"))
                        out.append(_mk(family, form, BILINEAR_VEC, C, kind, variant="vec4"))
                    else:
                        out.append(_mk(family, form, BILINEAR, C, kind))
                elif form == "fold":
                    # DL3_XENT_PREF=0 for one run, unset for the other: the variant follows from the launcher's condition
                    for env in ("0", None):
                        v = "pref" if fold_prefetches(BILINEAR[2], BILINEAR[4], C, env) else "nopref"
                        if env is None and v == "nopref":
                            continue   # C = 1, 9, 25 at Wi = 7: the same kernel as the run with the variable set
                        out.append(_mk(family, form, BILINEAR, C, kind, variant=v, pref_env=env))
                else:
                    dims = SHUFFLE_TRAIN if family in ("xent", "focal") else SHUFFLE_TAIL
                    out.append(_mk(family, form, dims, C, kind))
        if family == "focal":   # one case per form whose void pixels are 255 and -1 instead of C
            dims = {"plain": (1, PLAIN_HW), "bilinear": BILINEAR, "fold": BILINEAR, "shuffle": SHUFFLE_TRAIN}[form]
            out.append(_mk(family, form, dims, 25, "negative", void="255/-1",
                           variant="nopref" if form == "fold" else ""))
    return out


FAMILIES = tuple(ENTRY)
CASES = {f: _family_cases(f) for f in FAMILIES}
ALL = [c for f in FAMILIES for c in CASES[f]]


def group(family, form):
    return [c for c in CASES[family] if c.form == form]


# ------------------------------------------------------------------------------------------------------ the inputs
def pixels(case):
    """(images, pixels per image) at the full resolution"""
    d = case.dims
    if case.form == "plain":
        return d
    if case.form in ("bilinear", "fold"):
        return d[0], d[3] * d[4]
    return d[0], d[1] * d[3] * d[2] * d[3]


def x_shape(case):
    d, C = case.dims, case.C
    if case.form == "plain":
        return (d[0], 1, d[1], C)
    if case.form in ("bilinear", "fold"):
        return (d[0], d[1], d[2], C)
    return (d[0], d[1], d[2], C * d[3] * d[3])


def oracle_form(case):
    """(form, shape) as tests/eval_oracle.py full_logits takes them"""
    d = case.dims
    if case.form == "plain":
        return "plain", None
    if case.form in ("bilinear", "fold"):
        return "bilinear", (d[3], d[4])
    return "shuffle", d[3]


def seed(case):
    """from the id; the two variants of a fold case share their input (they must agree bit for bit)"""
    key = case.id[:-len(case.variant) - 1] if case.form == "fold" and case.variant else case.id
    return (zlib.crc32(key.encode()) + case.salt) & 0x7FFFFFFF


def labels(case):
    """[B, HW] float32: about one pixel in eight is void; the others cycle through 0..C-1, each image starting one class
    further, so that every class — C - 1 included — is the label of some pixel of every image.  Jaccard keeps its
    generator's property that some class is absent from some image: class 0 from image 0, where there is a second image."""
    B, HW = pixels(case)
    C = case.C
    i = np.arange(HW)
    void = i % 8 == 5
    rank = np.cumsum(~void) - 1
    t = np.empty((B, HW), np.float32)
    for b in range(B):
        t[b] = (rank + b) % C
        if case.void == "C":
            t[b][void] = C
        else:
            t[b][void] = np.where(i[void] % 16 == 5, 255.0, -1.0)
    if case.family == "jaccard" and B > 1:
        t[0][t[0] == 0] = C
    return t


def inputs(case):
    """-> x (float32, x_shape), labels [B,HW], weights [B,HW] (the test also runs the null weights pointer)"""
    rng = np.random.default_rng(seed(case))
    x = (rng.standard_normal(x_shape(case)) * LOGIT_STD[case.family]).astype(np.float32)
    if case.kind == "negative":
        x = (x + np.float32(NEGATIVE_SHIFT)).astype(np.float32)
    B, HW = pixels(case)
    if case.family == "eval":    # tests/test_gpu_eval.py: uniform weights, a quarter of them zero
        w = rng.random((B, HW)) * (rng.random((B, HW)) > 0.25)
    else:                        # the loss families: [0.5, 2), a fifth of them zero
        w = rng.uniform(0.5, 2.0, (B, HW)) * (rng.random((B, HW)) > 0.2)
    return x, labels(case), w.astype(np.float32)


def alpha(case):
    """the focal families' per-class weights, uniform in [0.5, 2]"""
    return np.random.default_rng(seed(case) ^ 0x5A5A).uniform(0.5, 2.0, case.C).astype(np.float32)


def is_void(t, C):
    t = np.asarray(t)
    return (t < 0) | (t >= C)


# ------------------------------------------------------------------------------------------------- the references
# the float results each family's own test file puts under the yardstick (device distance from the float64 oracle at most
# twice the float32 oracle's own); everything else a family returns is an integer or a mask and compared exactly
QUANTITIES = {"xent": ("loss", "dlogits"), "focal": ("loss", "dlogits"), "jaccard": ("sums", "coef", "lj", "dlogits"),
              "mine": ("v",), "eval": ("loss_sum",), "unary": ("U",)}
GAMMAS = (0.5, 2.0)          # tests/test_gpu_focal.py
LAMBDA = 0.75                # tests/test_gpu_jaccard.py
SCALES_CLIPS = ((0.0, 0.0), (0.0, 1e-5), (0.5, 0.0), (0.5, 1e-5))   # tests/test_gpu_crf_unary.py SCALES x CLIPS


def reference(family, form, x, shape, t, w, dtype, gamma=2.0, alpha=None, scale=0.0, clip=0.0):
    """one family's existing oracle on one input -> dict.  form / x / shape as tests/eval_oracle.py full_logits takes them,
    so that a test can hand in full-resolution logits of its own as ("plain", z, None)."""
    from tests import eval_oracle as E
    if family == "xent":
        from tests import ops_oracle as OO
        z = E.full_logits(form, x, shape, dtype)
        C = z.shape[-1]
        z = z.reshape(-1, C)
        tt = np.asarray(t).reshape(-1)
        nnz = max(tt.size if w is None else int((np.asarray(w) != 0).sum()), 1)
        r = OO.softmax_xent(z, tt, None if w is None else np.asarray(w).reshape(-1), nnz, dt=dtype)
        loss = float(r["l"].astype(np.float64).sum()) if dtype == np.float64 else float(np.cumsum(r["l"], dtype=dtype)[-1])
        return dict(loss=loss, dlogits=r["dl"].reshape(np.asarray(t).shape + (C,)), logits=z)
    if family == "focal":
        from tests import focal_oracle as F
        return F.evaluate(form, x, shape, t, w, gamma, alpha, dtype)
    if family == "jaccard":
        from tests import jaccard_oracle as J
        return J.evaluate(form, x, shape, t, w, LAMBDA, dtype)
    if family == "mine":
        from tests import mine_oracle as M
        return dict(v=M.pixel_v(form, x, shape, t, w, dtype))
    if family == "eval":
        return E.eval_tail(form, x, shape, t, w, dtype)
    if family == "unary":
        from tests import crf_unary_oracle as UO
        xx = np.asarray(x).reshape(x.shape[0], -1, x.shape[-1]) if form == "plain" else x
        return dict(U=UO.unary(form, xx, shape, False, scale or None, clip or None, dtype))
    raise ValueError(family)


def distance(q, a, b):
    """the family's own distance of quantity q: the largest absolute difference (the Jaccard sums: I and S, Y is exact)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if q == "sums":
        a, b = a[..., :2], b[..., :2]
    if q == "loss_sum":   # tests/test_gpu_eval.py: relative, per image
        return float((np.abs(a - b) / np.abs(b)).max())
    if q == "U":          # tests/test_gpu_crf_unary.py: over the largest |U| (all zero at C = 1 without scale: absolute)
        return float(np.abs(a - b).max() / (np.abs(b).max() or 1.0))
    return float(np.abs(a - b).max())


def variants(case):
    """the keyword sets one case is run with besides its two weightings: focal (gamma, alpha), unary (scale, clip)"""
    if case.family == "focal":
        a = alpha(case)
        return [dict(gamma=g, alpha=al) for g in GAMMAS for al in (None, a)]
    if case.family == "unary":
        return [dict(scale=s, clip=c) for s, c in SCALES_CLIPS]
    return [dict()]


def weightings(case, w):
    return (None,) if case.family == "unary" else (w, None)


def runs(case):
    """every run of one case: (x, labels, weights or None, keywords, float64 reference, float32 reference)"""
    x, t, w = inputs(case)
    form, shape = oracle_form(case)
    for ww in weightings(case, w):
        for kw in variants(case):
            yield (x, t, ww, kw, reference(case.family, form, x, shape, t, ww, np.float64, **kw),
                   reference(case.family, form, x, shape, t, ww, np.float32, **kw))


def describe(case, w, kw):
    s = case.id + (" weighted" if w is not None else " unweighted")
    for k, v in sorted(kw.items()):
        s += " %s=%s" % (k, "array" if isinstance(v, np.ndarray) else v)
    return s
