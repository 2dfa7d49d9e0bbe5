"""The case table of tests/test_gpu_pwconv.py (the 1x1-convolution GEMMs: csrc/pwstream.hip, pwlds.hip, pwws.hip, pwsmall.hip,
pwwgrad.hip, pwfused.hip behind the planner csrc/pwplan.h) and what a case needs on the host: its seeded operands, its
reference, the exactness conditions, and the launch description tools/pwplan_probe.cpp is asked with.  Importable without a
GPU: tests/test_pwconv_cases_host.py checks the table here against the planner itself.

EXACT cases (Case.exact).  Every operand is a small integer (invstd: 0.5, 1 or 2): the input x, the transform (scale 1 or 2,
integer shift), the weights (-1, 0, 1 at density Case.wd), the bias, g, yraw, cA / cB / cC, the addend and add_scale = 2, the
mean.  Every product is then an integer (a multiple of 0.5 in sum(v * xhat)), and where the sum of the ABSOLUTE values of the
terms of a sum stays below 2**24 (2**23 for the multiples of 0.5) every partial sum in every order is an integer below 2**24
too: fp32 holds it exactly, on the f32 MFMA, as 3 x bf16 split math (|operand| <= 256: one bf16 piece) and in the folds.  The
device must therefore return the reference's VALUES, compared with ==.  `conditions()` evaluates those sums of absolute values
from the operands alone; the host test asserts them for every exact case.  The references of the exact cases are evaluated in
fp32: under the same conditions fp32 BLAS is exact as well — and a sum of non-negative terms that reaches 2**24 never rounds
back below it, so the fp32 value of a condition is below 2**24 exactly when the true one is (the host test also compares the
fp32 references with float64 ones on every case of at most 8 192 rows).

REAL-VALUED cases (exact = False): normal operands of the older tests; outputs are held element-wise to
ops_oracle.assert_reduction with the abs-sum sum_k |a_k||b_k| + |bias| + |addend| and a chain of K + 4, sums and weight
gradients per channel to 1e-3 of the sum of the absolute terms (the bar of tests/test_gpu_dwconv.py).

PLANS[id] is the plan the case is there for — kernel, instantiation, launches, partial rows / slabs and which of its last
row, column and K tiles are whole (=) or ragged (<) — in the words of `describe()`; it is what tools/pwplan_probe.cpp printed
when the case was written, and the host test fails when the planner answers anything else."""
import zlib
from collections import namedtuple

import numpy as np

LIM = float(2 ** 24)
ACT_NAME = {0: "", 1: "relu", 2: "relu6"}

# entry: fwd (dl3_pwconv_fwd, or _fwd_add when add), bwd_data, bwd_weight (dl3_pwconv_bwd_weight, or _dy when dy_out), fused
# M, K, N: the LAYER's rows, input and output channels (bwd-data reduces over N and is K wide)
# form / act: the input transform ("none", "affine", "act", "affine+act"; act 1 relu, 2 relu6) — forward operand transform,
#   activation mask of bwd-data / fused, operand transform of the weight gradient
# two: two-tensor dY (cA*g + cB*yraw + cC);  add: 0 none, 1 a tensor of the output's shape, 2 one row per ADD_DIV rows
# stats: statistic partials asked for (fused: 1 sums against x, 2 against another tensor);  bias: forward bias
# dy_out: the weight-gradient launch writes dY;  dbias: ... and the bias gradient;  slabs: dw == NULL, the caller folds
# lay: ((operand, column offset, extra leading dimension), ...) for x, g (yraw shares it), y / dx (the addend shares it), dy;
#   ("mis",): every operand one float off its 16-byte boundary
# knobs: ((name, value), ...) of the environment for the launch (DL3_GEMM_CFG, DL3_WGRAD_CFG, DL3_GEMM_PRE, DL3_GEMM_MATH,
#   DL3_FUSED_V: all read per call)
# exact: see above;  wd: density of the non-zero weights
Case = namedtuple("Case", "id entry M K N form act two add stats bias dy_out dbias slabs lay knobs exact wd")
ADD_DIV = 64


def _c(id, entry, M, K, N, form="none", act=0, two=False, add=0, stats=True, bias=False, dy_out=False, dbias=False, slabs=False,
       lay=(), knobs=(), exact=True, wd=1.0):
    assert (act != 0) == form.endswith("act"), id
    return Case(id, entry, M, K, N, form, act, two, add, stats, bias, dy_out, dbias, slabs, tuple(lay), tuple(knobs), exact, wd)


GEMM_TILES = {0: (128, 128), 1: (256, 64), 2: (256, 32), 3: (128, 160), 4: (128, 96), 5: (32, 256), 6: (32, 128)}   # kGemmCfgs
WGRAD_TILES = {0: (64, 64), 1: (128, 128), 2: (160, 128), 3: (128, 160), 4: (64, 128), 5: (128, 64), 6: (32, 128), 7: (128, 32),
               8: (96, 128), 9: (128, 96)}                                                                              # kWgCfgs
FORMS3 = (("affine+act", 2), ("act", 1), ("affine", 0))


# ---- the stream kernel under every tile configuration: one whole tile, a ragged last row tile, a ragged last column tile, two
# whole K-tiles and a ragged third; forward / single-tensor bwd-data / two-tensor bwd-data; f32 MFMA and split math -----------
def _stream():
    out = []
    for cfg, (bm, bn) in GEMM_TILES.items():
        m, n = bm + 37, bn + 36
        for math in ("f32", "split"):
            if math == "split" and cfg >= 5:
                continue   # (the 32-row tiles keep the f32 MFMA: plan_gemm_one)
            k = 40 if math == "f32" else 72
            kn = (("DL3_GEMM_CFG", str(cfg)),) + ((("DL3_GEMM_MATH", "split"),) if math == "split" else ())
            tag = "stream%s-cfg%d" % ("-split" if math == "split" else "", cfg)
            f, a = FORMS3[cfg % 3]
            out.append(_c(tag + "-fwd", "fwd", m, k, n, f, a, bias=cfg % 2 == 0, knobs=kn))
            # (a residual keeps cfg 4 off the prefetching instantiation, which has cases of its own)
            out.append(_c(tag + "-bwd1", "bwd_data", m, n, k, *FORMS3[(cfg + 1) % 3], add=1, knobs=kn))
            out.append(_c(tag + "-two", "bwd_data", m, n, k, *FORMS3[(cfg + 2) % 3], two=True, add=2 if cfg % 2 else 1, knobs=kn))
    # the prefetching 128x96 tile (EPI 2): forced at a few hundred rows, single- and two-tensor dY, f32 and split
    for math in ("f32", "split"):
        kn = (("DL3_GEMM_CFG", "4"),) + ((("DL3_GEMM_MATH", "split"),) if math == "split" else ())
        k = 40 if math == "f32" else 72
        tag = "stream%s-pre" % ("-split" if math == "split" else "")
        out.append(_c(tag + "-bwd1", "bwd_data", 128 * 2 + 37, 96 + 36, k, "affine+act", 2, knobs=kn))
        out.append(_c(tag + "-two", "bwd_data", 128 + 5, 96 * 2, k, "act", 1, two=True, knobs=kn))
    # ... with whole tiles only (the generic epilogue never runs) and with DL3_GEMM_PRE=0 (the generic epilogue only)
    out.append(_c("stream-pre-whole", "bwd_data", 256, 96, 32, "affine+act", 2, knobs=(("DL3_GEMM_CFG", "4"),)))
    out.append(_c("stream-pre-off", "bwd_data", 128 * 2 + 37, 96 + 36, 40, "affine+act", 2,
                  knobs=(("DL3_GEMM_CFG", "4"), ("DL3_GEMM_PRE", "0"))))
    # forward with an addend: one row per 64-row image (the straight-line epilogue takes it) and a residual tensor
    out.append(_c("stream-fwd-add-image64", "fwd", 128 + 64, 40, 128 + 36, "affine", add=2, knobs=(("DL3_GEMM_CFG", "0"),)))
    out.append(_c("stream-fwd-add-tensor", "fwd", 128 + 37, 40, 128 + 36, "act", 1, add=1, bias=True, knobs=(("DL3_GEMM_CFG", "0"),)))
    # no statistic partials, slices of wider buffers on every operand
    out.append(_c("stream-fwd-slices-no-stats", "fwd", 300, 64, 96, "affine+act", 2, stats=False, lay=(("x", 8, 4), ("y", 4, 12))))
    out.append(_c("stream-bwd-slices", "bwd_data", 300, 96, 64, "affine+act", 1, two=True, add=1,
                  lay=(("x", 4, 4), ("g", 8, 0), ("dx", 12, 4))))
    return out


# ---- the LDS-staged kernel: cfg 0-4 x load mode 0 (scalar loads: every operand off its boundary), 2 (N no multiple of 4) and
# 1 (16-byte loads on both: a reduction beyond DL3_STREAM_KMAX, K = 2052 / 2304), forward and bwd-data each ------------------------
def _lds():
    out = []
    for cfg in range(5):
        bm, bn = GEMM_TILES[cfg]
        m = bm + 37
        kn = (("DL3_GEMM_CFG", str(cfg)),)
        f, a = FORMS3[cfg % 3]
        g, b = FORMS3[(cfg + 1) % 3]
        big = 2052 if cfg % 2 == 0 else 2304
        out += [
            _c("lds-cfg%d-mode0-fwd" % cfg, "fwd", m, 40, bn + 36, f, a, bias=True, lay=(("mis",),), knobs=kn),
            _c("lds-cfg%d-mode0-bwd" % cfg, "bwd_data", m, bn + 36, 40, g, b, two=True, add=1, lay=(("mis",),), knobs=kn),
            _c("lds-cfg%d-mode2-fwd" % cfg, "fwd", m, 40, bn + 35, f, a, bias=cfg % 2 == 1, knobs=kn),
            _c("lds-cfg%d-mode2-bwd" % cfg, "bwd_data", m, bn + 35, 40, g, b, two=cfg % 2 == 0, add=2, knobs=kn),
            _c("lds-cfg%d-mode1-fwd" % cfg, "fwd", m, big, bn + 36, f, a, bias=True, knobs=kn),
            _c("lds-cfg%d-mode1-bwd" % cfg, "bwd_data", m, bn + 36, big, g, b, two=cfg % 2 == 1, add=cfg % 3, knobs=kn),
        ]
    # the planner's own pick for a long reduction, whole tiles only
    out.append(_c("lds-mode1-auto-whole", "fwd", 256, 2304, 64, "affine+act", 2, bias=True))
    return out


# ---- the K-split kernel (1 024 - 16 384 rows, reduction >= 192, 64- / 96- / 160-wide output): tn 2 / 3 / 5 x two --------------------
KSPLIT = [
    _c("ksplit-tn2-fwd", "fwd", 1024, 192, 64, "affine+act", 2),
    _c("ksplit-tn3-fwd-ragged", "fwd", 1024 + 19, 196, 96, "act", 1, bias=True),
    _c("ksplit-tn5-fwd-ragged-columns", "fwd", 1056 + 7, 200, 132, "affine", bias=True, add=1),
    _c("ksplit-tn5-bwd1", "bwd_data", 1024 + 40, 160, 192, "affine+act", 2),
    _c("ksplit-tn3-bwd1-add", "bwd_data", 1024, 96, 256, "act", 1, add=2),
    _c("ksplit-tn2-two", "bwd_data", 1024 + 5, 64, 192, "affine+act", 1, two=True, add=1),
    _c("ksplit-tn3-two", "bwd_data", 1030, 92, 196, "none", two=True),
    _c("ksplit-tn5-two", "bwd_data", 1024, 160, 320, "affine+act", 2, two=True, add=2),
]

# ---- pw_fwd_ws_kernel (route 1, from 32 768 rows): all seven (KQ, TN), whole and with a ragged last 32-column block — the
# widths of alpha != 1 and of other class counts (16 -> 80, 24 -> 136, 32 -> 24, 32 -> 172, 96 -> 16, 144 -> 20, 192 -> 28) ---------
WS = [_c("ws-%dx%d-%s" % (k, n, "whole" if r == 0 else "ragged"), "fwd", 32768 + r, k, n, *FORMS3[i % 3], bias=i % 2 == 1, lay=lay, wd=wd)
      for i, (k, n, r, lay, wd) in enumerate([
          (16, 96, 0, (), 0.5), (16, 80, 13, (), 1.0), (24, 160, 0, (), 0.4), (24, 136, 5, (), 0.35), (32, 32, 0, (), 1.0),
          (32, 24, 31, (), 0.25), (32, 192, 0, (), 0.4), (32, 172, 1, (), 1.0), (96, 32, 0, (), 0.08),
          (96, 16, 17, (("x", 8, 0),), 0.25), (144, 32, 0, (), 0.25), (144, 20, 9, (("y", 0, 12),), 0.1), (192, 32, 0, (), 0.08),
          (192, 28, 3, (), 0.3)])]
WS.append(_c("ws-32x172-1250-partial-rows", "fwd", 40000, 32, 172, "affine+act", 2, wd=0.25))

# ---- pw_ws2_kernel: forward and bwd-data at tn 3 / 4 / 5 at the route's row threshold and its narrowest output, the 384 -> 64
# two-tensor form with and without residual, the packed logits forward (FLAT); pw_narrowk_kernel ------------------------------------------
WS2 = [
    _c("ws2-fwd-tn3", "fwd", 98304, 96, 192, "affine+act", 2, wd=0.03),
    _c("ws2-fwd-tn3-ragged", "fwd", 98304 + 7, 96, 200, "act", 1, bias=True, wd=0.08),
    _c("ws2-fwd-tn4", "fwd", 131072 + 33, 64, 128, "affine+act", 2, lay=(("x", 64, 0),), wd=0.03),
    _c("ws2-fwd-tn5", "fwd", 98304 + 1, 160, 320, "affine", lay=(("y", 0, 64),), wd=0.015),
    _c("ws2-bwd-tn3", "bwd_data", 65536 + 40, 192, 96, "affine+act", 2, wd=0.5),
    _c("ws2-bwd-tn4", "bwd_data", 131072, 128, 64, "act", 1, wd=0.5),
    _c("ws2-bwd-tn4-ragged-columns", "bwd_data", 131072 + 9, 136, 64, "affine+act", 2, wd=0.5),
    _c("ws2-bwd-tn5", "bwd_data", 65536 + 7, 320, 160, "affine", wd=0.25),
    _c("ws2-bwd-tn5-no-stats", "bwd_data", 65536, 320, 160, "affine+act", 2, stats=False, wd=0.25),
    _c("ws2-bwd-384to64", "bwd_data", 131072 + 50, 64, 384, "affine+act", 2, two=True, wd=0.04),
    _c("ws2-bwd-384to64-add", "bwd_data", 131072, 64, 384, "act", 1, two=True, add=1, wd=0.04),
    _c("flat-logits-21", "fwd", 8192 + 5, 256, 21, "affine+act", 1, bias=True, wd=0.25),
    _c("flat-logits-32-no-stats", "fwd", 8192, 256, 32, "act", 2, stats=False),
    _c("narrowk-21", "bwd_data", 16384 + 9, 256, 21, stats=False),
    _c("narrowk-32", "bwd_data", 16384, 256, 32, stats=False),
]

# ---- shapes above a row threshold that the benchmarked networks do not have -----------------------------------------------------------
OFF_BENCH = [
    # the prefetching 128x96 tile with 80 of its 96 columns (bwd-data 480 <- 80: the cost model's own pick)
    _c("pre-480to80-partial-column-tile", "bwd_data", 65536 + 5, 80, 480, "affine+act", 2, wd=0.125),
    _c("pre-480to80-two", "bwd_data", 65536, 80, 480, "act", 1, two=True, wd=0.0625),
    _c("pre-96to48-whole", "bwd_data", 65536, 96, 48, "affine+act", 2, wd=0.5),
    # the column split (23 blocks of 32): two launches into one output and one set of partial rows
    _c("colsplit-fwd", "fwd", 32768 + 64, 256, 608, "affine+act", 2, wd=0.04),
    _c("colsplit-bwd1", "bwd_data", 32768, 608, 256, "act", 1, wd=0.125),
]


# ---- the tiled weight-gradient kernel: cfg 0-9 x load mode 1 / 0 / 2 and split math; K and N ragged against the tile, M no
# multiple of the 16-row stage ------------------------------------------------------------------------------------------------------------
def _wgrad():
    out = []
    for cfg, (bk, bn) in WGRAD_TILES.items():
        kn = (("DL3_WGRAD_CFG", str(cfg)),)
        f, a = FORMS3[cfg % 3]
        g, b = FORMS3[(cfg + 1) % 3]
        k, n = bk + 20, bn + 36
        out += [
            _c("wgrad-cfg%d-mode1" % cfg, "bwd_weight", 100, k, n, f, a, two=True, dy_out=cfg % 2 == 0, knobs=kn),
            _c("wgrad-cfg%d-mode0" % cfg, "bwd_weight", 100, k - 1, n, g, b, two=cfg % 2 == 1, dbias=cfg % 2 == 0, knobs=kn),
            _c("wgrad-cfg%d-mode2" % cfg, "bwd_weight", 100, k, n - 1, f, a, two=cfg % 2 == 0, dbias=cfg % 2 == 1, knobs=kn),
            _c("wgrad-cfg%d-split" % cfg, "bwd_weight", 100, k, n, g, b, two=True, dy_out=cfg % 2 == 1,
               knobs=kn + (("DL3_GEMM_MATH", "split"),)),
        ]
    out += [
        _c("wgrad-whole-tiles", "bwd_weight", 64, 128, 128, "affine+act", 2, two=True, dy_out=True, knobs=(("DL3_WGRAD_CFG", "1"),)),
        _c("wgrad-less-than-a-stage", "bwd_weight", 7, 160, 128, "affine", two=True, dy_out=True, knobs=(("DL3_WGRAD_CFG", "2"),)),
        _c("wgrad-slabs-left", "bwd_weight", 1040, 96, 24, "affine+act", 2, two=True, slabs=True),
        _c("wgrad-mode0-misaligned", "bwd_weight", 100, 64, 64, "act", 1, two=True, lay=(("mis",),)),
        _c("wgrad-slices-dy", "bwd_weight", 300, 64, 96, "affine+act", 2, two=True, dy_out=True,
           lay=(("x", 8, 4), ("g", 4, 4), ("dy", 0, 8))),
    ]
    return out


# ---- pw_wgrad_row_kernel (from 32 768 rows, K within one tile row of cfg 2 / 8): K below the tile row — 80 -> 480 is the expand
# convolution of alpha = 0.5 — and the whole tile rows 160 / 96; with and without the dY store, two-tensor and single dY -----------------
ROW = [
    _c("row-80x480-two-dy", "bwd_weight", 65536 + 9, 80, 480, "affine+act", 2, two=True, dy_out=True),
    _c("row-80x480-single", "bwd_weight", 65536, 80, 480, "act", 1, dbias=True),
    _c("row-88x528-two", "bwd_weight", 32768 + 5, 88, 528, "affine", two=True),
    _c("row-88x528-single-dy", "bwd_weight", 32768, 88, 528, "affine+act", 2, dy_out=True, lay=(("dy", 0, 8),)),
    _c("row-136x816-two-dy", "bwd_weight", 32768 + 3, 136, 816, "act", 1, two=True, dy_out=True),
    _c("row-136x816-single", "bwd_weight", 32768, 136, 816, "affine+act", 2),
    _c("row-152x912-two", "bwd_weight", 32768 + 17, 152, 912, "affine+act", 1, two=True, slabs=True),
    _c("row-152x912-single-dy", "bwd_weight", 32768, 152, 912, "affine", dy_out=True),
    _c("row-160x328-whole-row-two-dy", "bwd_weight", 32768, 160, 328, "affine+act", 2, two=True, dy_out=True),
    _c("row-96x576-whole-row-single", "bwd_weight", 32768 + 9, 96, 576, "none"),
    _c("row-160x384-whole-tiles-two-dy", "bwd_weight", 32768, 160, 384, "affine+act", 1, two=True, dy_out=True),
    _c("wgrad-narrow-21", "bwd_weight", 131072 + 7, 256, 21, "affine+act", 1, dbias=True),
    _c("wgrad-narrow-32", "bwd_weight", 131072, 256, 32, "act", 2),
]


# ---- dl3_pwconv_bwd_fused: every (K blocks, N blocks, auxiliary operand) instantiation of the round-5 kernel and of the
# round-4 one (DL3_FUSED_V=1); whole and partial last blocks; fewer rows than a stage, whole stages only -------------------------------
def fused_shapes(version):
    return sorted((kb, nb, aux) for kb in range(1, 7) for nb in range(1, 7) for aux in (False, True)
                  if kb * nb <= (5 if version == 1 else 6) and (not aux or kb <= 2))


def _fused():
    out = []
    for version in (2, 1):
        for i, (kb, nb, aux) in enumerate(fused_shapes(version)):
            k = 32 * kb - (0 if i % 2 else 4 * (1 + i % 5))
            n = 32 * nb - (0 if i % 3 else 4 * (1 + i % 7))
            m = (64, 203, 20, 32 * 7 + 1)[i % 4]
            f, a = FORMS3[i % 3]
            # an auxiliary operand: a residual addend, sums against another tensor than x, or both
            add = 1 if aux and i % 2 == 0 else 0
            st = (1 if add and i % 3 == 2 else 2) if aux else (1 if i % 5 else 0)
            out.append(_c("fused%s-%dx%d%s" % ("-v1" if version == 1 else "", kb, nb, "-aux" if aux else ""), "fused", m, k, n, f, a,
                          two=i % 4 != 3, add=add, stats=st, slabs=i % 6 == 5,
                          knobs=(("DL3_FUSED_V", "1"),) if version == 1 else ()))
    out.append(_c("fused-more-stages-than-workgroups", "fused", 40000 + 3, 24, 144, "affine+act", 2, two=True, add=1, stats=2))
    return out


# ---- real-valued cases (B): normal operands at the off-benchmark shapes and at the split-math forms ---------------------------------------
REAL = [
    _c("real-stream-fwd", "fwd", 300, 160, 164, "affine+act", 2, bias=True, exact=False),
    # split math at its own bar (the 32-row tiles the planner picks for a few hundred rows keep the f32 MFMA: a tile is forced,
    # or the rows are enough for a 128-row one)
    _c("real-stream-split-fwd", "fwd", 300, 160, 164, "affine+act", 2, bias=True,
       knobs=(("DL3_GEMM_CFG", "0"), ("DL3_GEMM_MATH", "split")), exact=False),
    _c("real-stream-split-two", "bwd_data", 300, 164, 160, "affine+act", 1, two=True, add=1,
       knobs=(("DL3_GEMM_CFG", "3"), ("DL3_GEMM_MATH", "split")), exact=False),
    _c("real-stream-split-bwd1-pre", "bwd_data", 300, 132, 160, "affine+act", 2,
       knobs=(("DL3_GEMM_CFG", "4"), ("DL3_GEMM_MATH", "split")), exact=False),
    _c("real-stream-split-auto", "bwd_data", 65536 + 8, 160, 960, "affine+act", 2, two=True, knobs=(("DL3_GEMM_MATH", "split"),),
       exact=False),
    _c("real-stream-two", "bwd_data", 300, 164, 160, "affine+act", 1, two=True, add=1, exact=False),
    _c("real-lds-mode1-fwd", "fwd", 165, 2052, 100, "act", 1, bias=True, exact=False),
    _c("real-lds-mode1-bwd", "bwd_data", 165, 100, 2304, "affine+act", 2, two=True, exact=False),
    _c("real-ksplit-fwd", "fwd", 1043, 196, 96, "act", 1, bias=True, exact=False),
    _c("real-ws-32x172", "fwd", 32768 + 1, 32, 172, "affine+act", 2, exact=False),
    _c("real-ws2-fwd", "fwd", 98304 + 7, 96, 200, "act", 1, bias=True, exact=False),
    _c("real-pre-480to80", "bwd_data", 65536 + 5, 80, 480, "affine+act", 2, exact=False),
    _c("real-row-80x480-two-dy", "bwd_weight", 65536 + 9, 80, 480, "affine+act", 2, two=True, dy_out=True, exact=False),
    _c("real-row-136x816-single", "bwd_weight", 32768, 136, 816, "act", 1, exact=False),
    _c("real-wgrad-split", "bwd_weight", 100, 116, 164, "affine", two=True, knobs=(("DL3_GEMM_MATH", "split"),), exact=False),
    _c("real-fused", "fused", 2500, 24, 144, "affine", two=True, add=1, stats=2, exact=False),
]



# ---- the case lists of the older 1x1 tests (tests/test_gpu_ops.py: PW_CASES, BD_CASES, MSK_CASES, BW_CASES, FUSED_CASES, FUSED6_CASES,
# the benchmarked routes of the row, weight-stationary and logits kernels) held to the derived bounds as well: same shapes, operand
# forms and layouts, the operands drawn here.  (Not the full-size cases of millions of rows: a float64 reference per element of those
# takes longer than a test of this suite may.)
def _old():
    from tests import test_gpu_ops as T
    out = []

    def form(act):
        return ("none", 0) if act is None else ("affine+act", act)

    fwd = list(T.PW_CASES) + [(98304 + 7, 160, 960, 0, 0, False, 2), (100000, 96, 576, 0, 0, True, 1), (131072 + 33, 64, 384, 64, 0, False, 2)]
    fwd += [c[:7] for c in T.WS_CASES] + [(32768, 256, 21, 0, 0, True, None), (32768 + 64, 256, 608, 0, 0, False, 1)]
    for i, (M, K, N, lxe, lye, bias, act) in enumerate(fwd):
        lay = ((("x", lxe, 0),) if lxe else ()) + ((("y", lye, 0),) if lye else ())
        out.append(_c("old-fwd-%d-%dx%dx%d" % (i, M, K, N), "fwd", M, K, N, *form(act), bias=bias, lay=lay, exact=False))
    bwd = list(T.BD_CASES) + [(M, K, N, act, False, add, True) for M, K, N, act, add in T.MSK_CASES]
    bwd += [(65536 + 40, 960, 160, 2, False, 0, True), (131072 + 50, 64, 384, None, True, 1, True), (32768, 256, 21, None, False, 0, False)]
    for i, (M, K, N, act, two, add, stats) in enumerate(bwd):
        out.append(_c("old-bwd-%d-%dx%dx%d" % (i, M, K, N), "bwd_data", M, K, N, *form(act), two=two, add=add, stats=stats, exact=False))
    bw = list(T.BW_CASES) + [(65536 + 8, 160, 960, 2, True, False), (65536, 960, 160, 2, True, False), (40000, 160, 960, 2, False, False),
                             (32768 + 3, 96, 576, 2, True, False), (131072, 256, 21, None, False, True)]
    for i, (M, K, N, act, two, dbias) in enumerate(bw):
        out.append(_c("old-wgrad-%d-%dx%dx%d" % (i, M, K, N), "bwd_weight", M, K, N, *form(act), two=two, dbias=dbias,
                      dy_out=two and N % 4 == 0, exact=False))
    for i, (M, K, N, act, two, has_add, stats) in enumerate(list(T.FUSED_CASES) + list(T.FUSED6_CASES)):
        out.append(_c("old-fused-%d-%dx%dx%d" % (i, M, K, N), "fused", M, K, N, *form(act), two=two, add=int(has_add), stats=stats,
                      exact=False))
    return out


OLD = _old()
GEMM_CASES = _stream() + _lds() + KSPLIT + WS + WS2 + OFF_BENCH
WGRAD_CASES = _wgrad() + ROW
FUSED_CASES = _fused()
CASES = GEMM_CASES + WGRAD_CASES + FUSED_CASES + REAL + OLD
BY_ID = {c.id: c for c in CASES}


# ---- layout ------------------------------------------------------------------------------------------------------------------------------------
def layout(case, operand):
    """(column offset, extra leading-dimension width) of an operand"""
    for item in case.lay:
        if item[0] == operand:
            return item[1], item[2]
    return 0, 0


def misaligned(case):
    return ("mis",) in case.lay


def out_width(case):
    """columns of the launch's main output: y is N wide, dx is K wide"""
    return case.N if case.entry == "fwd" else case.K


def ld(case, operand):
    width = {"x": case.K, "g": case.N, "dy": case.N, "y": case.N, "dx": case.K}[operand]
    off, extra = layout(case, operand)
    return off + width + extra


# ---- the probe's arguments (tools/pwplan_probe.cpp) ---------------------------------------------------------------------------------------
F_TWO, F_ACT, F_ADD, F_UNALIGNED, F_STATS, F_BIAS, F_XFORM, F_DUNALIGNED, F_DYOUT, F_DW = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512


def knob_env(case):
    """the DL3_* environment of the case's launch; split math is an argument of the probe, not a knob of its process"""
    return tuple((k, v) for k, v in case.knobs if k not in ("DL3_GEMM_MATH", "DL3_FUSED_V"))


def split_math(case):
    return ("DL3_GEMM_MATH", "split") in case.knobs


def runs_split_math(case):
    """the declared plan is a split-math instantiation (the knob alone does not make it one: the 32-row tiles keep the f32 MFMA)"""
    words = PLANS[case.id].split()
    return "split" in words or "split1" in words


def probe_spec(case):
    """the argument that describes the case's launch to the probe (None: dl3_pwconv_bwd_fused plans itself)"""
    M, K, N = case.M, case.K, case.N
    mis = misaligned(case)
    fl = ((F_TWO if case.two else 0) | (F_ACT if case.act else 0) | (F_ADD if case.add else 0) | (F_UNALIGNED if mis else 0) |
          (F_XFORM if case.form.startswith("affine") else 0))
    sp = 1 if split_math(case) else 0
    div = ADD_DIV if case.add == 2 else 1
    if case.entry == "fwd":
        fl |= (F_STATS if case.stats else 0) | (F_BIAS if case.bias else 0)
        return "f:%d:%d:%d:%d:%d:%d:%d:%d" % (M, K, N, fl, sp, ld(case, "x"), ld(case, "y"), div)
    if case.entry == "bwd_data":
        fl |= F_STATS if case.stats else 0
        return "b:%d:%d:%d:%d:%d:%d:%d:%d:%d" % (M, K, N, fl, sp, ld(case, "g"), ld(case, "dx"), ld(case, "x"), div)
    if case.entry == "bwd_weight":
        fl |= (F_DUNALIGNED if mis else 0) | (F_DYOUT if case.dy_out else 0) | (0 if case.slabs else F_DW)
        return "w:%d:%d:%d:%d:%d" % (M, K, N, fl, sp)
    return None


def _edge(size, tile):
    return "=" if tile and size % tile == 0 else "<"


def describe(case, plan):
    """the plan of a case in one line, from the probe's answer (a dict; fused: None — its dispatch is restated below)"""
    if case.entry == "fused":
        kb, nb = -(-case.K // 32), -(-case.N // 32)
        aux = bool(case.add) or case.stats == 2
        return "fused%d kb%d nb%d aux%d K%s N%s M%s%s" % (1 if ("DL3_FUSED_V", "1") in case.knobs else 2, kb, nb, aux, _edge(case.K, 32),
                                                          _edge(case.N, 32), _edge(case.M, 32), " M<32" if case.M < 32 else "")
    if case.entry == "bwd_weight":
        p = plan
        return "%s cfg%d vec%d split%d dys%d slabs%d K%s N%s M%s%s" % (
            p["kernel"], p["cfg"], p["vec"], p["split"], int(case.dy_out), p["slabs"], _edge(case.K, p["BKT"]),
            _edge(case.N, p["BNT"]), _edge(case.M, p["MS"]), " M<16" if case.M < p["MS"] else "")
    parts = []
    for p in plan["plans"]:
        inst = {"stream": "cfg%d %s%s%s" % (p["cfg"], "two" if p["two"] else ("fwd" if p["fwd"] else "bwd1"), " pre" if p["pre"] else "",
                                           " split" if p["split"] else ""),
                "lds": "cfg%d mode%d" % (p["cfg"], p["vmode"]),
                "ksplit": "tn%d two%d" % (p["tn"], p["two"]),
                "ws": "kq%d tn%d" % (p["kq"], p["tn"]),
                "ws2": "kq%d tn%d %s%s" % (p["kq"], p["tn"], "two" if p["two"] else ("fwd" if p["fwd"] else "bwd"), " add" if p["add"] else ""),
                "flat": "", "narrowk": ""}[p["kernel"]]
        parts.append("%s %s rows%d M%s N%s K%s" % (p["kernel"], inst, p["rows"], _edge(p["M"], p["BM"]), _edge(p["N"], p["BN"]),
                                                   _edge(p["K"], p["KT"])))
    return " + ".join(" ".join(s.split()) for s in parts)


def instantiation(case, text=None):
    """the kernel instantiation(s) a plan line names: the words in front of the sizes"""
    text = PLANS[case.id] if text is None else text
    out = []
    for part in text.split(" + "):
        words = part.split()
        keep = [w for w in words if not (w.startswith(("rows", "slabs")) or w[:2] in ("M=", "M<", "N=", "N<", "K=", "K<"))]
        out.append(" ".join(keep))
    return out


# every instantiation the launchers can name (csrc/pw*.hip: launch_stream, launch_lds, launch_ws, launch_ksplit, launch_wgrad, the
# fused launcher), in the words of describe()
def universe():
    u = set()
    for cfg in range(7):
        u |= {"stream cfg%d %s" % (cfg, f) for f in ("fwd", "bwd1", "two")}
    for cfg in range(5):
        u |= {"stream cfg%d %s split" % (cfg, f) for f in ("fwd", "bwd1", "two")}
        u |= {"lds cfg%d mode%d" % (cfg, m) for m in range(3)}
    u |= {"stream cfg4 %s pre%s" % (f, s) for f in ("bwd1", "two") for s in ("", " split")}
    u |= {"ksplit tn%d two%d" % (tn, two) for tn in (2, 3, 5) for two in (0, 1)}
    u |= {"ws kq%d tn%d" % kt for kt in ((2, 3), (3, 5), (4, 1), (4, 6), (12, 1), (18, 1), (24, 1))}
    u |= {"ws2 kq%d tn%d %s" % (kq, tn, f) for kq, tn in ((12, 3), (8, 4), (20, 5)) for f in ("fwd", "bwd")}
    u |= {"ws2 kq48 tn2 two", "ws2 kq48 tn2 two add", "flat", "narrowk"}
    for cfg in range(10):
        u |= {"wgrad cfg%d vec%d split0" % (cfg, v) for v in range(3)} | {"wgrad cfg%d vec1 split1" % cfg}
    u |= {"wgrad_row cfg%d vec1 split0 dys%d" % (cfg, d) for cfg in (2, 8) for d in (0, 1)}
    u |= {"wgrad_narrow"}
    for v in (1, 2):
        u |= {"fused%d kb%d nb%d aux%d" % (v, kb, nb, aux) for kb, nb, aux in fused_shapes(v)}
    return u


def covered():
    out = set()
    for c in CASES:
        for inst in instantiation(c):
            w = inst.split()
            if w[0] == "wgrad":
                inst = " ".join(w[:4])            # (the tiled kernel stores dY under a run-time flag)
            elif w[0] == "wgrad_narrow":
                inst = "wgrad_narrow"
            out.add(inst)
    return out


# combinations a launcher's switch could name and the planner cannot produce: name -> reason.  The host test fails when the
# probe produces one of them for a case or for a shape of tests/golden/pwconv_plan_table.json.
EXEMPT = {}


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------
def act(z, a):
    return np.maximum(z, 0) if a == 1 else (np.minimum(np.maximum(z, 0), 6) if a == 2 else z)


def mask(z, a):
    if a == 1:
        return (z > 0).astype(z.dtype)
    if a == 2:
        return ((z > 0) & (z < 6)).astype(z.dtype)
    return np.ones_like(z)


def draw(case):
    """the seeded operands of a case, float32: dict(x, s, t, w, bias, g, yraw, cA, cB, cC, add, other, mean, invstd) — None where
    the case has none"""
    M, K, N = case.M, case.K, case.N
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    f32 = np.float32
    d = dict.fromkeys("x s t w bias g yraw cA cB cC add other mean invstd".split())
    affine = case.form.startswith("affine")
    wo = out_width(case)
    rows_add = M if case.add == 1 else -(-M // ADD_DIV)
    if case.exact:
        # (relu6 on the bare input: values on either side of 6, and 6 itself)
        d["x"] = rng.integers(-3, 9 if case.act == 2 and not affine else 4, (M, K)).astype(f32)
        if affine:
            d["s"], d["t"] = rng.choice([1, 2], K).astype(f32), rng.integers(-2, 3, K).astype(f32)
        d["w"] = (rng.choice([-1, 1], (K, N)) * (rng.random((K, N)) < case.wd)).astype(f32)
        if case.bias:
            d["bias"] = rng.integers(-3, 4, N).astype(f32)
        if case.entry != "fwd":
            d["g"] = rng.integers(-2, 3, (M, N)).astype(f32)
            if case.two:
                d["yraw"] = rng.integers(-2, 3, (M, N)).astype(f32)
                d["cA"], d["cB"] = rng.choice([-2, -1, 1, 2], N).astype(f32), rng.choice([-2, -1, 1, 2], N).astype(f32)
                d["cC"] = rng.integers(-2, 3, N).astype(f32)
            d["mean"], d["invstd"] = rng.integers(-2, 3, K).astype(f32), rng.choice([0.5, 1, 2], K).astype(f32)
        if case.add:
            d["add"] = rng.integers(-3, 4, (rows_add, wo)).astype(f32)
        if case.entry == "fused" and case.stats == 2:
            d["other"] = rng.integers(-3, 4, (M, K)).astype(f32)
        return d
    a = case.act
    d["x"] = rng.normal(0, 4.0 if a == 2 else 1.0, (M, K)).astype(f32)
    if affine:
        d["s"], d["t"] = rng.uniform(0.5, 1.5, K).astype(f32), rng.normal(0, 0.5, K).astype(f32)
    if a and case.entry in ("bwd_data", "fused"):
        # (no pre-activation within 1e-4 of a kink of the mask: there fp32 and float64 may legitimately differ)
        from tests import ops_oracle as R
        s = d["s"] if affine else np.ones(K, f32)
        t = d["t"] if affine else np.zeros(K, f32)
        d["x"] = R.unambiguous_mask_input(d["x"], s, t, a)
    d["w"] = rng.normal(0, 0.2, (K, N)).astype(f32)
    if case.bias:
        d["bias"] = rng.normal(0, 1, N).astype(f32)
    if case.entry != "fwd":
        d["g"] = rng.normal(0, 1, (M, N)).astype(f32)
        if case.two:
            d["yraw"] = rng.normal(0, 1, (M, N)).astype(f32)
            d["cA"], d["cB"], d["cC"] = [rng.normal(0, 1, N).astype(f32) for _ in range(3)]
        d["mean"], d["invstd"] = rng.normal(0, 1, K).astype(f32), rng.uniform(0.5, 2, K).astype(f32)
    if case.add:
        d["add"] = rng.normal(0, 1, (rows_add, wo)).astype(f32)
    if case.entry == "fused" and case.stats == 2:
        d["other"] = rng.normal(0, 1, (M, K)).astype(f32)
    return d


ADD_SCALE = 2.0   # dl3_pwconv_bwd_data's add_scale (the forward and the fused launch add the addend itself)
CHUNK = 1 << 14


def reference(case, d, dt=None):
    """the reference of a case, evaluated in row chunks: dict of
         out [M][width] (y / dx), out_abs_max (largest sum of absolute terms of an output element), out_abs (not exact: the
         sums themselves), s1, s2 [width] and their sums of absolute terms a1, a2 (float64), dw [K][N], dw_abs, dbias, dbias_abs,
         dy [M][N].
    dt: the arithmetic of the products — float32 for exact cases (exact under conditions()), float64 otherwise"""
    dt = dt or (np.float32 if case.exact else np.float64)
    M, K, N = case.M, case.K, case.N
    a = case.act
    wo = out_width(case)
    gemm_out = case.entry in ("fwd", "bwd_data", "fused")
    r = {}
    if gemm_out:
        r["out"] = np.empty((M, wo), dt)
        r["out_abs_max"] = 0.0
        if not case.exact:
            r["out_abs"] = np.empty((M, wo), np.float64)
        r["s1"], r["s2"], r["a1"], r["a2"] = (np.zeros(wo) for _ in range(4))
    if case.entry in ("bwd_weight", "fused"):
        r["dw"], r["dw_abs"] = np.zeros((K, N), dt), np.zeros((K, N), dt)
        r["dbias"], r["dbias_abs"] = np.zeros(N), np.zeros(N)
        if case.dy_out:
            r["dy"] = np.empty((M, N), dt)
    w = d["w"].astype(dt)
    s = d["s"].astype(dt) if d["s"] is not None else None
    t = d["t"].astype(dt) if d["t"] is not None else None
    for m0 in range(0, M, CHUNK):
        sl = slice(m0, min(M, m0 + CHUNK))
        x = d["x"][sl].astype(dt)
        z = x if s is None else s * x + t
        xin = act(z, a)
        # magnitudes of the operand elements: exact cases need the products' own sizes; real-valued ones the sum of the absolute
        # terms an element is made of (a transform or a two-tensor dY whose terms cancel still carries their rounding)
        xmag = np.abs(xin) if (case.exact or s is None) else np.abs(s * x) + np.abs(t)
        if case.entry == "fwd":
            o, oa = xin @ w, xmag @ np.abs(w)
            if case.bias:
                o, oa = o + d["bias"].astype(dt), oa + np.abs(d["bias"]).astype(dt)
        else:
            g = d["g"][sl].astype(dt)
            dY = (d["cA"].astype(dt) * g + d["cB"].astype(dt) * d["yraw"][sl].astype(dt) + d["cC"].astype(dt)) if case.two else g
            r["dy_abs_max"] = max(r.get("dy_abs_max", 0.0), float(np.abs(dY).max()))
            dmag = np.abs(dY) if (case.exact or not case.two) else (
                np.abs(d["cA"].astype(dt) * g) + np.abs(d["cB"].astype(dt) * d["yraw"][sl].astype(dt)) + np.abs(d["cC"].astype(dt)))
            if "dw" in r:
                r["dw"] += xin.T @ dY
                r["dw_abs"] += xmag.T @ dmag
                r["dbias"] += dY.sum(0, dtype=np.float64)
                r["dbias_abs"] += dmag.sum(0, dtype=np.float64)
                if case.dy_out:
                    r["dy"][sl] = dY
            if gemm_out:
                mk = mask(z, a)
                o, oa = (dY @ w.T) * mk, (dmag @ np.abs(w).T) * mk
        if gemm_out:
            if case.add:
                sc = dt(ADD_SCALE if case.entry == "bwd_data" else 1.0)
                rows = np.arange(sl.start, sl.stop) // (ADD_DIV if case.add == 2 else 1)
                ad = sc * d["add"][rows].astype(dt)
                o, oa = o + ad, oa + np.abs(ad)
            r["out"][sl] = o
            r["out_abs_max"] = max(r["out_abs_max"], float(oa.max()))
            if not case.exact:
                r["out_abs"][sl] = oa
            o64, oa64 = o.astype(np.float64), oa.astype(np.float64)
            r["s1"] += o64.sum(0)
            r["a1"] += np.abs(o64).sum(0)
            if case.entry == "fwd":
                r["s2"] += (o64 * o64).sum(0)
                r["a2"] += (o64 * o64).sum(0)
            else:
                sx = (d["other"] if d["other"] is not None else d["x"])[sl].astype(np.float64)
                xh = (sx - d["mean"].astype(np.float64)) * d["invstd"].astype(np.float64)
                r["s2"] += (o64 * xh).sum(0)
                r["a2"] += np.abs(o64 * xh).sum(0)
    return r


def conditions(case, d, r):
    """the exactness conditions of an exact case, each as (name, value, limit): value < limit must hold"""
    out = [("|x~|", float(np.abs(act(d["x"] if d["s"] is None else d["s"] * d["x"] + d["t"], case.act)).max()), 257.0),
           ("|w|", float(np.abs(d["w"]).max()), 257.0)]
    if "out" in r:
        out.append(("max sum_k |a||b| of an output", r["out_abs_max"], LIM))
        if case.stats:
            out += [("sum_m |out| per channel", float(r["a1"].max()), LIM),
                    ("sum_m |out^2| or |out * xhat| per channel", float(r["a2"].max()), LIM if case.entry == "fwd" else LIM / 2)]
    if case.entry != "fwd":
        out.append(("|dY|", r["dy_abs_max"], 257.0))
    if "dw" in r:
        out += [("sum_m |x~||dY| per dW element", float(r["dw_abs"].max()), LIM),
                ("sum_m |dY| per channel", float(r["dbias_abs"].max()), LIM)]
    return out


PLANS = {
    'stream-cfg0-fwd': 'stream cfg0 fwd rows2 M< N< K<',
    'stream-cfg0-bwd1': 'stream cfg0 bwd1 rows2 M< N< K<',
    'stream-cfg0-two': 'stream cfg0 two rows2 M< N< K<',
    'stream-split-cfg0-fwd': 'stream cfg0 fwd split rows2 M< N< K<',
    'stream-split-cfg0-bwd1': 'stream cfg0 bwd1 split rows2 M< N< K<',
    'stream-split-cfg0-two': 'stream cfg0 two split rows2 M< N< K<',
    'stream-cfg1-fwd': 'stream cfg1 fwd rows2 M< N< K<',
    'stream-cfg1-bwd1': 'stream cfg1 bwd1 rows2 M< N< K<',
    'stream-cfg1-two': 'stream cfg1 two rows2 M< N< K<',
    'stream-split-cfg1-fwd': 'stream cfg1 fwd split rows2 M< N< K<',
    'stream-split-cfg1-bwd1': 'stream cfg1 bwd1 split rows2 M< N< K<',
    'stream-split-cfg1-two': 'stream cfg1 two split rows2 M< N< K<',
    'stream-cfg2-fwd': 'stream cfg2 fwd rows2 M< N< K<',
    'stream-cfg2-bwd1': 'stream cfg2 bwd1 rows2 M< N< K<',
    'stream-cfg2-two': 'stream cfg2 two rows2 M< N< K<',
    'stream-split-cfg2-fwd': 'stream cfg2 fwd split rows2 M< N< K<',
    'stream-split-cfg2-bwd1': 'stream cfg2 bwd1 split rows2 M< N< K<',
    'stream-split-cfg2-two': 'stream cfg2 two split rows2 M< N< K<',
    'stream-cfg3-fwd': 'stream cfg3 fwd rows2 M< N< K<',
    'stream-cfg3-bwd1': 'stream cfg3 bwd1 rows2 M< N< K<',
    'stream-cfg3-two': 'stream cfg3 two rows2 M< N< K<',
    'stream-split-cfg3-fwd': 'stream cfg3 fwd split rows2 M< N< K<',
    'stream-split-cfg3-bwd1': 'stream cfg3 bwd1 split rows2 M< N< K<',
    'stream-split-cfg3-two': 'stream cfg3 two split rows2 M< N< K<',
    'stream-cfg4-fwd': 'stream cfg4 fwd rows2 M< N< K<',
    'stream-cfg4-bwd1': 'stream cfg4 bwd1 rows2 M< N< K<',
    'stream-cfg4-two': 'stream cfg4 two rows2 M< N< K<',
    'stream-split-cfg4-fwd': 'stream cfg4 fwd split rows2 M< N< K<',
    'stream-split-cfg4-bwd1': 'stream cfg4 bwd1 split rows2 M< N< K<',
    'stream-split-cfg4-two': 'stream cfg4 two split rows2 M< N< K<',
    'stream-cfg5-fwd': 'stream cfg5 fwd rows3 M< N< K<',
    'stream-cfg5-bwd1': 'stream cfg5 bwd1 rows3 M< N< K<',
    'stream-cfg5-two': 'stream cfg5 two rows3 M< N< K<',
    'stream-cfg6-fwd': 'stream cfg6 fwd rows3 M< N< K<',
    'stream-cfg6-bwd1': 'stream cfg6 bwd1 rows3 M< N< K<',
    'stream-cfg6-two': 'stream cfg6 two rows3 M< N< K<',
    'stream-pre-bwd1': 'stream cfg4 bwd1 pre rows3 M< N< K<',
    'stream-pre-two': 'stream cfg4 two pre rows2 M< N= K<',
    'stream-split-pre-bwd1': 'stream cfg4 bwd1 pre split rows3 M< N< K<',
    'stream-split-pre-two': 'stream cfg4 two pre split rows2 M< N= K<',
    'stream-pre-whole': 'stream cfg4 bwd1 pre rows2 M= N= K=',
    'stream-pre-off': 'stream cfg4 bwd1 rows3 M< N< K<',
    'stream-fwd-add-image64': 'stream cfg0 fwd rows2 M< N< K<',
    'stream-fwd-add-tensor': 'stream cfg0 fwd rows2 M< N< K<',
    'stream-fwd-slices-no-stats': 'stream cfg6 fwd rows10 M< N< K=',
    'stream-bwd-slices': 'stream cfg6 two rows10 M< N< K=',
    'lds-cfg0-mode0-fwd': 'lds cfg0 mode0 rows2 M< N< K<',
    'lds-cfg0-mode0-bwd': 'lds cfg0 mode0 rows2 M< N< K<',
    'lds-cfg0-mode2-fwd': 'lds cfg0 mode2 rows2 M< N< K<',
    'lds-cfg0-mode2-bwd': 'lds cfg0 mode2 rows2 M< N< K<',
    'lds-cfg0-mode1-fwd': 'lds cfg0 mode1 rows2 M< N< K<',
    'lds-cfg0-mode1-bwd': 'lds cfg0 mode1 rows2 M< N< K<',
    'lds-cfg1-mode0-fwd': 'lds cfg1 mode0 rows2 M< N< K<',
    'lds-cfg1-mode0-bwd': 'lds cfg1 mode0 rows2 M< N< K<',
    'lds-cfg1-mode2-fwd': 'lds cfg1 mode2 rows2 M< N< K<',
    'lds-cfg1-mode2-bwd': 'lds cfg1 mode2 rows2 M< N< K<',
    'lds-cfg1-mode1-fwd': 'lds cfg1 mode1 rows2 M< N< K=',
    'lds-cfg1-mode1-bwd': 'lds cfg1 mode1 rows2 M< N< K=',
    'lds-cfg2-mode0-fwd': 'lds cfg2 mode0 rows2 M< N< K<',
    'lds-cfg2-mode0-bwd': 'lds cfg2 mode0 rows2 M< N< K<',
    'lds-cfg2-mode2-fwd': 'lds cfg2 mode2 rows2 M< N< K<',
    'lds-cfg2-mode2-bwd': 'lds cfg2 mode2 rows2 M< N< K<',
    'lds-cfg2-mode1-fwd': 'lds cfg2 mode1 rows2 M< N< K<',
    'lds-cfg2-mode1-bwd': 'lds cfg2 mode1 rows2 M< N< K<',
    'lds-cfg3-mode0-fwd': 'lds cfg3 mode0 rows2 M< N< K<',
    'lds-cfg3-mode0-bwd': 'lds cfg3 mode0 rows2 M< N< K<',
    'lds-cfg3-mode2-fwd': 'lds cfg3 mode2 rows2 M< N< K<',
    'lds-cfg3-mode2-bwd': 'lds cfg3 mode2 rows2 M< N< K<',
    'lds-cfg3-mode1-fwd': 'lds cfg3 mode1 rows2 M< N< K=',
    'lds-cfg3-mode1-bwd': 'lds cfg3 mode1 rows2 M< N< K=',
    'lds-cfg4-mode0-fwd': 'lds cfg4 mode0 rows2 M< N< K<',
    'lds-cfg4-mode0-bwd': 'lds cfg4 mode0 rows2 M< N< K<',
    'lds-cfg4-mode2-fwd': 'lds cfg4 mode2 rows2 M< N< K<',
    'lds-cfg4-mode2-bwd': 'lds cfg4 mode2 rows2 M< N< K<',
    'lds-cfg4-mode1-fwd': 'lds cfg4 mode1 rows2 M< N< K<',
    'lds-cfg4-mode1-bwd': 'lds cfg4 mode1 rows2 M< N< K<',
    'lds-mode1-auto-whole': 'lds cfg2 mode1 rows1 M= N= K=',
    'ksplit-tn2-fwd': 'ksplit tn2 two0 rows32 M= N= K=',
    'ksplit-tn3-fwd-ragged': 'ksplit tn3 two0 rows33 M< N= K<',
    'ksplit-tn5-fwd-ragged-columns': 'ksplit tn5 two0 rows34 M< N< K=',
    'ksplit-tn5-bwd1': 'ksplit tn5 two0 rows34 M< N= K=',
    'ksplit-tn3-bwd1-add': 'ksplit tn3 two0 rows32 M= N= K=',
    'ksplit-tn2-two': 'ksplit tn2 two1 rows33 M< N= K=',
    'ksplit-tn3-two': 'ksplit tn3 two1 rows33 M< N< K<',
    'ksplit-tn5-two': 'ksplit tn5 two1 rows32 M= N= K=',
    'ws-16x96-whole': 'ws kq2 tn3 rows256 M= N= K=',
    'ws-16x80-ragged': 'ws kq2 tn3 rows257 M< N< K=',
    'ws-24x160-whole': 'ws kq3 tn5 rows256 M= N= K=',
    'ws-24x136-ragged': 'ws kq3 tn5 rows257 M< N< K=',
    'ws-32x32-whole': 'ws kq4 tn1 rows256 M= N= K=',
    'ws-32x24-ragged': 'ws kq4 tn1 rows257 M< N< K=',
    'ws-32x192-whole': 'ws kq4 tn6 rows256 M= N= K=',
    'ws-32x172-ragged': 'ws kq4 tn6 rows257 M< N< K=',
    'ws-96x32-whole': 'ws kq12 tn1 rows256 M= N= K=',
    'ws-96x16-ragged': 'ws kq12 tn1 rows257 M< N< K=',
    'ws-144x32-whole': 'ws kq18 tn1 rows256 M= N= K=',
    'ws-144x20-ragged': 'ws kq18 tn1 rows257 M< N< K=',
    'ws-192x32-whole': 'ws kq24 tn1 rows256 M= N= K=',
    'ws-192x28-ragged': 'ws kq24 tn1 rows257 M< N< K=',
    'ws-32x172-1250-partial-rows': 'ws kq4 tn6 rows313 M= N< K=',
    'ws2-fwd-tn3': 'ws2 kq12 tn3 fwd rows128 M= N= K=',
    'ws2-fwd-tn3-ragged': 'ws2 kq12 tn3 fwd rows85 M< N< K=',
    'ws2-fwd-tn4': 'ws2 kq8 tn4 fwd rows256 M< N= K=',
    'ws2-fwd-tn5': 'ws2 kq20 tn5 fwd rows128 M< N= K=',
    'ws2-bwd-tn3': 'ws2 kq12 tn3 bwd rows128 M< N= K=',
    'ws2-bwd-tn4': 'ws2 kq8 tn4 bwd rows256 M= N= K=',
    'ws2-bwd-tn4-ragged-columns': 'ws2 kq8 tn4 bwd rows128 M< N< K=',
    'ws2-bwd-tn5': 'ws2 kq20 tn5 bwd rows128 M< N= K=',
    'ws2-bwd-tn5-no-stats': 'ws2 kq20 tn5 bwd rows128 M= N= K=',
    'ws2-bwd-384to64': 'ws2 kq48 tn2 two rows256 M< N= K=',
    'ws2-bwd-384to64-add': 'ws2 kq48 tn2 two add rows256 M= N= K=',
    'flat-logits-21': 'flat rows33 M< N< K<',
    'flat-logits-32-no-stats': 'flat rows32 M= N= K<',
    'narrowk-21': 'narrowk rows0 M< N= K<',
    'narrowk-32': 'narrowk rows0 M= N= K=',
    'pre-480to80-partial-column-tile': 'stream cfg4 bwd1 pre rows513 M< N< K=',
    'pre-480to80-two': 'stream cfg4 two pre rows512 M= N< K=',
    'pre-96to48-whole': 'stream cfg4 bwd1 pre rows512 M= N= K=',
    'colsplit-fwd': 'stream cfg2 fwd rows129 M< N= K= + stream cfg3 fwd rows257 M< N= K=',
    'colsplit-bwd1': 'stream cfg2 bwd1 rows128 M= N= K= + stream cfg3 bwd1 rows256 M= N= K=',
    'wgrad-cfg0-mode1': 'wgrad cfg0 vec1 split0 dys1 slabs1 K< N< M<',
    'wgrad-cfg0-mode0': 'wgrad cfg0 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg0-mode2': 'wgrad cfg0 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg0-split': 'wgrad cfg0 vec1 split1 dys0 slabs1 K< N< M<',
    'wgrad-cfg1-mode1': 'wgrad cfg1 vec1 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg1-mode0': 'wgrad cfg1 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg1-mode2': 'wgrad cfg1 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg1-split': 'wgrad cfg1 vec1 split1 dys1 slabs1 K< N< M<',
    'wgrad-cfg2-mode1': 'wgrad cfg2 vec1 split0 dys1 slabs1 K< N< M<',
    'wgrad-cfg2-mode0': 'wgrad cfg2 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg2-mode2': 'wgrad cfg2 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg2-split': 'wgrad cfg2 vec1 split1 dys0 slabs1 K< N< M<',
    'wgrad-cfg3-mode1': 'wgrad cfg3 vec1 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg3-mode0': 'wgrad cfg3 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg3-mode2': 'wgrad cfg3 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg3-split': 'wgrad cfg3 vec1 split1 dys1 slabs1 K< N< M<',
    'wgrad-cfg4-mode1': 'wgrad cfg4 vec1 split0 dys1 slabs1 K< N< M<',
    'wgrad-cfg4-mode0': 'wgrad cfg4 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg4-mode2': 'wgrad cfg4 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg4-split': 'wgrad cfg4 vec1 split1 dys0 slabs1 K< N< M<',
    'wgrad-cfg5-mode1': 'wgrad cfg5 vec1 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg5-mode0': 'wgrad cfg5 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg5-mode2': 'wgrad cfg5 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg5-split': 'wgrad cfg5 vec1 split1 dys1 slabs1 K< N< M<',
    'wgrad-cfg6-mode1': 'wgrad cfg6 vec1 split0 dys1 slabs1 K< N< M<',
    'wgrad-cfg6-mode0': 'wgrad cfg6 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg6-mode2': 'wgrad cfg6 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg6-split': 'wgrad cfg6 vec1 split1 dys0 slabs1 K< N< M<',
    'wgrad-cfg7-mode1': 'wgrad cfg7 vec1 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg7-mode0': 'wgrad cfg7 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg7-mode2': 'wgrad cfg7 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg7-split': 'wgrad cfg7 vec1 split1 dys1 slabs1 K< N< M<',
    'wgrad-cfg8-mode1': 'wgrad cfg8 vec1 split0 dys1 slabs1 K< N< M<',
    'wgrad-cfg8-mode0': 'wgrad cfg8 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg8-mode2': 'wgrad cfg8 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg8-split': 'wgrad cfg8 vec1 split1 dys0 slabs1 K< N< M<',
    'wgrad-cfg9-mode1': 'wgrad cfg9 vec1 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg9-mode0': 'wgrad cfg9 vec0 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg9-mode2': 'wgrad cfg9 vec2 split0 dys0 slabs1 K< N< M<',
    'wgrad-cfg9-split': 'wgrad cfg9 vec1 split1 dys1 slabs1 K< N< M<',
    'wgrad-whole-tiles': 'wgrad cfg1 vec1 split0 dys1 slabs1 K= N= M=',
    'wgrad-less-than-a-stage': 'wgrad cfg2 vec1 split0 dys1 slabs1 K= N= M< M<16',
    'wgrad-slabs-left': 'wgrad cfg7 vec1 split0 dys0 slabs13 K< N< M=',
    'wgrad-mode0-misaligned': 'wgrad cfg0 vec0 split0 dys0 slabs1 K= N= M<',
    'wgrad-slices-dy': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N< M<',
    'row-80x480-two-dy': 'wgrad_row cfg8 vec1 split0 dys1 slabs238 K< N< M<',
    'row-80x480-single': 'wgrad_row cfg8 vec1 split0 dys0 slabs238 K< N< M=',
    'row-88x528-two': 'wgrad_row cfg8 vec1 split0 dys0 slabs108 K< N< M<',
    'row-88x528-single-dy': 'wgrad_row cfg8 vec1 split0 dys1 slabs108 K< N< M=',
    'row-136x816-two-dy': 'wgrad_row cfg2 vec1 split0 dys1 slabs70 K< N< M<',
    'row-136x816-single': 'wgrad_row cfg2 vec1 split0 dys0 slabs70 K< N< M=',
    'row-152x912-two': 'wgrad_row cfg2 vec1 split0 dys0 slabs62 K< N< M<',
    'row-152x912-single-dy': 'wgrad_row cfg2 vec1 split0 dys1 slabs62 K< N< M=',
    'row-160x328-whole-row-two-dy': 'wgrad_row cfg2 vec1 split0 dys1 slabs76 K= N< M=',
    'row-96x576-whole-row-single': 'wgrad_row cfg8 vec1 split0 dys0 slabs99 K= N< M<',
    'row-160x384-whole-tiles-two-dy': 'wgrad_row cfg2 vec1 split0 dys1 slabs72 K= N= M=',
    'wgrad-narrow-21': 'wgrad_narrow cfg7 vec2 split0 dys0 slabs256 K= N< M<',
    'wgrad-narrow-32': 'wgrad_narrow cfg0 vec1 split0 dys0 slabs256 K= N< M=',
    'fused-1x1': 'fused2 kb1 nb1 aux0 K< N< M=',
    'fused-1x1-aux': 'fused2 kb1 nb1 aux1 K= N= M<',
    'fused-1x2': 'fused2 kb1 nb2 aux0 K< N= M< M<32',
    'fused-1x2-aux': 'fused2 kb1 nb2 aux1 K= N< M<',
    'fused-1x3': 'fused2 kb1 nb3 aux0 K< N= M=',
    'fused-1x3-aux': 'fused2 kb1 nb3 aux1 K= N= M<',
    'fused-1x4': 'fused2 kb1 nb4 aux0 K< N< M< M<32',
    'fused-1x4-aux': 'fused2 kb1 nb4 aux1 K= N= M<',
    'fused-1x5': 'fused2 kb1 nb5 aux0 K< N= M=',
    'fused-1x5-aux': 'fused2 kb1 nb5 aux1 K= N< M<',
    'fused-1x6': 'fused2 kb1 nb6 aux0 K< N= M< M<32',
    'fused-1x6-aux': 'fused2 kb1 nb6 aux1 K= N= M<',
    'fused-2x1': 'fused2 kb2 nb1 aux0 K< N< M=',
    'fused-2x1-aux': 'fused2 kb2 nb1 aux1 K= N= M<',
    'fused-2x2': 'fused2 kb2 nb2 aux0 K< N= M< M<32',
    'fused-2x2-aux': 'fused2 kb2 nb2 aux1 K= N< M<',
    'fused-2x3': 'fused2 kb2 nb3 aux0 K< N= M=',
    'fused-2x3-aux': 'fused2 kb2 nb3 aux1 K= N= M<',
    'fused-3x1': 'fused2 kb3 nb1 aux0 K< N< M< M<32',
    'fused-3x2': 'fused2 kb3 nb2 aux0 K= N= M<',
    'fused-4x1': 'fused2 kb4 nb1 aux0 K< N= M=',
    'fused-5x1': 'fused2 kb5 nb1 aux0 K= N< M<',
    'fused-6x1': 'fused2 kb6 nb1 aux0 K< N= M< M<32',
    'fused-v1-1x1': 'fused1 kb1 nb1 aux0 K< N< M=',
    'fused-v1-1x1-aux': 'fused1 kb1 nb1 aux1 K= N= M<',
    'fused-v1-1x2': 'fused1 kb1 nb2 aux0 K< N= M< M<32',
    'fused-v1-1x2-aux': 'fused1 kb1 nb2 aux1 K= N< M<',
    'fused-v1-1x3': 'fused1 kb1 nb3 aux0 K< N= M=',
    'fused-v1-1x3-aux': 'fused1 kb1 nb3 aux1 K= N= M<',
    'fused-v1-1x4': 'fused1 kb1 nb4 aux0 K< N< M< M<32',
    'fused-v1-1x4-aux': 'fused1 kb1 nb4 aux1 K= N= M<',
    'fused-v1-1x5': 'fused1 kb1 nb5 aux0 K< N= M=',
    'fused-v1-1x5-aux': 'fused1 kb1 nb5 aux1 K= N< M<',
    'fused-v1-2x1': 'fused1 kb2 nb1 aux0 K< N= M< M<32',
    'fused-v1-2x1-aux': 'fused1 kb2 nb1 aux1 K= N= M<',
    'fused-v1-2x2': 'fused1 kb2 nb2 aux0 K< N< M=',
    'fused-v1-2x2-aux': 'fused1 kb2 nb2 aux1 K= N= M<',
    'fused-v1-3x1': 'fused1 kb3 nb1 aux0 K< N= M< M<32',
    'fused-v1-4x1': 'fused1 kb4 nb1 aux0 K= N< M<',
    'fused-v1-5x1': 'fused1 kb5 nb1 aux0 K< N= M=',
    'fused-more-stages-than-workgroups': 'fused2 kb1 nb5 aux1 K< N< M<',
    'real-stream-fwd': 'stream cfg6 fwd rows10 M< N< K=',
    'real-stream-split-fwd': 'stream cfg0 fwd split rows3 M< N< K=',
    'real-stream-split-two': 'stream cfg3 two split rows3 M< N< K=',
    'real-stream-split-bwd1-pre': 'stream cfg4 bwd1 pre split rows3 M< N< K=',
    'real-stream-split-auto': 'stream cfg3 two split rows513 M< N= K=',
    'real-stream-two': 'stream cfg6 two rows10 M< N< K=',
    'real-lds-mode1-fwd': 'lds cfg2 mode1 rows1 M< N< K<',
    'real-lds-mode1-bwd': 'lds cfg2 mode1 rows1 M< N< K=',
    'real-ksplit-fwd': 'ksplit tn3 two0 rows33 M< N= K<',
    'real-ws-32x172': 'ws kq4 tn6 rows257 M< N< K=',
    'real-ws2-fwd': 'ws2 kq12 tn3 fwd rows85 M< N< K=',
    'real-pre-480to80': 'stream cfg4 bwd1 pre rows513 M< N< K=',
    'real-row-80x480-two-dy': 'wgrad_row cfg8 vec1 split0 dys1 slabs238 K< N< M<',
    'real-row-136x816-single': 'wgrad_row cfg2 vec1 split0 dys0 slabs70 K< N< M=',
    'real-wgrad-split': 'wgrad cfg0 vec1 split1 dys0 slabs1 K< N< M<',
    'real-fused': 'fused2 kb1 nb5 aux1 K< N< M<',
    'old-fwd-0-256x16x96': 'stream cfg6 fwd rows8 M= N< K=',
    'old-fwd-1-512x96x24': 'stream cfg6 fwd rows16 M= N< K=',
    'old-fwd-2-300x32x21': 'lds cfg2 mode2 rows2 M< N< K=',
    'old-fwd-3-4100x256x21': 'lds cfg2 mode2 rows17 M< N< K=',
    'old-fwd-4-300x30x21': 'lds cfg2 mode0 rows2 M< N< K<',
    'old-fwd-5-1024x160x960': 'stream cfg6 fwd rows32 M= N< K=',
    'old-fwd-6-384x960x160': 'stream cfg6 fwd rows12 M= N< K=',
    'old-fwd-7-130x24x144': 'stream cfg6 fwd rows5 M< N< K<',
    'old-fwd-8-64x320x256': 'stream cfg6 fwd rows2 M= N= K=',
    'old-fwd-9-200x512x256': 'stream cfg6 fwd rows7 M< N= K=',
    'old-fwd-10-4x320x256': 'stream cfg6 fwd rows1 M< N= K=',
    'old-fwd-11-256x256x1344': 'stream cfg6 fwd rows8 M= N< K=',
    'old-fwd-12-256x64x384': 'stream cfg6 fwd rows8 M= N= K=',
    'old-fwd-13-520x728x728': 'stream cfg6 fwd rows17 M< N< K<',
    'old-fwd-14-300x1024x1536': 'stream cfg6 fwd rows10 M< N= K=',
    'old-fwd-15-260x1536x2048': 'stream cfg6 fwd rows9 M< N= K=',
    'old-fwd-16-200x2048x256': 'stream cfg6 fwd rows7 M< N= K=',
    'old-fwd-17-384x304x256': 'stream cfg6 fwd rows12 M= N= K=',
    'old-fwd-18-384x256x48': 'stream cfg6 fwd rows12 M= N< K=',
    'old-fwd-19-128x256x728': 'stream cfg6 fwd rows4 M= N< K=',
    'old-fwd-20-2048x960x160': 'ksplit tn5 two0 rows64 M= N= K=',
    'old-fwd-21-1100x576x96': 'ksplit tn3 two0 rows35 M< N= K=',
    'old-fwd-22-8192x384x96': 'ksplit tn3 two0 rows256 M= N= K=',
    'old-fwd-23-4096x256x144': 'ksplit tn5 two0 rows128 M= N< K=',
    'old-fwd-24-1056x196x132': 'ksplit tn5 two0 rows33 M= N< K<',
    'old-fwd-25-2048x384x64': 'ksplit tn2 two0 rows64 M= N= K=',
    'old-fwd-26-98311x160x960': 'ws2 kq20 tn5 fwd rows42 M< N= K=',
    'old-fwd-27-100000x96x576': 'ws2 kq12 tn3 fwd rows42 M= N= K=',
    'old-fwd-28-131105x64x384': 'ws2 kq8 tn4 fwd rows85 M< N= K=',
    'old-fwd-29-32845x16x96': 'ws kq2 tn3 rows257 M< N= K=',
    'old-fwd-30-40000x32x16': 'ws kq4 tn1 rows313 M= N< K=',
    'old-fwd-31-32773x96x24': 'ws kq12 tn1 rows257 M< N< K=',
    'old-fwd-32-33000x24x144': 'ws kq3 tn5 rows258 M< N< K=',
    'old-fwd-33-32800x144x24': 'ws kq18 tn1 rows257 M= N< K=',
    'old-fwd-34-36000x144x32': 'ws kq18 tn1 rows282 M= N= K=',
    'old-fwd-35-32799x32x192': 'ws kq4 tn6 rows257 M< N= K=',
    'old-fwd-36-50000x192x32': 'ws kq24 tn1 rows391 M< N= K=',
    'old-fwd-37-32768x24x144': 'ws kq3 tn5 rows256 M= N< K=',
    'old-fwd-38-32768x256x21': 'flat rows128 M= N< K<',
    'old-fwd-39-32832x256x608': 'stream cfg2 fwd rows129 M< N= K= + stream cfg3 fwd rows257 M< N= K=',
    'old-bwd-0-256x16x96': 'stream cfg6 two rows8 M= N< K=',
    'old-bwd-1-300x256x21': 'lds cfg2 mode0 rows2 M< N= K<',
    'old-bwd-2-384x160x960': 'stream cfg6 two rows12 M= N< K=',
    'old-bwd-3-512x960x160': 'stream cfg6 two rows16 M= N< K=',
    'old-bwd-4-256x320x256': 'stream cfg6 two rows8 M= N< K=',
    'old-bwd-5-130x144x24': 'stream cfg6 two rows5 M< N< K<',
    'old-bwd-6-256x512x256': 'stream cfg6 two rows8 M= N= K=',
    'old-bwd-7-520x728x728': 'stream cfg6 two rows17 M< N< K<',
    'old-bwd-8-260x1536x2048': 'stream cfg6 two rows9 M< N= K=',
    'old-bwd-9-300x1024x1536': 'stream cfg6 two rows10 M< N= K=',
    'old-bwd-10-200x2048x256': 'stream cfg6 two rows7 M< N= K=',
    'old-bwd-11-384x304x256': 'stream cfg6 two rows12 M= N< K=',
    'old-bwd-12-384x256x48': 'stream cfg6 two rows12 M= N= K=',
    'old-bwd-13-2048x160x960': 'ksplit tn5 two1 rows64 M= N= K=',
    'old-bwd-14-1100x96x576': 'ksplit tn3 two1 rows35 M< N= K=',
    'old-bwd-15-4096x160x320': 'ksplit tn5 two1 rows128 M= N= K=',
    'old-bwd-16-2048x64x384': 'ksplit tn2 two1 rows64 M= N= K=',
    'old-bwd-17-65736x960x160': 'stream cfg4 two pre rows47 M< N= K=',
    'old-bwd-18-65536x576x96': 'ws2 kq12 tn3 bwd rows42 M= N= K=',
    'old-bwd-19-66000x192x32': 'stream cfg4 two pre rows516 M< N= K=',
    'old-bwd-20-65536x384x64': 'stream cfg4 two pre rows128 M= N= K=',
    'old-bwd-21-65536x960x160': 'ws2 kq20 tn5 bwd rows42 M= N= K=',
    'old-bwd-22-65736x160x960': 'stream cfg3 bwd1 rows514 M< N= K=',
    'old-bwd-23-65536x576x96': 'ws2 kq12 tn3 bwd rows42 M= N= K=',
    'old-bwd-24-8192x384x64': 'stream cfg6 bwd1 rows256 M= N= K=',
    'old-bwd-25-4096x320x256': 'stream cfg6 bwd1 rows128 M= N< K=',
    'old-bwd-26-1000x144x24': 'stream cfg6 bwd1 rows32 M< N< K<',
    'old-bwd-27-32768x728x728': 'stream cfg0 bwd1 rows256 M= N< K<',
    'old-bwd-28-8192x160x960': 'ksplit tn5 two0 rows256 M= N= K=',
    'old-bwd-29-4128x96x576': 'ksplit tn3 two0 rows129 M= N= K=',
    'old-bwd-30-65576x960x160': 'ws2 kq20 tn5 bwd rows42 M< N= K=',
    'old-bwd-31-131122x64x384': 'ws2 kq48 tn2 two add rows256 M< N= K=',
    'old-bwd-32-32768x256x21': 'narrowk rows0 M= N= K<',
    'old-wgrad-0-1024x16x96': 'wgrad cfg6 vec1 split0 dys1 slabs16 K< N< M=',
    'old-wgrad-1-2048x160x960': 'wgrad cfg0 vec1 split0 dys1 slabs3 K< N= M=',
    'old-wgrad-2-2048x960x160': 'wgrad cfg7 vec1 split0 dys1 slabs3 K< N= M=',
    'old-wgrad-3-1000x256x21': 'wgrad cfg7 vec2 split0 dys0 slabs12 K= N< M<',
    'old-wgrad-4-4x320x256': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N= M< M<16',
    'old-wgrad-5-4096x96x576': 'wgrad cfg7 vec1 split0 dys1 slabs12 K< N= M=',
    'old-wgrad-6-512x512x256': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N= M=',
    'old-wgrad-7-700x24x144': 'wgrad cfg6 vec1 split0 dys1 slabs8 K< N< M<',
    'old-wgrad-8-1040x728x728': 'wgrad cfg7 vec1 split0 dys1 slabs1 K< N< M=',
    'old-wgrad-9-600x1536x2048': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N= M<',
    'old-wgrad-10-600x2048x256': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N= M<',
    'old-wgrad-11-768x304x256': 'wgrad cfg0 vec1 split0 dys1 slabs1 K< N= M=',
    'old-wgrad-12-768x256x48': 'wgrad cfg0 vec1 split0 dys1 slabs4 K= N< M=',
    'old-wgrad-13-520x1024x1536': 'wgrad cfg0 vec1 split0 dys1 slabs1 K= N= M<',
    'old-wgrad-14-65544x160x960': 'wgrad_row cfg2 vec1 split0 dys1 slabs64 K= N< M<',
    'old-wgrad-15-65536x960x160': 'wgrad cfg3 vec1 split0 dys1 slabs64 K< N= M=',
    'old-wgrad-16-40000x160x960': 'wgrad_row cfg2 vec1 split0 dys0 slabs64 K= N< M=',
    'old-wgrad-17-32771x96x576': 'wgrad_row cfg8 vec1 split0 dys1 slabs99 K= N< M<',
    'old-wgrad-18-131072x256x21': 'wgrad_narrow cfg7 vec2 split0 dys0 slabs256 K= N< M=',
    'old-fused-0-4113x16x96': 'fused2 kb1 nb3 aux1 K< N= M<',
    'old-fused-1-3000x32x16': 'fused2 kb1 nb1 aux0 K= N< M<',
    'old-fused-2-2500x24x144': 'fused2 kb1 nb5 aux1 K< N< M<',
    'old-fused-3-2048x144x24': 'fused2 kb5 nb1 aux0 K< N< M=',
    'old-fused-4-1000x96x24': 'fused2 kb3 nb1 aux0 K= N< M<',
    'old-fused-5-777x144x32': 'fused2 kb5 nb1 aux0 K< N= M<',
    'old-fused-6-1500x64x64': 'fused2 kb2 nb2 aux1 K= N= M<',
    'old-fused-7-640x64x64': 'fused2 kb2 nb2 aux0 K= N= M=',
    'old-fused-8-20x16x96': 'fused2 kb1 nb3 aux1 K< N= M< M<32',
    'old-fused-9-40000x128x32': 'fused2 kb4 nb1 aux0 K= N= M=',
    'old-fused-10-3000x32x192': 'fused2 kb1 nb6 aux1 K= N= M<',
    'old-fused-11-2100x32x192': 'fused2 kb1 nb6 aux0 K= N= M<',
    'old-fused-12-4000x192x32': 'fused2 kb6 nb1 aux0 K= N= M=',
    'old-fused-13-1500x64x96': 'fused2 kb2 nb3 aux1 K= N= M<',
    'old-fused-14-1500x96x64': 'fused2 kb3 nb2 aux0 K= N= M<',
    'old-fused-15-36000x24x144': 'fused2 kb1 nb5 aux1 K< N< M=',
}
