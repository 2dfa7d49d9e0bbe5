#!/usr/bin/env python3
"""Every entry point of the output head's six files (csrc/misc.hip, losstail.hip, evaltail.hip, crfunary.hip, mine.hip,
jaccard.hip) through capi on fixed seeded inputs — the A/B aid of a refactor of csrc/tailmath.h.  DL3_LIBPATH selects the library.

    head_entry_points.py --dump DIR          small shapes (the operator tests'), every output to DIR/<case>.<name>.npy
    head_entry_points.py --compare DIR DIR   byte comparison of two dumps; prints what differs (CPU only)
    head_entry_points.py --big --repeat 14   512 x 512 x 21 (B = 32 from 32 x 32 logits; Subpixel B = 16, r = 8), every
                                             launch K times: run under `rocprofv3 --kernel-trace`
    head_entry_points.py --table LABEL=DIR.. per-kernel median microseconds of such traces, one column per run (CPU only)
"""
import argparse
import csv
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_case(tag, C, Nb, Hi, Wi, Ho, Wo, Ns, H, W, r, repeat, big, out):
    import torch
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    L, ptr = capi.lib(), capi.ptr
    gen = torch.Generator(device="cuda").manual_seed(1000 + C)
    keep = []

    def randn(*shape):
        return 3.0 * torch.randn(*shape, device="cuda", generator=gen)

    def buf(shape, dtype=torch.float32, fill=float("nan")):
        t = torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device="cuda")
        keep.append(t)
        return t

    def call(name, *args):
        for _ in range(repeat):
            capi.call(name, *args, capi.stream())

    def save(name, *tensors):
        torch.cuda.synchronize()
        if out:
            for i, t in enumerate(tensors):
                np.save(os.path.join(out, "%s.%s.%d.npy" % (tag, name, i)), t.cpu().numpy())

    HWb, HWs = Ho * Wo, H * r * W * r
    x_lo, u = randn(Nb, Hi, Wi, C), randn(Ns, H, W, C * r * r)

    def targets(M):   # labels with void pixels, weights with zeros, the device-side normaliser
        lab = torch.randint(0, C + 1, (M + 1,), device="cuda", generator=gen).float()
        wgt = torch.rand(M + 1, device="cuda", generator=gen) * (torch.rand(M + 1, device="cuda", generator=gen) > 0.25)
        nnz = buf(1)
        call("dl3_count_nonzero", ptr(wgt), M, ptr(nnz))
        save("count_nonzero.%d" % M, nnz)
        return lab, wgt, nnz

    for form, N, HW, src in (("bilinear", Nb, HWb, x_lo), ("shuffle", Ns, HWs, u)):
        M = N * HW
        lab, wgt, nnz = targets(M)
        geo = (N, Hi, Wi, Ho, Wo, C) if form == "bilinear" else (N, H, W, C, r)
        full = buf(M * C)   # the materialised logits of this form: the plain entry points' input
        if form == "bilinear":
            capi.call("dl3_resize_bilinear_fwd", ptr(src), C, None, None, 0, ptr(full), C, N, Hi, Wi, Ho, Wo, C, capi.stream())
        else:
            capi.call("dl3_phase_shift", ptr(src), ptr(full), N, H, W, C, r, 0, capi.stream())
        save(form + ".materialised", full)
        # training loss tails
        P = L.dl3_rows_partials(M)
        if form == "bilinear":
            probs, dl, lp = buf(M * C), buf(M * C), buf(P)
            call("dl3_softmax_xent", ptr(full), ptr(lab), ptr(wgt), ptr(nnz), ptr(probs), ptr(dl), ptr(lp), M, C)
            save("softmax_xent", probs, dl, lp)
            call("dl3_upsample_softmax_xent", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(probs), ptr(dl), ptr(lp), *geo)
            save("upsample_softmax_xent", probs, dl, lp)
            xf, lpf = buf(N * Ho * Wi * C), buf(L.dl3_xent_fold_partials(N, Ho))
            for pref in ("1", "0"):
                os.environ["DL3_XENT_PREF"] = pref
                call("dl3_upsample_softmax_xent_fold", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(xf), ptr(lpf), *geo)
                save("xent_fold.pref" + pref, xf, lpf)
            del os.environ["DL3_XENT_PREF"]
            del probs
            # the focal loss in the same three forms (gamma = 2, one weight per class)
            alpha = 0.5 + 1.5 * torch.rand(C, device="cuda", generator=gen)
            keep.append(alpha)
            call("dl3_focal_xent", ptr(full), ptr(lab), ptr(wgt), ptr(nnz), ptr(alpha), 2.0, ptr(dl), ptr(lp), M, C)
            save("focal_xent", dl, lp)
            call("dl3_upsample_focal_xent", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(alpha), 2.0, ptr(dl), ptr(lp), *geo)
            save("upsample_focal_xent", dl, lp)
            for pref in ("1", "0"):
                os.environ["DL3_XENT_PREF"] = pref
                call("dl3_upsample_focal_xent_fold", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(alpha), 2.0, ptr(xf), ptr(lpf),
                     *geo)
                save("focal_fold.pref" + pref, xf, lpf)
            del os.environ["DL3_XENT_PREF"]
        else:
            du, lp = buf(src.numel()), buf(L.dl3_shuffle_xent_partials(*geo))
            call("dl3_shuffle_softmax_xent", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(du), ptr(lp), *geo)
            save("shuffle_softmax_xent", du, lp)
            alpha = 0.5 + 1.5 * torch.rand(C, device="cuda", generator=gen)
            keep.append(alpha)
            call("dl3_shuffle_focal_xent", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(alpha), 2.0, ptr(du), ptr(lp), *geo)
            save("shuffle_focal_xent", du, lp)
            dl = buf(M * C)
        # mining front
        v = buf(M)
        call("dl3_pixel_xent_" + form, ptr(src), ptr(lab), ptr(wgt), ptr(v), *geo)
        save("pixel_xent_" + form, v)
        ws_bytes = L.dl3_topk_workspace_bytes(M)
        ws, k, tau, wout, nout = buf(ws_bytes // 4, torch.int32, 0), buf(1, torch.int32, 0), buf(1), buf(M), buf(1)
        call("dl3_topk_threshold", ptr(v), M, 0.25, 0, None, ptr(ws), ws_bytes, ptr(k), ptr(tau))
        call("dl3_mine_weights", ptr(v), ptr(wgt), ptr(tau), ptr(k), ptr(wout), ptr(nout), ptr(ws), M)
        save("mine_" + form, k, tau, wout, nout)
        # soft-Jaccard
        Pj = L.dl3_jaccard_partials(N, HW)
        part, sums, coef, stats, row = (buf(N * Pj * 3 * C, torch.float64), buf(N * C * 3, torch.float64), buf(N * C * 2),
                                        buf(3, torch.float64), buf(1))
        lpj = buf(L.dl3_jaccard_loss_partials(N, HW))
        if form == "bilinear":
            call("dl3_jaccard_sums_bilinear", ptr(src), ptr(lab), ptr(wgt), ptr(part), *geo)
            call("dl3_jaccard_coef", ptr(part), Pj, N, C, 0.5, ptr(sums), ptr(coef), ptr(stats), ptr(row))
            call("dl3_upsample_softmax_xent_jaccard", ptr(src), ptr(lab), ptr(wgt), ptr(nnz), ptr(coef), 0.5, ptr(dl), ptr(lpj),
                 *geo)
            save("jaccard_bilinear", part, sums, coef, stats, row, dl, lpj)
        call("dl3_jaccard_sums_plain", ptr(full), ptr(lab), ptr(wgt), ptr(part), N, HW, C)
        call("dl3_jaccard_coef", ptr(part), Pj, N, C, 0.5, ptr(sums), ptr(coef), ptr(stats), ptr(row))
        call("dl3_softmax_xent_jaccard", ptr(full), ptr(lab), ptr(wgt), ptr(nnz), ptr(coef), 0.5, ptr(dl), ptr(lpj), N, HW, C)
        save("jaccard_plain." + form, part, sums, coef, stats, row, dl, lpj)
        # CRF unary (the full-size call takes a quarter of the batch: its planar output is as large as the logits)
        Bu = max(1, N // 4) if big else N
        U = dl   # reuse: [Bu][C][HW]
        ugeo = (Bu,) + geo[1:]
        call("dl3_crf_unary_" + form, ptr(src), ptr(U), *ugeo, 0.9, 1e-5)
        save("crf_unary_" + form, U[:Bu * C * HW])
        call("dl3_crf_unary_plain", ptr(full), 0, ptr(U), Bu, HW, C, 0.9, 1e-5)
        save("crf_unary_plain." + form, U[:Bu * C * HW])
        # evaluation tail: the form itself (every per-pixel buffer 16-byte aligned, then entered 4 bytes in) and plain
        for off in (0, 1):
            for f, s, g, Pe in ((form, src, geo, getattr(L, "dl3_eval_tail_%s_partials" % form)(*geo)),
                                ("plain", full, (N, HW, C), L.dl3_eval_tail_plain_partials(N, HW, C))):
                pe, ls, nz, cnt, conf, mask = (buf(N * Pe, torch.float64), buf(N, torch.float64), buf(N, torch.int32, -1),
                                               buf(N * 3 * C, torch.int32, -1), buf(C * C, torch.int64, 0),
                                               buf(M + 1, torch.int32, -1))
                call("dl3_eval_tail_" + f, ptr(s), ptr(lab, off), ptr(wgt, off), pe.data_ptr(), ls.data_ptr(), nz.data_ptr(),
                     cnt.data_ptr(), conf.data_ptr(), ptr(mask, off), *g)
                save("eval_tail_%s.%s.off%d" % (f, form, off), pe, ls, nz, cnt, conf, mask[off:off + M])
        torch.cuda.synchronize()
        del keep[:]


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = []
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        same = os.path.exists(pa) and os.path.exists(pb) and open(pa, "rb").read() == open(pb, "rb").read()
        if not same:
            x, y = (np.load(p) if os.path.exists(p) else None for p in (pa, pb))
            d = "missing" if x is None or y is None else "%d of %d values, max rel %.3e" % (
                (x != y).sum(), x.size, float(np.nanmax(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))))
            bad.append("%s: %s" % (n, d))
    print("%d files, %d differ" % (len(names), len(bad)))
    print("\n".join(bad))


def table(specs):
    cols = {}
    for spec in specs:
        label, d = spec.split("=", 1)
        per = {}
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                name = re.sub(r"^void |\(anonymous namespace\)::", "", row["Kernel_Name"]).split("(")[0]
                per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        cols[label] = per
    labels = list(cols)
    # one row per (kernel, launch site): a kernel launched from several entry points shows up as several equal-sized groups
    print("%-44s %6s " % ("kernel (median us of n launches)", "n") + " ".join("%10s" % l for l in labels))
    for k in sorted(set().union(*[set(c) for c in cols.values()])):
        n = min(len(c.get(k, [])) for c in cols.values())
        print("%-44s %6d " % (k[:44], n) + " ".join("%10.1f" % np.median(cols[l][k]) if k in cols[l] else "%10s" % "-"
                                                    for l in labels))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--table", nargs="+", metavar="LABEL=DIR")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.table:
        return table(a.table)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    if a.big:
        run_case("big21", 21, 32, 32, 32, 512, 512, 16, 64, 64, 8, a.repeat, True, a.dump)
    else:
        for C in (5, 21, 32):   # one per register row: MAXC = 8, 24, 32
            run_case("c%d.a" % C, C, 2, 6, 8, 20, 24, 2, 5, 6, 4, a.repeat, False, a.dump)     # 16-byte paths, prefetch form
            run_case("c%d.b" % C, C, 3, 7, 5, 21, 23, 3, 3, 5, 3, a.repeat, False, a.dump)     # odd sizes: the scalar paths


if __name__ == "__main__":
    main()
