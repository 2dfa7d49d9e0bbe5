#!/usr/bin/env python3
"""Bit digests of the depthwise 3x3 operators on every case of tests/dwconv_cases.CASES, for comparing two builds of the
library (a refactor of csrc/dwconv.hip must not move a bit).

    DL3_LIBPATH=build_variants/parent/libdl3.so python tools/dw_bits.py -o A.txt      (GPU; a fresh process per library)
    python tools/dw_bits.py -o B.txt
    python tools/dw_bits.py --verdict A.txt B.txt -o profiles/dwconv_refactor_bits.txt   (no GPU)

One line per case, on the inputs tests/test_gpu_dwconv.py draws for it (same seeds, same order, the case's DL3_DW_PPB):
the SHA-256 (first 16 hex digits) of y, of all rows of the forward BatchNorm partials, and per backward entry point
(dl3_dwconv3x3_bwd, and dl3_dwconv3x3_bwd_sx for an sx case) of dx, of all weight-gradient partial rows and of all
BatchNorm-sum partial rows.  An output the case does not have (no statistics, no dx) reads `-`."""
import argparse
import hashlib
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def verdict(a, b, out):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    diff = [x.split()[0] for x, y in zip(la, lb) if x != y]
    same = la == lb
    text = "\n".join(la + ["# %s vs %s: %d lines each, %s" % (
        a, b, len(la), "IDENTICAL" if same else "DIFFERENT (%d vs %d lines; first cases: %s)" % (len(la), len(lb), diff[:5]))]) + "\n"
    sys.stdout.write(text.splitlines()[-1] + "\n")
    if out:
        open(out, "w").write(text)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--verdict", nargs=2, metavar=("A", "B"), help="compare two digest files instead of running")
    ap.add_argument("-o", "--output", default=None)
    a = ap.parse_args()
    if a.verdict:
        return verdict(a.verdict[0], a.verdict[1], a.output)

    import numpy as np
    import torch
    from tests import dwconv_cases as D
    from tests.gpu_util import call, dev, ptr, release

    def sha(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] if t is not None else "-"

    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    lines = []
    for case in D.CASES:
        if case.ppb is None:
            os.environ.pop("DL3_DW_PPB", None)
        else:
            os.environ["DL3_DW_PPB"] = str(case.ppb)
        geom, impl = case.geom, case.impl
        N, H, W, C, stride, rate, pt, pl, Ho, Wo = geom
        P = D.plan_of(case).Pmax
        # the draws of tests/test_gpu_dwconv.py::_drive, in its order
        rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 1)
        x, s, t, act, _ = D.draw_view(case)
        w = rng.normal(0, 0.3, (3, 3, C)).astype(np.float32)
        xd, wd = dev(x), dev(w)
        view = (ptr(dev(s)), ptr(dev(t)), act) if s is not None else (None, None, act)
        y = nan(N, Ho, Wo, C)
        part = nan(P, C, 2) if case.stats else None
        call("dl3_dwconv3x3_fwd", ptr(xd), *view, ptr(wd), ptr(y), *geom, ptr(part) if case.stats else None, impl)
        out = ["y", sha(y), "part", sha(part)]
        g = rng.normal(0, 1, (N, Ho, Wo, C)).astype(np.float32)
        if case.grad == "bn":
            yraw = rng.normal(0, 1, g.shape).astype(np.float32)
            cA, cB, cC = [rng.normal(0, 1, C).astype(np.float32) for _ in range(3)]
            operand = (ptr(dev(yraw)), ptr(dev(cA)), ptr(dev(cB)), ptr(dev(cC)))
        else:
            operand = (None, None, None, None)
        add = rng.normal(0, 1, x.shape).astype(np.float32) if case.add else None
        mean = rng.normal(0, 1, C).astype(np.float32)
        invstd = rng.uniform(0.5, 2, C).astype(np.float32)
        other = rng.normal(0, 1, x.shape).astype(np.float32) if case.sx else None
        head = (ptr(dev(g)), *operand, ptr(xd), *view, ptr(wd))
        addp, meanp, invp = ptr(dev(add)) if case.add else None, ptr(dev(mean)), ptr(dev(invstd))
        for sx in ((False, True) if case.sx else (False,)):
            dx = nan(N, H, W, C) if case.dx else None
            dpart = nan(P, C, 2) if case.stats else None
            wpart = nan(P, 9, C)
            stat = (meanp, invp, ptr(dpart)) if case.stats else (None, None, None)
            mid = (ptr(dx) if case.dx else None, addp) + ((ptr(dev(other)),) if sx else ())
            call("dl3_dwconv3x3_bwd_sx" if sx else "dl3_dwconv3x3_bwd", *head, *mid, *stat, ptr(wpart), *geom, impl)
            out += ["bwd_sx" if sx else "bwd", "dx", sha(dx), "wpart", sha(wpart), "dpart", sha(dpart)]
        lines.append("%-36s %s" % (case.id, " ".join(out)))
        release()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.output:
        open(a.output, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
