"""Cost of the soft-Jaccard loss (csrc/jaccard.hip).

  python tools/jaccard_step_profile.py step [--batch 16] [--size 512] [--steps 30] [--warmup 5] [--weight 1.0] [--plain-only]
      the training step (the captured fwd_bwd plan + Adam) of MobileNetV2 at size x size x 21 on a resident batch, one
      host-clock window closed by a device synchronise per measurement: cross-entropy, cross-entropy + weight * L_J,
      cross-entropy again — same process, same binary; the two cross-entropy windows show the spread.  --plain-only
      never passes the jaccard keyword: the form the parent commit's tree understands (the untouched path).
  python tools/jaccard_step_profile.py kernels [--batch 16] [--size 512] [--classes 21] [--reps 20] [--warmup 3]
      the new entry points on resident buffers, one device-event pair per call, the median of --reps calls: the sums pass
      and the loss + gradient pass of both forms (bilinear: size/8 -> size), dl3_jaccard_coef (its two launches), and
      beside them today's dl3_upsample_softmax_xent_fold and the resize backward the unfolded gradient needs; with the
      algorithmic bytes and operations, bytes/s and FLOP/s, and the share of the nearer bound.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl3_amd  # noqa: E402,F401
from dl3_amd import capi  # noqa: E402

COPY_RATE = 6.3e12    # bytes / s: the achievable HBM copy rate the project measures against
VALU_RATE = 157.3e12  # FLOP / s: fp32 vector peak (MI355X_MICROARCH)


def _engine(a, weight):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session(seed=1)
    shape = (a.size, a.size, 3)
    model = Deeplabv3(weights=None, input_shape=shape, classes=21, backbone="mobilenetv2", OS=16)
    kw = {} if weight is None else dict(jaccard=weight)
    eng = model._engine(a.batch, True, dropout=True, **kw)
    rng = np.random.default_rng(1000)
    x = rng.integers(0, 256, (a.batch,) + shape).astype(np.float32)
    y = rng.integers(0, 22, (a.batch, a.size * a.size)).astype(np.float32)   # 21 = void
    eng.set_input(x)
    eng.set_targets(y, (y < 21).astype(np.float32))
    return model, eng


def _time_steps(eng, steps, warmup):
    for _ in range(warmup):
        eng.fwd_bwd()
        eng.adam(None, 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.fwd_bwd()
        eng.adam(None, 1.0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def step(a):
    plain = ("cross-entropy", None)
    plan = [plain] if a.plain_only else [plain, ("+ %g * L_J" % a.weight, a.weight), plain]
    print("training step, MobileNetV2 %d x %d x 21, B = %d: ms per step over %d steps after %d (host clock, device "
          "synchronise)" % (a.size, a.size, a.batch, a.steps, a.warmup))
    for label, weight in plan:
        model, eng = _engine(a, weight)
        ms = _time_steps(eng, a.steps, a.warmup)
        extra = "  launches %d" % (len(eng.ops_fwd) + len(eng.ops_bwd))
        if weight is not None:
            _, _, lj, ce = eng.jaccard_record()
            extra += ", cross-entropy %.6f, L_J %.6f" % (ce, lj)
        print("  %-14s %9.3f ms  loss %.6f%s" % (label, ms, eng.loss_value(), extra))
        del model, eng
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def call(name, *args):
    """capi.call behind a count of the arguments: ctypes passes surplus ones on, and every later one then lands in the
    wrong slot (a byte count where the stream handle belongs)"""
    want = len(capi.protos()[name][1])
    if len(args) != want:
        raise TypeError("%s takes %d arguments, got %d" % (name, want, len(args)))
    capi.call(name, *args)


def kernels(a):
    B, S, C = a.batch, a.size, a.classes
    Hi, HW = S // 8, S * S
    N = B * HW
    L = capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = 3 * torch.randn(B, Hi, Hi, C, device="cuda", generator=g)
    full = 3 * torch.randn(N, C, device="cuda", generator=g)
    lab = torch.randint(0, C + 1, (N,), device="cuda", generator=g).to(torch.float32)
    w = (lab < C).to(torch.float32)
    nnz = torch.full((4,), float(w.sum().item()), device="cuda")
    P, LP = L.dl3_jaccard_partials(B, HW), L.dl3_jaccard_loss_partials(B, HW)
    part = torch.zeros(B * P * 3 * C, dtype=torch.float64, device="cuda")
    sums = torch.zeros(B * C * 3, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    coef = torch.zeros(B * C * 2, device="cuda")
    grad = torch.empty(N * C, device="cuda")
    lpart = torch.zeros(max(LP, L.dl3_xent_fold_partials(B, S), L.dl3_rows_partials(N)) + 1, device="cuda")
    xfold = torch.empty(B * S * Hi * C, device="cuda")
    dlo = torch.empty(B * Hi * Hi * C, device="cuda")
    nws = int(L.dl3_resize_bilinear_bwd_workspace(B, Hi, Hi, S, S, C))
    ws = torch.empty(max((nws + 3) // 4, 4), device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731

    def sums_bil():
        call("dl3_jaccard_sums_bilinear", p(lo), p(lab), p(w), p(part), B, Hi, Hi, S, S, C, st)

    def sums_plain():
        call("dl3_jaccard_sums_plain", p(full), p(lab), p(w), p(part), B, HW, C, st)

    def coefs():
        call("dl3_jaccard_coef", p(part), P, B, C, 1.0, p(sums), p(coef), p(stats), p(lpart) + 4 * LP, st)

    def loss_bil():
        call("dl3_upsample_softmax_xent_jaccard", p(lo), p(lab), p(w), p(nnz), p(coef), 1.0, p(grad), p(lpart), B, Hi, Hi,
                  S, S, C, st)

    def loss_plain():
        call("dl3_softmax_xent_jaccard", p(full), p(lab), p(w), p(nnz), p(coef), 1.0, p(grad), p(lpart), B, HW, C, st)

    def fold_today():
        call("dl3_upsample_softmax_xent_fold", p(lo), p(lab), p(w), p(nnz), p(xfold), p(lpart), B, Hi, Hi, S, S, C, st)

    def rows_today():
        call("dl3_resize_bilinear_bwd_rows", p(xfold), p(dlo), C, B, Hi, Hi, S, C, 0, st)

    def resize_bwd():
        call("dl3_resize_bilinear_bwd", p(grad), C, p(dlo), C, B, Hi, Hi, S, S, C, 0, p(ws), nws, st)

    # operations per pixel, counted from the source: 9 per interpolated logit (three lerps of a subtract and a fused
    # multiply-add), a subtract and an accurate expf (~20) per class and the maximum; the sums pass adds three double
    # operations per class (counted twice each), the loss pass ~8 per class for the two gradient halves and a logf (~20)
    lo_bytes = 4 * B * Hi * Hi * C
    f_soft, f_lerp = C * (1 + 20 + 1), C * 9
    rows = [("dl3_jaccard_sums_bilinear", sums_bil, 8 * N + lo_bytes, N * (f_lerp + f_soft + 6 * C)),
            ("dl3_jaccard_sums_plain", sums_plain, (4 * C + 8) * N, N * (f_soft + 6 * C)),
            ("dl3_jaccard_coef (2 launches)", coefs, 8 * B * P * 3 * C, 40 * B * C),
            ("dl3_upsample_softmax_xent_jaccard", loss_bil, (4 * C + 8) * N + lo_bytes, N * (f_lerp + f_soft + 8 * C + 20)),
            ("dl3_softmax_xent_jaccard", loss_plain, (8 * C + 8) * N, N * (f_soft + 8 * C + 20)),
            ("dl3_resize_bilinear_bwd (unfolded)", resize_bwd, 4 * C * N + lo_bytes, 0),
            ("today: ..._softmax_xent_fold", fold_today, 8 * N + lo_bytes + 4 * B * S * Hi * C, N * (f_lerp + f_soft + 4 * C + 20)),
            ("today: ..._bilinear_bwd_rows", rows_today, 4 * B * S * Hi * C + lo_bytes, 0)]
    print("soft-Jaccard kernels at B = %d, %d x %d x %d (N = %d pixels): median (min - max) of %d calls after %d" % (
        B, S, S, C, N, a.reps, a.warmup))
    print("  %-36s %9s %22s %10s %8s %10s  %s" % ("entry point", "ms", "", "bytes", "TB/s", "TFLOP/s", "nearer bound"))
    for name, fn, nbytes, flop in rows:
        ms, lo_, hi_ = _median_ms(fn, a.reps, a.warmup)
        t = ms * 1e-3
        tb, tf = nbytes / COPY_RATE, flop / VALU_RATE
        bound = "HBM %.0f %%" % (100 * tb / t) if tb >= tf else "VALU %.0f %%" % (100 * tf / t)
        print("  %-36s %9.3f (%8.3f - %8.3f) %8.1f MB %8.2f %10.2f  %s" % (
            name, ms, lo_, hi_, nbytes / 1e6, nbytes / t / 1e12, flop / t / 1e12, bound))
    sums_bil()
    coefs()
    torch.cuda.synchronize()
    print("  L_J %.6f, classes present %d, partial rows per image %d" % (float(stats[0].item()), int(stats[1].item()), P))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernels"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    {"step": step, "kernels": kernels}[a.mode](a)
