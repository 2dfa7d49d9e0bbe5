"""Cost of the focal loss (csrc/losstail.hip).

  python tools/focal_step_profile.py step [--batch 16] [--size 512] [--steps 30] [--warmup 5] [--gamma 2.0] [--plain-only]
      the training step (the captured fwd_bwd plan + Adam) of MobileNetV2 at size x size x 21 on a resident batch, one
      host-clock window closed by a device synchronise per measurement: cross-entropy, focal (gamma, 21 class weights),
      cross-entropy again — same process, same binary; the two cross-entropy windows show the spread.  --plain-only
      never passes the focal keyword: the form the parent commit's tree understands (the untouched path).
  python tools/focal_step_profile.py kernels [--batch 16] [--size 512] [--classes 21] [--reps 20] [--warmup 3]
      the four focal entry points beside their cross-entropy counterparts on resident buffers, one device-event pair per
      call, the median of --reps calls, with the algorithmic bytes and bytes/s (bilinear: size/8 -> size; shuffle: r = 8).
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


def _engine(a, focal):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session(seed=1)
    shape = (a.size, a.size, 3)
    model = Deeplabv3(weights=None, input_shape=shape, classes=21, backbone="mobilenetv2", OS=16)
    kw = {} if focal is None else dict(focal=focal)
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
    alpha = tuple(float(v) for v in np.linspace(0.5, 2.0, 21))
    plan = [plain] if a.plain_only else [plain, ("focal gamma %g" % a.gamma, (a.gamma, alpha)), plain]
    print("training step, MobileNetV2 %d x %d x 21, B = %d: ms per step over %d steps after %d (host clock, device "
          "synchronise)" % (a.size, a.size, a.batch, a.steps, a.warmup))
    for label, focal in plan:
        model, eng = _engine(a, focal)
        ms = _time_steps(eng, a.steps, a.warmup)
        loss = [r[0] for r in eng.ops_fwd if "xent" in r[0]]
        print("  %-16s %9.3f ms  loss %.9g  launches %d  %s" % (label, ms, eng.loss_value(), len(eng.ops_fwd) + len(eng.ops_bwd),
                                                                " ".join(loss)))
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
    """capi.call behind a count of the arguments (ctypes passes surplus ones on)"""
    want = len(capi.protos()[name][1])
    if len(args) != want:
        raise TypeError("%s takes %d arguments, got %d" % (name, want, len(args)))
    capi.call(name, *args)


def kernels(a):
    B, S, C, r = a.batch, a.size, a.classes, 8
    Hi, HW = S // 8, S * S
    N = B * HW
    L = capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = 3 * torch.randn(B, Hi, Hi, C, device="cuda", generator=g)
    full = 3 * torch.randn(N, C, device="cuda", generator=g)    # also the unshuffled Subpixel output [B,S/r,S/r,C*r*r]
    lab = torch.randint(0, C + 1, (N,), device="cuda", generator=g).to(torch.float32)
    w = (lab < C).to(torch.float32)
    nnz = torch.full((4,), float(w.sum().item()), device="cuda")
    alpha = 0.5 + 1.5 * torch.rand(C, device="cuda", generator=g)
    grad = torch.empty(N * C, device="cuda")
    Ps = L.dl3_shuffle_xent_partials(B, S // r, S // r, C, r)
    lpart = torch.zeros(max(L.dl3_xent_fold_partials(B, S), L.dl3_rows_partials(N), Ps), device="cuda")
    xfold = torch.empty(B * S * Hi * C, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731
    head = (p(lab), p(w), p(nnz))
    bil, shf = (B, Hi, Hi, S, S, C, st), (B, S // r, S // r, C, r, st)
    lo_bytes = 4 * B * Hi * Hi * C
    rows = [
        ("plain", "dl3_softmax_xent", lambda: call("dl3_softmax_xent", p(full), *head, None, p(grad), p(lpart), N, C, st),
         "dl3_focal_xent", lambda: call("dl3_focal_xent", p(full), *head, p(alpha), 2.0, p(grad), p(lpart), N, C, st),
         (8 * C + 8) * N),
        ("bilinear", "dl3_upsample_softmax_xent",
         lambda: call("dl3_upsample_softmax_xent", p(lo), *head, None, p(grad), p(lpart), *bil),
         "dl3_upsample_focal_xent", lambda: call("dl3_upsample_focal_xent", p(lo), *head, p(alpha), 2.0, p(grad), p(lpart), *bil),
         (4 * C + 8) * N + lo_bytes),
        ("bilinear_fold", "dl3_upsample_softmax_xent_fold",
         lambda: call("dl3_upsample_softmax_xent_fold", p(lo), *head, p(xfold), p(lpart), *bil),
         "dl3_upsample_focal_xent_fold",
         lambda: call("dl3_upsample_focal_xent_fold", p(lo), *head, p(alpha), 2.0, p(xfold), p(lpart), *bil),
         8 * N + lo_bytes + 4 * B * S * Hi * C),
        ("shuffle", "dl3_shuffle_softmax_xent", lambda: call("dl3_shuffle_softmax_xent", p(full), *head, p(grad), p(lpart), *shf),
         "dl3_shuffle_focal_xent", lambda: call("dl3_shuffle_focal_xent", p(full), *head, p(alpha), 2.0, p(grad), p(lpart), *shf),
         (8 * C + 8) * N),
    ]
    print("loss tails at B = %d, %d x %d x %d (N = %d pixels), gamma = 2, %d class weights: median (min - max) ms of %d calls "
          "after %d; bytes: the algorithmic traffic (the focal form adds %d bytes of alpha per workgroup)" % (
              B, S, S, C, N, C, a.reps, a.warmup, 4 * C))
    print("  %-14s %-32s %9s %22s %10s %8s %7s" % ("form", "entry point", "ms", "", "bytes", "TB/s", "HBM"))
    for form, n0, f0, n1, f1, nbytes in rows:
        t0 = None
        for name, fn in ((n0, f0), (n1, f1)):
            ms, lo_, hi_ = _median_ms(fn, a.reps, a.warmup)
            t = ms * 1e-3
            print("  %-14s %-32s %9.3f (%8.3f - %8.3f) %8.1f MB %8.2f %5.0f %%%s" % (
                form, name, ms, lo_, hi_, nbytes / 1e6, nbytes / t / 1e12, 100 * nbytes / COPY_RATE / t,
                "" if t0 is None else "   x %.3f" % (t / t0)))
            t0 = t if t0 is None else t0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernels"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    {"step": step, "kernels": kernels}[a.mode](a)
