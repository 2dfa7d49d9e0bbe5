"""Cost of hard-example mining (csrc/mine.hip).

  python tools/mine_step_profile.py step [--batch 16] [--size 512] [--steps 30] [--warmup 5] [--p 0.25] [--unmined-only]
      the training step (the captured fwd_bwd plan + Adam) of MobileNetV2 at size x size x 21 on a resident batch, one
      host-clock window closed by a device synchronise per measurement: unmined, mined (p, S = 0), unmined again — same
      process, same binary; the two unmined windows show the spread.  --unmined-only never passes the mining keyword:
      the form the parent commit's tree understands (the untouched path).
  python tools/mine_step_profile.py kernels [--batch 16] [--size 512] [--classes 21] [--reps 20] [--warmup 3]
      the new entry points on resident buffers, one device-event pair per call, the median of --reps calls: the
      per-pixel loss of the bilinear form (size/8 -> size), dl3_topk_threshold (its seven launches), dl3_mine_weights;
      with the algorithmic bytes and operations, bytes/s and FLOP/s, and the share of the nearer bound.
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


def _engine(a, mining):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session(seed=1)
    shape = (a.size, a.size, 3)
    model = Deeplabv3(weights=None, input_shape=shape, classes=21, backbone="mobilenetv2", OS=16)
    kw = {} if mining is None else dict(mining=mining)
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
    plan = [("unmined", None)] if a.unmined_only else [("unmined", None), ("mined p=%g" % a.p, (a.p, 0)), ("unmined", None)]
    print("training step, MobileNetV2 %d x %d x 21, B = %d: ms per step over %d steps after %d (host clock, device "
          "synchronise)" % (a.size, a.size, a.batch, a.steps, a.warmup))
    for label, mining in plan:
        model, eng = _engine(a, mining)
        ms = _time_steps(eng, a.steps, a.warmup)
        extra = ""
        if mining is not None:
            v, w2, tau, k, n = eng.mining_record()
            extra = "  k %d of %d, n' %d, tau %.4f, launches %d" % (k, v.size, n, tau, len(eng.ops_fwd) + len(eng.ops_bwd))
        else:
            extra = "  launches %d" % (len(eng.ops_fwd) + len(eng.ops_bwd))
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


def kernels(a):
    B, S, C = a.batch, a.size, a.classes
    Hi = S // 8
    N = B * S * S
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = 3 * torch.randn(B, Hi, Hi, C, device="cuda", generator=g)
    lab = torch.randint(0, C + 1, (N,), device="cuda", generator=g).to(torch.float32)
    w = (lab < C).to(torch.float32)
    v, w2 = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    nws = int(capi.lib().dl3_topk_workspace_bytes(N))
    ws = torch.zeros(nws // 4, dtype=torch.int32, device="cuda")
    k = torch.zeros(4, dtype=torch.int32, device="cuda")
    tau, nnz = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")

    def pixel():
        capi.call("dl3_pixel_xent_bilinear", lo.data_ptr(), lab.data_ptr(), w.data_ptr(), v.data_ptr(), B, Hi, Hi, S, S, C, st)

    def topk():
        capi.call("dl3_topk_threshold", v.data_ptr(), N, a.p, 0, None, ws.data_ptr(), nws, k.data_ptr(), tau.data_ptr(), st)

    def weights():
        capi.call("dl3_mine_weights", v.data_ptr(), w.data_ptr(), tau.data_ptr(), k.data_ptr(), w2.data_ptr(), nnz.data_ptr(),
                  ws.data_ptr(), N, st)

    # operations per pixel of the loss pass, counted from the source: 9 per interpolated logit (three lerps of a
    # subtract and a fused multiply-add), a subtract, an accurate expf (~20) and a double add per class, the maximum,
    # one double quotient, one double log (~60) and the product
    flop_pixel = N * (C * (9 + 1 + 20 + 1 + 1) + 70)
    rows = [("dl3_pixel_xent_bilinear", pixel, 4 * (3 * N + B * Hi * Hi * C), flop_pixel),
            ("dl3_topk_threshold (7 launches)", topk, 4 * 3 * N, 3 * 4 * N),
            ("dl3_mine_weights (2 launches)", weights, 4 * 3 * N, 3 * N)]
    print("mining kernels at B = %d, %d x %d x %d (N = %d pixels), p = %g: median (min - max) of %d calls after %d" % (
        B, S, S, C, N, a.p, a.reps, a.warmup))
    print("  %-34s %9s %22s %10s %8s %10s  %s" % ("entry point", "ms", "", "bytes", "TB/s", "TFLOP/s", "nearer bound"))
    for name, fn, nbytes, flop in rows:
        ms, lo_, hi_ = _median_ms(fn, a.reps, a.warmup)
        t = ms * 1e-3
        tb, tf = nbytes / COPY_RATE, flop / VALU_RATE
        bound = "HBM %.0f %%" % (100 * tb / t) if tb >= tf else "VALU %.0f %%" % (100 * tf / t)
        print("  %-34s %9.3f (%8.3f - %8.3f) %8.1f MB %8.2f %10.2f  %s" % (
            name, ms, lo_, hi_, nbytes / 1e6, nbytes / t / 1e12, flop / t / 1e12, bound))
    topk()      # one fresh pair: dl3_mine_weights counts into the workspace its dl3_topk_threshold call zeroed
    weights()
    torch.cuda.synchronize()
    print("  k %d, tau %.5f, n' %d" % (int(k[0].item()), float(tau[0].item()), int(nnz[0].item())))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernels"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--p", type=float, default=0.25)
    ap.add_argument("--unmined-only", action="store_true")
    a = ap.parse_args()
    {"step": step, "kernels": kernels}[a.mode](a)
