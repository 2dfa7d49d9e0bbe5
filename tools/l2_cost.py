"""Cost of the L2 weight penalty (csrc/l2reg.hip), by DESIGN.md §5's rules: warm-up, device events or a
host clock closed by a device synchronise, medians.

  python tools/l2_cost.py kernels [--reps 50] [--inner 10] [--warmup 5]
      over the real arenas of MobileNetV2 and Xception OS=8 (21 classes; utils.add_weight_decay's default table), on
      resident buffers, one device-event pair around --inner calls: the penalty launch pair (dl3_l2_penalty with the gradient addend:
      the tile kernel and its fold) and dl3_adam_step over the same arena in the same process, with the algorithmic bytes
      (penalty: p read, g read and written on the regularised elements, 12 bytes; Adam: 28 bytes per element).
  python tools/l2_cost.py step [--batch 16] [--size 512] [--steps 20] [--warmup 5] [--repeats 3] [--plain-only]
      the whole training step (the captured fwd_bwd plan, the penalty launches where there are any, Adam) on a resident
      batch, a host-clock window closed by a device synchronise, the median of --repeats windows: without the regulariser,
      with add_weight_decay(model), without again — same process, same binary; the two plain figures show the spread.
      --plain-only never sets a regulariser.
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

NETS = (("mobilenetv2", 16), ("xception", 8))


def _model(backbone, OS, size):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session(seed=1)
    return Deeplabv3(weights=None, input_shape=(size, size, 3), classes=21, backbone=backbone, OS=OS)


def _median_ms(fn, reps, warmup, inner):
    """ms per call: `inner` calls back to back inside one event pair (the launches take microseconds)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def kernels(a):
    from dl3_amd import utils as U
    print("penalty launch pair beside dl3_adam_step over the same arena: median (min - max) ms per call over %d event pairs of %d "
          "calls each after %d" % (a.reps, a.inner, a.warmup))
    print("  %-18s %-28s %9s %22s %10s %8s" % ("arena", "launch", "ms", "", "bytes", "TB/s"))
    for backbone, OS in NETS:
        model = _model(backbone, OS, 128)
        covered = U.add_weight_decay(model)
        model.compile()
        eng = model._engine(1, True, use_graph=False)
        tab = eng._l2["arenas"][0]
        reg = int(tab["runs"][:, 1].sum().item())
        n = eng.n_param
        eng.grads.normal_(0, 1e-3)

        def adam():
            capi.call("dl3_adam_step", capi.ptr(eng.params), capi.ptr(eng.grads), capi.ptr(eng.adam_m), capi.ptr(eng.adam_v),
                      n, 1e-9, 0.9, 0.999, 1e-8, 1.0, capi.stream())
        rows = (("dl3_l2_penalty (+ fold)", lambda: eng.l2_penalty(1.0), 12 * reg), ("dl3_adam_step", adam, 28 * n))
        label = "%s OS=%d" % (backbone, OS)
        t0 = None
        for name, fn, nbytes in rows:
            ms, lo, hi = _median_ms(fn, a.reps, a.warmup, a.inner)
            print("  %-18s %-28s %9.4f (%8.4f - %8.4f) %8.1f MB %8.2f%s" % (
                label, name, ms, lo, hi, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, "" if t0 is None else "   penalty / adam = %.3f" % (t0 / ms)))
            t0 = ms if t0 is None else t0
        print("  %-18s %d weights, %d runs, %d tiles, %d of %d arena elements regularised" % (
            "", covered, tab["S"], tab["tiles"], reg, n))
        del model, eng
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _time_steps(eng, steps, warmup, repeats):
    def run(k):
        for _ in range(k):
            eng.fwd_bwd()
            eng.l2_penalty(1.0)
            eng.adam(None, 1.0)
        torch.cuda.synchronize()
    run(warmup)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def step(a):
    plan = ["without"] if a.plain_only else ["without", "with add_weight_decay", "without"]
    print("training step at %d x %d x 21, B = %d: median (min - max) ms per step of %d windows of %d steps after %d (host "
          "clock, device synchronise)" % (a.size, a.size, a.batch, a.repeats, a.steps, a.warmup))
    for backbone, OS in NETS:
        for label in plan:
            model = _model(backbone, OS, a.size)
            if label != "without":
                from dl3_amd import utils as U
                U.add_weight_decay(model)
            model.compile()
            eng = model._engine(a.batch, True, dropout=True)
            rng = np.random.default_rng(1000)
            x = rng.integers(0, 256, (a.batch, a.size, a.size, 3)).astype(np.float32)
            y = rng.integers(0, 22, (a.batch, a.size * a.size)).astype(np.float32)   # 21 = void
            eng.set_input(x)
            eng.set_targets(y, (y < 21).astype(np.float32))
            ms, lo, hi = _time_steps(eng, a.steps, a.warmup, a.repeats)
            print("  %-12s OS=%-2d %-22s %9.3f (%9.3f - %9.3f) ms  loss %.9g  regularised weights %d" % (
                backbone, OS, label, ms, lo, hi, eng.loss_value(), len(eng.l2 or ())))
            del model, eng
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "kernels"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    {"step": step, "kernels": kernels}[a.mode](a)
