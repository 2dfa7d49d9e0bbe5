"""Cost of multi-scale / flip inference (csrc/tta.hip, tta.py).

  python tools/tta_profile.py kernels [--batch 8] [--size 512] [--classes 21] [--reps 20] [--warmup 3]
      dl3_tta_accumulate and dl3_tta_resize_image between size x size and every pass size of the default scales, on
      resident buffers: one device-event pair per launch, the median of --reps launches after --warmup.  Prints ms per
      pass, the algorithmic bytes, bytes over time and that as a fraction of the 6.3 TB/s copy rate.
  python tools/tta_profile.py predict [--batch 8] [--size 512] [--classes 21] [--reps 5]
      one Model.predict_multiscale call (MobileNetV2, default six scales and flip, output="mask", images resident on the
      device) beside the sum of its twelve forward passes (forward plan + softmax of each pass size on its own).
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl3_amd  # noqa: E402,F401
from dl3_amd import capi, tta  # noqa: E402

COPY_RATE = 6.3e12   # bytes / s: the achievable HBM copy rate the project measures against


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
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    acc = torch.rand(B, S, S, C, device="cuda", generator=g)
    img = (255 * torch.rand(B, S, S, 3, device="cuda", generator=g)).to(torch.uint8)
    imgf = img.to(torch.float32)
    sizes = sorted({tta.scaled_size(S, s) for s in tta.DEFAULT_SCALES})
    print("dl3_tta_accumulate into %d x %d x %d, B = %d: median (min - max) of %d launches after %d warm-up" % (
        S, S, C, B, a.reps, a.warmup))
    print("  %-28s %9s %20s %10s %8s %8s" % ("pass", "ms", "", "bytes", "TB/s", "of 6.3"))
    for hs in sizes:
        p = torch.softmax(torch.randn(B, hs, hs, C, device="cuda", generator=g), -1)
        for label, first, nlast in (("first (store)", 1, 0), ("middle (add)", 0, 0), ("last (add, divide)", 0, 12)):
            def fn(p=p, hs=hs, first=first, nlast=nlast):
                capi.call("dl3_tta_accumulate", p.data_ptr(), acc.data_ptr(), B, hs, hs, S, S, C, 1, first, nlast, st)
            ms, lo, hi = _median_ms(fn, a.reps, a.warmup)
            nbytes = 4 * C * B * ((1 if first else 2) * S * S + hs * hs)
            print("  %4d -> %-4d %-18s %9.3f (%7.3f - %7.3f) %8.1f MB %8.2f %8.2f" % (
                hs, S, label, ms, lo, hi, nbytes / 1e6, nbytes / ms / 1e9, nbytes / (ms * 1e-3) / COPY_RATE))
            acc.uniform_(generator=g)   # keep the accumulator finite across hundreds of adds
        del p
    print("dl3_tta_resize_image from %d x %d x 3, B = %d" % (S, S, B))
    for hs in sizes:
        dst = torch.empty(B, hs, hs, 3, device="cuda")
        for label, src, eb in (("uint8", img, 1), ("float32", imgf, 4)):
            def fn(src=src, dst=dst, hs=hs, eb=eb):
                capi.call("dl3_tta_resize_image", src.data_ptr(), 1 if eb == 1 else 0, dst.data_ptr(), B, S, S, hs, hs, 1, st)
            ms, lo, hi = _median_ms(fn, a.reps, a.warmup)
            nbytes = B * 3 * (eb * S * S + 4 * hs * hs)
            print("  %4d -> %-4d %-18s %9.3f (%7.3f - %7.3f) %8.1f MB %8.2f %8.2f" % (
                S, hs, label, ms, lo, hi, nbytes / 1e6, nbytes / ms / 1e9, nbytes / (ms * 1e-3) / COPY_RATE))


def predict(a):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    B, S, C = a.batch, a.size, a.classes
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=(S, S, 3), classes=C, backbone="mobilenetv2")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (255 * torch.rand(B, S, S, 3, device="cuda", generator=g)).to(torch.uint8)

    def call():
        t0 = time.perf_counter()
        model.predict_multiscale(x, batch_size=B, output="mask")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):   # builds the siblings; the engines capture their hipGraph on the second forward
        call()
    ts = [call() for _ in range(a.reps)]
    whole = statistics.median(ts)
    print("predict_multiscale, MobileNetV2 %d x %d x %d, B = %d, scales %s and flip, output = mask, images on the device" % (
        S, S, C, B, tta.DEFAULT_SCALES))
    print("  whole call: median %.2f ms (min %.2f, max %.2f) of %d calls = %.2f ms per image" % (
        whole, min(ts), max(ts), a.reps, whole / B))
    total = 0.0
    for s, hs, ws, flipped in tta.pass_list((S, S), tta.DEFAULT_SCALES, False):
        eng = (model if (hs, ws) == (S, S) else tta.sibling(model, hs, ws))._engine(B, False)
        ms, lo, hi = _median_ms(lambda eng=eng: eng.probs_device(), a.reps, 2)
        total += 2 * ms
        print("  forward + softmax at %4d x %-4d %8.3f ms (%.3f - %.3f), twice" % (hs, ws, ms, lo, hi))
    print("  sum of the twelve forward passes %.2f ms; the call's remainder %.2f ms (resize, accumulate, argmax, weight "
          "hand-over, host launch path, mask copy)" % (total, whole - total))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "predict"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_profile: needs a GPU; nothing is measured without one")
    if a.reps is None:
        a.reps = 20 if a.mode == "kernels" else 5
    {"kernels": kernels, "predict": predict}[a.mode](a)
