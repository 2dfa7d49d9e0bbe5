"""Cost of sliding-window inference (csrc/slide.hip, slide.py).

  python tools/slide_profile.py kernels [--window 512] [--classes 21] [--batch 8] [--reps 20] [--warmup 3]
      dl3_slide_gather, dl3_slide_accumulate and dl3_slide_finalize on resident buffers for images of 512 x 512,
      1024 x 2048 and 375 x 500, both blends, in the launches Model.predict_sliding issues at that batch size: one
      device-event pair per launch, the median of --reps launches after --warmup.  Prints ms per launch, the algorithmic
      bytes, bytes over time and that as a fraction of the 6.3 TB/s copy rate.  Then the yardstick: dl3_tta_accumulate's
      middle pass at window -> window beside dl3_slide_accumulate on a fully covered chunk, the two alternating in one
      loop.
  python tools/slide_profile.py predict [--window 512] [--classes 21] [--batch 8] [--reps 5]
      one Model.predict_sliding(output="mask") call on a 1024 x 2048 image (MobileNetV2, default stride, image resident
      on the device) beside Model.predict_mask on the same number of window-sized images: the difference is what the cut,
      the blend and the arg-max at image size cost.
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
from dl3_amd import capi, slide  # noqa: E402

COPY_RATE = 6.3e12   # bytes / s: the achievable HBM copy rate the project measures against
SIZES = ((512, 512), (1024, 2048), (375, 500))


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = [_timed(fn) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def _line(label, ms, lo, hi, nbytes):
    print("  %-44s %9.3f (%7.3f - %7.3f) %9.1f MB %7.2f %6.2f" % (label, ms, lo, hi, nbytes / 1e6, nbytes / ms / 1e9,
                                                                 nbytes / (ms * 1e-3) / COPY_RATE))


def _touched(size, window, stride, k0, nw):
    """canvas pixels under the windows k0 .. k0 + nw - 1"""
    m = np.zeros(size, bool)
    for y0, x0 in slide.grid(size, window, stride)[2][k0:k0 + nw]:
        m[y0:y0 + window[0], x0:x0 + window[1]] = True
    return int(m.sum())


def kernels(a):
    S, C, B = a.window, a.classes, a.batch
    window, stride = (S, S), slide.default_stride((S, S))
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    probs = torch.softmax(torch.randn(B, S, S, C, device="cuda", generator=g), -1)
    xbuf = torch.empty(B, S, S, 3, device="cuda")
    print("window %d x %d, stride %s, C = %d, launches of up to %d windows: median (min - max) of %d launches after %d warm-up" % (
        S, S, stride, C, B, a.reps, a.warmup))
    print("  %-44s %9s %20s %12s %7s %6s" % ("launch", "ms", "", "bytes", "TB/s", "of 6.3"))
    for size in SIZES:
        Hi, Wi = size
        ny, nx, _ = slide.grid(size, window, stride)
        img = (255 * torch.rand(Hi, Wi, 3, device="cuda", generator=g)).to(torch.uint8)
        acc = torch.zeros(Hi, Wi, C, device="cuda")
        mask = torch.empty(Hi, Wi, dtype=torch.int32, device="cuda")
        print("image %d x %d: %d x %d windows" % (Hi, Wi, ny, nx))
        cuts = [(k0, min(B, ny * nx - k0)) for k0 in range(0, ny * nx, B)]
        for k0, nw in cuts:
            def fn():
                capi.call("dl3_slide_gather", img.data_ptr(), 1, Hi, Wi, S, S, stride[0], stride[1], k0, nw, 127.5,
                          xbuf.data_ptr(), st)
            ms, lo, hi = _median_ms(fn, a.reps, a.warmup)
            _line("gather uint8, windows %d..%d" % (k0, k0 + nw - 1), ms, lo, hi, 3 * (_touched(size, window, stride, k0, nw)
                                                                                  + 4 * nw * S * S))
        for blend in ("uniform", "pyramid"):
            for k0, nw in cuts:
                def fn():
                    capi.call("dl3_slide_accumulate", probs.data_ptr(), acc.data_ptr(), None, Hi, Wi, S, S, C, stride[0],
                              stride[1], k0, nw, slide.BLENDS[blend], st)
                ms, lo, hi = _median_ms(fn, a.reps, a.warmup)
                _line("accumulate %s, windows %d..%d" % (blend, k0, k0 + nw - 1), ms, lo, hi,
                      4 * C * (nw * S * S + 2 * _touched(size, window, stride, k0, nw)))
                acc.zero_()
            for label, pout, pmask, nbytes in (("finalize %s -> mask" % blend, None, mask.data_ptr(), Hi * Wi * (4 * C + 4)),
                                               ("finalize %s -> probabilities in place" % blend, acc.data_ptr(), None,
                                                Hi * Wi * 8 * C)):
                acc.uniform_(generator=g)

                def fn():
                    capi.call("dl3_slide_finalize", acc.data_ptr(), None, pout, pmask, Hi, Wi, S, S, C, stride[0], stride[1],
                              slide.BLENDS[blend], st)
                ms, lo, hi = _median_ms(fn, a.reps, a.warmup)
                _line(label, ms, lo, hi, nbytes)
        del img, acc, mask

    # the yardstick: the same kind of [pixel][C] rows, moved by dl3_tta_accumulate's middle pass (B windows resized window
    # -> window and added) and by dl3_slide_accumulate on the first chunk of the 1024 x 2048 image, alternating
    Hi, Wi = 1024, 2048
    nw = min(B, len(slide.grid((Hi, Wi), window, stride)[2]))
    acc_t = torch.rand(B, S, S, C, device="cuda", generator=g)
    acc_s = torch.zeros(Hi, Wi, C, device="cuda")

    def f_tta():
        capi.call("dl3_tta_accumulate", probs.data_ptr(), acc_t.data_ptr(), B, S, S, S, S, C, 0, 0, 0, st)

    def f_slide(blend):
        capi.call("dl3_slide_accumulate", probs.data_ptr(), acc_s.data_ptr(), None, Hi, Wi, S, S, C, stride[0], stride[1], 0, nw,
                  slide.BLENDS[blend], st)

    for _ in range(a.warmup):
        f_tta(), f_slide("uniform"), f_slide("pyramid")
    torch.cuda.synchronize()
    ts = {"tta": [], "uniform": [], "pyramid": []}
    for _ in range(a.reps):
        ts["tta"].append(_timed(f_tta))
        ts["uniform"].append(_timed(lambda: f_slide("uniform")))
        ts["pyramid"].append(_timed(lambda: f_slide("pyramid")))
    print("yardstick, alternating launches (%d each):" % a.reps)
    nb = {"tta": 4 * C * B * 3 * S * S, "uniform": 4 * C * (nw * S * S + 2 * _touched((Hi, Wi), window, stride, 0, nw))}
    nb["pyramid"] = nb["uniform"]
    rates = {}
    for k, label in (("tta", "dl3_tta_accumulate middle pass %d -> %d, B = %d" % (S, S, B)),
                     ("uniform", "dl3_slide_accumulate uniform, windows 0..%d" % (nw - 1)),
                     ("pyramid", "dl3_slide_accumulate pyramid, windows 0..%d" % (nw - 1))):
        ms = statistics.median(ts[k])
        _line(label, ms, min(ts[k]), max(ts[k]), nb[k])
        rates[k] = (nb[k] / ms / 1e9, nb[k] / max(ts[k]) / 1e9, nb[k] / min(ts[k]) / 1e9)
    spread = rates["tta"][2] - rates["tta"][1]
    print("  dl3_tta_accumulate: %.2f TB/s, run-to-run spread %.2f TB/s (%.2f - %.2f); dl3_slide_accumulate: uniform %.2f, "
          "pyramid %.2f TB/s" % (rates["tta"][0], spread, rates["tta"][1], rates["tta"][2], rates["uniform"][0],
                                 rates["pyramid"][0]))


def predict(a):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    S, C, B = a.window, a.classes, a.batch
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=(S, S, 3), classes=C, backbone="mobilenetv2")
    g = torch.Generator(device="cuda").manual_seed(0)
    Hi, Wi = 1024, 2048
    x = (255 * torch.rand(1, Hi, Wi, 3, device="cuda", generator=g)).to(torch.uint8)
    n = len(slide.grid((Hi, Wi), (S, S))[2])
    xw = (255 * torch.rand(n, S, S, 3, device="cuda", generator=g)).to(torch.uint8)

    def call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    for blend in ("uniform", "pyramid"):
        for name, fn in (("predict_sliding %s" % blend, lambda: model.predict_sliding(x, blend=blend, batch_size=B)),
                         ("predict_mask", lambda: model.predict_mask(xw, batch_size=B))):
            for _ in range(3):   # the engines capture their hipGraph on the second forward
                call(fn)
            ts = [call(fn) for _ in range(a.reps)]
            res[name] = statistics.median(ts)
            print("  %-28s median %8.2f ms (min %.2f, max %.2f) of %d calls" % (name, res[name], min(ts), max(ts), a.reps))
        print("  %s: %d x %d image = %d windows of %d x %d in batches of %d; overhead over predict_mask on %d windows: %.2f ms" % (
            blend, Hi, Wi, n, S, S, B, n, res["predict_sliding %s" % blend] - res["predict_mask"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "predict"])
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slide_profile: needs a GPU; nothing is measured without one")
    if a.reps is None:
        a.reps = 20 if a.mode == "kernels" else 5
    print("MobileNetV2 %d x %d x %d, images on the device, host wall clock around a synchronised call" % (
        a.window, a.window, a.classes) if a.mode == "predict" else "sliding-window kernels")
    {"kernels": kernels, "predict": predict}[a.mode](a)
