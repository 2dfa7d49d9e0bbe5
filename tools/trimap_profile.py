"""Cost of the trimap evaluation (csrc/trimap.hip, trimap.py).

  python tools/trimap_profile.py kernels [--size 512] [--classes 21] [--batch 16] [--reps 32] [--warmup 3]
      dl3_trimap_rings (both metrics) and dl3_trimap_confusion on resident buffers, widths (1, 2, 4, 8, 16, 32): one
      device-event pair per call, the median of --reps calls after --warmup, beside the algorithmic bytes.  Run it under
      `rocprofv3 --kernel-trace --stats` (in a run of its own) for the per-kernel times: dl3_trimap_rings is two kernels.
      Labels: the arg-max of box-smoothed noise with about 1 % void, generated on the device; predictions: the labels
      shifted by (2, 3) pixels.
  python tools/trimap_profile.py model [--size 512] [--classes 21] [--batch 16] [--images 64] [--reps 3] [--root DIR]
      wall clock of Model.confusion_matrix and (where the checkout has it) Model.confusion_matrix_trimap over --images host
      images, MobileNetV2, best of --reps behind a device synchronisation, the two alternating.  --root: time another
      checkout of the package (one without the trimap pass reports confusion_matrix alone).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

WIDTHS = (1, 2, 4, 8, 16, 32)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _labels(B, S, C, void=0.01):
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(B, C, S, S, device="cuda", generator=g)
    for _ in range(4):
        z = torch.nn.functional.avg_pool2d(z, 9, stride=1, padding=4)
    lab = z.argmax(1).to(torch.float32)
    lab[torch.rand(B, S, S, device="cuda", generator=g) < void] = float(C)
    return lab.contiguous()


def kernels(a):
    import ctypes
    from dl3_amd import capi
    B, S, C = a.batch, a.size, a.classes
    n = B * S * S
    st = torch.cuda.current_stream().cuda_stream
    lab = _labels(B, S, C)
    pred = torch.roll(lab, (2, 3), (1, 2)).clamp(max=C - 1).to(torch.int32).contiguous()
    ring = torch.empty(n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(capi.lib().dl3_trimap_workspace_bytes(B, S, S), dtype=torch.uint8, device="cuda")
    band = torch.zeros(len(WIDTHS) + 1, C, C, dtype=torch.int64, device="cuda")
    cw = (ctypes.c_int * len(WIDTHS))(*WIDTHS)
    wmax = WIDTHS[-1]
    rows = 2 * wmax + 4   # source rows a lane of the column pass reads for its 4 output rows

    def f_rings(metric):
        capi.call("dl3_trimap_rings", lab.data_ptr(), ring.data_ptr(), ws.data_ptr(), B, S, S, C, wmax, metric, 3, st)

    def f_conf():
        capi.call("dl3_trimap_confusion", pred.data_ptr(), lab.data_ptr(), ring.data_ptr(), band.data_ptr(), B, S, S, C, cw,
                  len(WIDTHS), st)
    calls = (("dl3_trimap_rings chebyshev", lambda: f_rings(0), n * (4 + 1 + rows / 4 + 1)),
             ("dl3_trimap_rings euclidean", lambda: f_rings(1), n * (4 + 1 + rows / 4 + 1)),
             ("dl3_trimap_confusion", f_conf, n * (4 + 4 + 1)))
    for _ in range(a.warmup):
        for _, fn, _ in calls:
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _, _ in calls}
    for _ in range(a.reps):
        for name, fn, _ in calls:
            ts[name].append(_timed(fn))
    seeds = float((ring == 0).float().mean())
    print("B = %d, %d x %d, C = %d, widths %s; %.1f %% of the pixels are seeds; median (min - max) of %d calls, device events"
          % (B, S, S, C, WIDTHS, 100 * seeds, a.reps))
    print("algorithmic bytes a pixel: rings 4 (label) + 1 (row distance written) + %.1f (%d rows read for 4 output rows) + 1; "
          "confusion 4 + 4 + 1" % (rows / 4, rows))
    for name, _, nbytes in calls:
        ms = statistics.median(ts[name])
        print("  %-28s %8.1f us (%6.1f - %6.1f)  %7.1f MB  %6.3f TB/s" % (name, ms * 1e3, min(ts[name]) * 1e3,
                                                                          max(ts[name]) * 1e3, nbytes / 1e6, nbytes / ms / 1e9))


def model(a):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    S, C, B, N = a.size, a.classes, a.batch, a.images
    G.clear_session()
    m = Deeplabv3(weights=None, input_shape=(S, S, 3), classes=C, backbone="mobilenetv2")
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (N, S, S, 3)).astype(np.float32)
    y = _labels(N, S, C).cpu().numpy().reshape(N, S * S, 1)

    def call(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    fns = [("confusion_matrix", lambda: m.confusion_matrix(x, y, batch_size=B))]
    if hasattr(m, "confusion_matrix_trimap"):
        for metric in ("chebyshev", "euclidean"):
            fns.append(("confusion_matrix_trimap %s" % metric,
                        lambda metric=metric: m.confusion_matrix_trimap(x, y, batch_size=B, widths=WIDTHS, metric=metric)))
    for _ in range(3):   # the engines capture their hipGraph on the second call
        for _, fn in fns:
            call(fn)
    ts = {name: [] for name, _ in fns}
    for _ in range(a.reps):
        for name, fn in fns:
            ts[name].append(call(fn))
    print("MobileNetV2 %d x %d x %d, %d host images in batches of %d, host wall clock around a synchronised call, best of %d"
          % (S, S, C, N, B, a.reps))
    for name, _ in fns:
        print("  %-36s best %8.2f ms (median %.2f, max %.2f)" % (name, min(ts[name]), statistics.median(ts[name]),
                                                                max(ts[name])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "model"])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trimap_profile: needs a GPU; nothing is measured without one")
    sys.path.insert(0, os.path.abspath(a.root))
    import dl3_amd  # noqa: E402,F401
    if a.reps is None:
        a.reps = 32 if a.mode == "kernels" else 3
    {"kernels": kernels, "model": model}[a.mode](a)
