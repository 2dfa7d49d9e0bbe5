"""Cost of the dense CRF's softmax unary (dl3_crf_unary_*, csrc/crfunary.hip) and of the two predict_mask CRF paths.

  python tools/crf_softmax_profile.py kernels [--batch 16] [--size 512] [--classes 21] [--reps 20]
      each unary form at size x size x classes on resident buffers, launched --reps times; run under
      `rocprofv3 --kernel-trace --stats` for the per-kernel times.  Prints the event-timed mean and the algorithmic bytes.
  python tools/crf_softmax_profile.py predict [--images 2] [--size 512] [--classes 21] [--reps 3]
      Model.predict_mask(crf=True) with crf_unary="labels" and "softmax" on the same images (MobileNetV2, the `original`
      head), alternated --reps times; prints ms per image.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl3_amd  # noqa: E402,F401
from dl3_amd import capi  # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(a):
    B, S, C = a.batch, a.size, a.classes
    N = S * S
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    U = torch.empty(B, C, N, device="cuda")
    forms = []
    x = 4 * torch.randn(B, N, C, device="cuda", generator=g)
    forms.append(("plain (logits)", x.numel() * 4,
                  lambda: capi.call("dl3_crf_unary_plain", x.data_ptr(), 0, U.data_ptr(), B, N, C, 0.0, 1e-5, st)))
    p = torch.softmax(x, -1)
    forms.append(("plain (probabilities)", p.numel() * 4,
                  lambda: capi.call("dl3_crf_unary_plain", p.data_ptr(), 1, U.data_ptr(), B, N, C, 0.0, 1e-5, st)))
    lo = 4 * torch.randn(B, S // 16, S // 16, C, device="cuda", generator=g)
    forms.append(("bilinear %d -> %d" % (S // 16, S), lo.numel() * 4,
                  lambda: capi.call("dl3_crf_unary_bilinear", lo.data_ptr(), U.data_ptr(), B, S // 16, S // 16, S, S, C, 0.0,
                                    1e-5, st)))
    for r in (4, 8):
        u = 4 * torch.randn(B, S // r, S // r, C * r * r, device="cuda", generator=g)
        forms.append(("shuffle r = %d" % r, u.numel() * 4,
                      lambda u=u, r=r: capi.call("dl3_crf_unary_shuffle", u.data_ptr(), U.data_ptr(), B, S // r, S // r, C, r,
                                                 0.0, 1e-5, st)))
    wr = U.numel() * 4
    print("dl3_crf_unary_* at %d x %d x %d, B = %d: %d launches each after one warm-up" % (S, S, C, B, a.reps))
    for name, rd, fn in forms:
        ms = _timed(fn, a.reps)
        print("  %-24s %8.3f ms   reads %7.1f MB writes %7.1f MB   %.2f TB/s" % (name, ms, rd / 1e6, wr / 1e6,
                                                                                 (rd + wr) / ms / 1e9))


def predict(a):
    from dl3_amd import graph as G
    from dl3_amd.utils import SegModel
    from oracle import dl3_oracle as O
    S, C, n = a.size, a.classes, a.images
    G.clear_session()
    model = SegModel(image_size=(S, S)).create_seg_model("original", n=C, backbone="mobilenetv2")
    params = O.init_params(O.param_shapes("mobilenetv2", C, head="original"), seed=1)
    for l in model.layers:
        if l.weights:
            l.set_weights([params[k] for k in l.weights])
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:S, :S]
    x = np.stack([np.stack([128 + 100 * np.sin(xx / 70.0 + i) * np.cos(yy / 90.0), 128 + 100 * np.cos((xx + yy) / 110.0),
                            128 + 60 * np.sin(yy / 40.0) + 40 * np.sin(xx / 25.0)], -1) for i in range(n)])
    x = np.clip(np.rint(x + rng.integers(-2, 3, (n, S, S, 3))), 0, 255).astype(np.float32)
    plain = model.predict_mask(x, batch_size=n)
    print("predict_mask(crf=True) at %d x %d x %d, %d images per call, labels in the arg-max mask: %s" % (
        S, S, C, n, [len(np.unique(m)) for m in plain]))
    for mode in ("labels", "softmax"):
        model.predict_mask(x, batch_size=n, crf=True, crf_unary=mode)   # warm-up
    for rep in range(a.reps):
        for mode in ("labels", "softmax"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = model.predict_mask(x, batch_size=n, crf=True, crf_unary=mode)
            dt = time.perf_counter() - t
            print("  rep %d crf_unary=%-8s %8.1f ms per image   (%d pixels differ from the arg-max mask)" % (
                rep, mode, 1e3 * dt / n, int((m != plain).sum())))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "predict"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    (kernels if a.what == "kernels" else predict)(a)
