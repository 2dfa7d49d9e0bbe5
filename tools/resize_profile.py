"""Cost of the device cv2.resize front end (dl3_cv_resize, csrc/cvresize.hip) over VOC-like sources.

  python tools/resize_profile.py kernels [--batch 128] [--size 512] [--reps 20]
      B sources, 375x500 and 500x375 alternating, resized to size x size on resident pools: blur off, then blur on for
      every image; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times.  Prints one JSON line per case
      with the event-timed mean and the algorithmic bytes per batch.
  python tools/resize_profile.py step [--batch 128] [--size 512] [--steps 30] [--repeats 3]
      the fed training step (feed.BatchFeeder, MobileNetV2 DeepLabV3+, dropout on) with the notebook's training
      augmentation over pre-resized size x size arrays and over the ragged sources (device_resize), alternated --repeats
      times on one engine; prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl3_amd  # noqa: E402,F401
from dl3_amd import augment as A  # noqa: E402

NB_TRAIN = dict(blur=5, horizontal_flip=True, brightness=0.3, zoom=0.1, rotation=5.0, do_ahisteq=True)
VOC = ((375, 500), (500, 375))


def algorithmic_bytes(src_px, dst_px, blur):
    """(minimum, with intermediates) bytes per batch: the sources are read once (3 + 1 B/px) and the uniform batch written
    once (3 + 1 B/px); the intermediates add the label-set pass (read 1 B/px of the source) and, with blur, the blurred
    copy of the pool (write 3, read 3 B/px of the source)"""
    lo = 4 * src_px + 4 * dst_px
    return lo, lo + src_px + (6 * src_px if blur else 0)


def kernels(a):
    B, H, W = a.batch, a.size, a.size
    rng = np.random.default_rng(0)
    sizes = [VOC[n % 2] for n in range(B)]
    src_px = sum(h * w for h, w in sizes)
    ipool = torch.from_numpy(rng.integers(0, 256, 3 * src_px, dtype=np.uint8)).cuda()
    lpool = torch.from_numpy(rng.integers(0, 21, src_px, dtype=np.uint8)).cuda()
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    lout = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    present = torch.empty(B, 8, dtype=torch.int32, device="cuda")
    for blur in (0, 1):
        t0 = time.perf_counter()
        tab, offs, info = A.front_tables(sizes, (H, W), blur=[blur] * B)
        host_ms = 1e3 * (time.perf_counter() - t0)
        dtab = torch.from_numpy(tab).cuda()
        ws = torch.empty(A.front_workspace_bytes(info), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            A.launch_front(info, dtab, offs, ipool, lpool, out, lout, present, ws)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            A.launch_front(info, dtab, offs, ipool, lpool, out, lout, present, ws)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        lo, hi = algorithmic_bytes(src_px, B * H * W, blur)
        print(json.dumps({"what": "dl3_cv_resize, blur %s" % ("on" if blur else "off"), "batch": B, "size": H,
                          "sources": "375x500 / 500x375 alternating", "ms_per_batch": ms, "bytes_min": lo,
                          "bytes_with_intermediates": hi, "gb_s_min": lo / ms / 1e6,
                          "gb_s_with_intermediates": hi / ms / 1e6, "output_bytes": 4 * B * H * W,
                          "us_per_output_mb": 1e3 * ms / (4 * B * H * W / 1e6), "front_tables_host_ms": host_ms,
                          "table_ints": int(tab.size), "workspace_bytes": ws.numel()}), flush=True)


def step(a):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    from dl3_amd.feed import BatchFeeder
    B, H, W = a.batch, a.size, a.size
    G.clear_session(seed=1)
    model = Deeplabv3(weights=None, input_shape=(H, W, 3), classes=21, backbone="mobilenetv2", OS=16)
    eng = model._engine(B, True, dropout=True)
    rng = np.random.default_rng(77)
    sizes = [VOC[n % 2] for n in range(B)]
    uniform, ragged = [], []
    for _ in range(3):
        img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).pin_memory()
        lab = rng.integers(0, 22, (B, H, W), dtype=np.uint8)
        lab[lab == 21] = 255
        uniform.append((img, torch.from_numpy(lab).pin_memory()))
        imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes]
        labs = [rng.integers(0, 21, hw, dtype=np.uint8) for hw in sizes]
        ragged.append((imgs, labs))
    plan = A.Plan((H, W), **NB_TRAIN)
    rplan = A.Plan(None, resize_shape=(W, H), device_resize=True, **NB_TRAIN)
    fixed = BatchFeeder(eng, 21, np.uint8, plan=plan)
    any_size = BatchFeeder(eng, 21, np.uint8, plan=rplan, pool_px=sum(h * w for h, w in sizes))
    r = random.Random(7)

    def batches(n, rag):
        for i in range(n):
            if rag:
                imgs, labs = ragged[i % 3]
                yield imgs, labs, [rplan.draw(r, hw) for hw in sizes]
            else:
                img, lab = uniform[i % 3]
                yield img, lab, [plan.draw(r) for _ in range(B)]

    def stepf():
        eng.fwd_bwd()
        eng.adam(None, 1.0)

    def timed(fd, rag, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fd.run(batches(n, rag), stepf)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    # the host half of a ragged batch on its own: draws + tables, and packing the pools into pinned memory
    t0 = time.perf_counter()
    for _ in range(5):
        A.batch_tables(rplan, sizes, [rplan.draw(r, hw) for hw in sizes])
    tables_ms = 1e3 * (time.perf_counter() - t0) / 5
    t0 = time.perf_counter()
    for _ in range(5):
        A.pack_pools(ragged[0][0], ragged[0][1], any_size.hx[0].numpy(), any_size.hl[0].numpy())
    pack_ms = 1e3 * (time.perf_counter() - t0) / 5
    timed(fixed, False, 3)
    timed(any_size, True, 3)
    res = {"pre_resized": [], "ragged": []}
    for _ in range(a.repeats):
        res["pre_resized"].append(timed(fixed, False, a.steps))
        res["ragged"].append(timed(any_size, True, a.steps))
    mp, mr = float(np.median(res["pre_resized"])), float(np.median(res["ragged"]))
    print(json.dumps({"what": "fed training step, notebook train augmentation: pre-resized arrays vs ragged sources",
                      "batch": B, "size": H, "steps_per_repeat": a.steps, "ms_per_step": res, "median_pre_resized": mp,
                      "median_ragged": mr, "img_s_pre_resized": 1e3 * B / mp, "img_s_ragged": 1e3 * B / mr,
                      "ratio_ragged_over_pre_resized": mr / mp, "host_draws_and_tables_ms_per_batch": tables_ms,
                      "host_pack_pools_ms_per_batch": pack_ms, "final_loss": eng.loss_value()}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernels", "step"])
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--size", type=int, default=512)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--repeats", type=int, default=3)
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    (kernels if a.mode == "kernels" else step)(a)


if __name__ == "__main__":
    main()
