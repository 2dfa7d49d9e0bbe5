"""Cost of the device-side training augmentation (dl3_augment, csrc/augment.hip).

  python tools/augment_profile.py kernels [--batch 128] [--size 512] [--reps 20]
      all flags on (blur 5, both flips, brightness, rotation, zoom, CLAHE), launched --reps times on resident buffers;
      run under `rocprofv3 --kernel-trace --stats` for the per-kernel times.  Prints the launch's event-timed mean and
      the algorithmic bytes per batch.
  python tools/augment_profile.py step [--batch 128] [--size 512] [--steps 30] [--repeats 3]
      the fed training step (feed.BatchFeeder, MobileNetV2 DeepLabV3+, dropout on) without augmentation and with the
      notebook's training augmentation, alternated --repeats times on one engine; prints one JSON line.
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

ALL = dict(blur=5, horizontal_flip=True, vertical_flip=True, brightness=0.3, rotation=5.0, zoom=0.1, do_ahisteq=True)
NB_TRAIN = dict(blur=5, horizontal_flip=True, brightness=0.3, zoom=0.1, rotation=5.0, do_ahisteq=True)


def algorithmic_bytes(B, H, W):
    """(minimum, with intermediates) bytes per batch at all flags on, no crop: the source is read once (3 + 1 B/px) and
    X (12 B/px) + the label map (1 B/px) written once; the intermediates add stage 1's uint8 image + label (write 4, read
    4), the present-label pass (read 1) and the YUV image (write 3, read 3)"""
    px = B * H * W
    return px * (4 + 13), px * (4 + 13 + 4 + 4 + 1 + 3 + 3)


def kernels(a):
    B, H, W = a.batch, a.size, a.size
    plan = A.Plan((H, W), **ALL)
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    labs = torch.from_numpy(rng.integers(0, 21, (B, H, W), dtype=np.uint8)).cuda()
    r = random.Random(1)
    tab, offs = A.tables(plan, [plan.draw(r) for _ in range(B)])
    tab = torch.from_numpy(tab).cuda()
    X = torch.empty(B, H, W, 3, device="cuda")
    L = torch.empty(B, H * W, dtype=torch.uint8, device="cuda")
    ws = torch.empty(A.workspace_bytes(plan, B), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        A.launch(plan, tab, offs, imgs, labs, 21, X, L, ws)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        A.launch(plan, tab, offs, imgs, labs, 21, X, L, ws)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    lo, hi = algorithmic_bytes(B, H, W)
    print(json.dumps({"what": "dl3_augment all flags", "batch": B, "size": H, "ms_per_batch": ms,
                      "bytes_min": lo, "bytes_with_intermediates": hi, "gb_s_min": lo / ms / 1e6,
                      "gb_s_with_intermediates": hi / ms / 1e6, "workspace_bytes": ws.numel()}))


def step(a):
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    from dl3_amd.feed import BatchFeeder
    B, H, W = a.batch, a.size, a.size
    G.clear_session(seed=1)
    model = Deeplabv3(weights=None, input_shape=(H, W, 3), classes=21, backbone="mobilenetv2", OS=16)
    eng = model._engine(B, True, dropout=True)
    rng = np.random.default_rng(77)
    host = []
    for _ in range(3):
        img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).pin_memory()
        lab = rng.integers(0, 22, (B, H, W), dtype=np.uint8)
        lab[lab == 21] = 255
        host.append((img, torch.from_numpy(lab).pin_memory()))
    plan = A.Plan((H, W), **NB_TRAIN)
    plain = BatchFeeder(eng, 21, np.uint8)
    aug = BatchFeeder(eng, 21, np.uint8, plan=plan)
    r = random.Random(7)

    def batches(n, with_params):
        for i in range(n):
            img, lab = host[i % 3]
            yield (img, lab, [plan.draw(r) for _ in range(B)]) if with_params else (img, lab)

    def stepf():
        eng.fwd_bwd()
        eng.adam(None, 1.0)

    def timed(fd, with_params, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fd.run(batches(n, with_params), stepf)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    # the host half on its own: the draws + augment.tables of one batch (what stage() adds per step)
    t0 = time.perf_counter()
    for _ in range(10):
        A.tables(plan, [plan.draw(r) for _ in range(B)])
    host_ms = 1e3 * (time.perf_counter() - t0) / 10
    timed(plain, False, 3)
    timed(aug, True, 3)
    res = {"plain": [], "augmented": []}
    for _ in range(a.repeats):
        res["plain"].append(timed(plain, False, a.steps))
        res["augmented"].append(timed(aug, True, a.steps))
    mp, ma = float(np.median(res["plain"])), float(np.median(res["augmented"]))
    print(json.dumps({"what": "fed training step, notebook train augmentation vs none", "batch": B, "size": H,
                      "steps_per_repeat": a.steps, "ms_per_step": res, "median_plain": mp, "median_augmented": ma,
                      "slowdown_pct": 100 * (ma / mp - 1), "host_draws_and_tables_ms_per_batch": host_ms,
                      "final_loss": eng.loss_value()}))


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
