"""-m gpu tests of the N>1 path on a ONE-GPU box.

RCCL refuses two ranks on one device, so the two-process test moves the data plane onto gloo
(DL3_DIST_BACKEND=gloo: gradients staged through host memory); everything else — sharding, per-rank dropout
streams, the all-reduce + 1/world + Adam logic, Model.distribute()/train_on_batch — is the code the 8-GPU run uses.
The RCCL binding itself (include/dl3.h dl3_comm_*) is exercised as a world of one, and bench.py's self-spawn form
(`python bench.py --gpus 2`, the form the driver uses) end to end.
"""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import dl3_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, CLASSES, GLOBAL_B = (64, 64, 3), 3, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _data():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (GLOBAL_B,) + SHAPE).astype(np.float32)
    y = rng.integers(0, CLASSES + 1, (GLOBAL_B, SHAPE[0] * SHAPE[1], 1)).astype(np.float32)
    sw = ((y[:, :, 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2])).astype(np.float32)
    return x, y, sw


def _model(seed):
    import dl3_amd  # noqa: F401
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=SHAPE, classes=CLASSES, backbone="mobilenetv2", OS=16)
    params = O.init_params(O.param_shapes("mobilenetv2", CLASSES), seed=seed)
    for l in model.layers:
        if l.weights:
            l.set_weights([params[n] for n in l.weights])
    return model


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), DL3_DIST_BACKEND="gloo")
    torch.cuda.set_device(0)
    model = _model(seed=1 + rank)  # deliberately different initial weights: the first step must broadcast rank 0's
    model.compile(optimizer=dict(lr=7e-4))
    model.distribute()
    dp = model._dp
    assert dp.world == 2 and dp.backend == "gloo" and dp.comm is None
    x, y, sw = _data()
    losses = [model.train_on_batch(x, y, sw, use_graph=False) for _ in range(2)]
    eng = model._active
    assert eng.B == GLOBAL_B // world and eng.rank == rank
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), grads=eng.grads.cpu().numpy(), params=eng.params.cpu().numpy(),
             losses=np.array(losses), seed=np.array([eng.seed], np.uint64), tail=np.array([eng.tail]),
             c0=np.array([eng.nnz_host]))
    dp.close()


def test_two_engine_processes_allreduce_equals_mean_of_shards(tmp_path):
    """two Engine processes on one GPU: after train_on_batch on the global batch, every rank holds the same weights,
    and the gradient arena of the LAST step equals — bit for bit — the SUM of the two single-process shard arenas
    computed from the same weights (gradients of sum_shard(l*w) / c0, the shard's count(w != 0) and loss sum in the
    tail: round 5, one collective per step and no host round trip); the weights equal the single-process Adam step on
    that sum with the scale c0 / count_all finished on the device; a second run reproduces the same bits."""
    runs = []
    for rep in range(2):
        d = tmp_path / ("run%d" % rep)
        d.mkdir()
        mp.spawn(_worker, args=(2, _free_port(), str(d)), nprocs=2, join=True)
        runs.append([np.load(str(d / ("rank%d.npz" % r))) for r in (0, 1)])
    r0, r1 = runs[0]
    assert np.array_equal(r0["grads"], r1["grads"]) and np.array_equal(r0["params"], r1["params"])
    assert np.array_equal(r0["losses"], r1["losses"])  # the mean over ranks is what every rank reports
    assert int(r0["seed"][0]) != int(r1["seed"][0])    # per-rank dropout streams
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a["grads"], b["grads"]) and np.array_equal(a["params"], b["params"])
    # single-process replay of both shards: step 1 from rank 0's initial weights, then the same Adam update
    x, y, sw = _data()
    model = _model(seed=1)
    # external_nnz: ONE loss over the merged batch, like the reference's multi_gpu_model: every rank differentiates
    # sum_shard(l*w) / c0 (c0 fixed: pixels per image), count and loss sum ride in the arena tail
    engs = [model._engine(2, True, use_graph=False, rank=r, external_nnz=True) for r in (0, 1)]
    shard = lambda r: (x[2 * r:2 * r + 2], y[2 * r:2 * r + 2], sw[2 * r:2 * r + 2])
    nnz_all = float((sw != 0).sum())
    tail = int(r0["tail"][0])
    assert engs[0].tail == tail and engs[0].nnz_host == float(r0["c0"][0]) == float(SHAPE[0] * SHAPE[1])
    p0 = engs[1].params.clone()
    for step in range(2):
        g = []
        for r, e in enumerate(engs):
            e.params.copy_(p0)   # (BatchNorm runs on batch statistics: the per-replica moving statistics do not matter)
            xs, ys, ws = shard(r)
            e.set_input(xs)
            e.set_targets(ys, ws)
            assert e.count_nnz() == float((ws != 0).sum())
            e.fwd_bwd()
            torch.cuda.synchronize()
            g.append(e.grads.cpu().numpy().copy())
            assert g[-1][tail] == float((ws != 0).sum())    # the shard's count travels behind the gradients
        total = g[0] + g[1]
        if step == 1:
            assert np.array_equal(r0["grads"], total), "all-reduced arena != sum of the shard arenas"
            assert total[tail] == nnz_all
            # the loss every rank reported: sum_all(l*w) / count_all
            assert abs(float(r0["losses"][1]) - float(total[tail + 1]) * engs[0].nnz_host / nnz_all) < 1e-6 * abs(float(r0["losses"][1]))
        # the update every rank applied: Adam on the summed arena, scale c0 / count_all finished on the device
        e = engs[0]
        e.grads.copy_(torch.from_numpy(total).cuda())
        e.adam(dict(lr=7e-4), norm=True)
        p0 = e.params.clone()
    assert np.array_equal(r0["params"], p0.cpu().numpy())


def _ragged_data():
    """5 images over 2 ranks (2 + 3), very different void fractions per shard"""
    rng = np.random.default_rng(3)
    n = 5
    x = rng.integers(0, 256, (n,) + SHAPE).astype(np.float32)
    y = rng.integers(0, CLASSES, (n, SHAPE[0] * SHAPE[1], 1)).astype(np.float32)
    y[:2][rng.uniform(size=y[:2].shape) < 0.7] = CLASSES      # rank 0's shard: 70 % void
    y[2:][rng.uniform(size=y[2:].shape) < 0.1] = CLASSES      # rank 1's shard: 10 % void
    sw = ((y[:, :, 0] < CLASSES) * rng.uniform(0.5, 2.0, y.shape[:2])).astype(np.float32)
    return x, y, sw


def _worker_global_loss(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), DL3_DIST_BACKEND="gloo")
    torch.cuda.set_device(0)
    model = _model(seed=1)
    model.compile(optimizer=dict(lr=7e-4))
    model.distribute()
    x, y, sw = _ragged_data()
    loss = model.train_on_batch(x, y, sw, use_graph=False, bn_mode="frozen", dropout=False)
    eng = model._active
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "g%d.npz" % rank), grads=eng.grads.cpu().numpy(), loss=np.array([loss]), B=np.array([eng.B]),
             tail=np.array([eng.tail]), c0=np.array([eng.nnz_host]))
    model._dp.close()


def test_data_parallel_loss_is_the_global_batch_loss(tmp_path):
    """the reference's multi_gpu_model merges the towers and evaluates ONE loss, sum(l*w) / count_all(w != 0);
    with unequal void fractions per shard a per-rank normalisation gives a different gradient.  With frozen BatchNorm
    (no per-replica batch statistics) the 2-rank step on a RAGGED global batch (5 = 2 + 3 images) must equal the
    single-process step on the same 5 images: loss and all-reduced gradient (up to fp32 summation order)."""
    mp.spawn(_worker_global_loss, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = [np.load(str(tmp_path / ("g%d.npz" % r))) for r in (0, 1)]
    assert (int(r0["B"][0]), int(r1["B"][0])) == (2, 3)
    assert np.array_equal(r0["grads"], r1["grads"]) and r0["loss"][0] == r1["loss"][0]
    x, y, sw = _ragged_data()
    model = _model(seed=1)
    eng = model._engine(5, True, use_graph=False, bn_mode="frozen", dropout=False)
    eng.set_input(x)
    eng.set_targets(y, sw)
    eng.fwd_bwd()
    torch.cuda.synchronize()
    tail = int(r0["tail"][0])
    want = eng.grads.cpu().numpy()[:eng.n_param]
    assert r0["grads"][tail] == float((sw != 0).sum())                   # count_all, summed by the one all-reduce
    got = r0["grads"][:eng.n_param] * np.float32(float(r0["c0"][0]) / r0["grads"][tail])   # what Adam applies: c0 / count_all
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("2-rank ragged step vs single process: loss %.7f vs %.7f, gradient rel-L2 %.2e" % (
        float(r0["loss"][0]), float(eng.loss[0].item()), err))
    assert abs(float(r0["loss"][0]) - float(eng.loss[0].item())) < 1e-5 * abs(float(eng.loss[0].item()))
    assert err < 1e-4
    # and it is NOT what per-rank normalisation would give: shard losses weighted by their own counts differ
    n0, n1 = float((sw[:2] != 0).sum()), float((sw[2:] != 0).sum())
    assert abs(n0 - n1) > 0.3 * (n0 + n1) / 2


def test_rccl_binding_world_of_one():
    """include/dl3.h dl3_comm_*: librccl is found (dlopen), a communicator comes up on cuda:0 and the collectives run on
    the caller's stream (a world of one: all-reduce and broadcast are identities)."""
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    L = capi.lib()
    raw = ctypes.create_string_buffer(128)
    capi.check(L.dl3_comm_unique_id(raw), "dl3_comm_unique_id")
    assert any(raw.raw)
    h = ctypes.c_void_p()
    capi.check(L.dl3_comm_init(ctypes.byref(h), raw.raw, 0, 1), "dl3_comm_init")
    assert h.value
    rng = np.random.default_rng(0)
    a = rng.normal(0, 1, 2113557).astype(np.float32)  # the MobileNetV2 gradient arena
    t = torch.from_numpy(a).cuda()
    out = torch.zeros_like(t)
    st = torch.cuda.current_stream().cuda_stream
    capi.call("dl3_comm_allreduce_f32", h, t.data_ptr(), out.data_ptr(), t.numel(), st)
    capi.call("dl3_comm_allreduce_f32", h, t.data_ptr(), t.data_ptr(), t.numel(), st)  # in place, as the step does
    capi.call("dl3_comm_broadcast_f32", h, t.data_ptr(), t.numel(), 0, st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), a) and np.array_equal(t.cpu().numpy(), a)
    assert L.dl3_comm_init(ctypes.byref(ctypes.c_void_p()), raw.raw, 3, 2) != 0  # rank outside the world: refused
    capi.check(L.dl3_comm_destroy(h), "dl3_comm_destroy")


def test_bench_self_spawns_its_ranks():
    """`python bench.py --gpus 2` without a launcher (the driver's form) re-executes itself under torch.distributed.run
    and prints ONE JSON line with n_gpus = 2 and the whole-job rate; here two ranks share the GPU over gloo."""
    env = dict(os.environ, DL3_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--batch", "2",
           "--size", "128", "--full", "--no-cpu-baseline", "--no-roofline"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["config"]["global_batch"] == 4
    assert rec["config"]["hipgraph"] is True and rec["config"]["parallelism"] == "dp2"
    # round 3: the line says which data plane produced it and what the exchange costs on its own
    assert rec["config"]["gradient_exchange"] == "gloo (host staged)" and rec["config"]["rccl_ranks"] is None
    assert rec["allreduce_ms"] > 0 and rec["config"]["dist_strict"] is False
    assert abs(rec["value"] - 4 * 3 / (rec["ms_per_step"] * 3e-3)) < 1e-6 * rec["value"]
    # round 6: the N > 1 line carries the fed leg too — every rank feeds its own shard into the data-parallel step
    assert rec["fed"]["value"] > 0 and rec["fed"]["steps"] == 3 and np.isfinite(rec["fed"]["final_loss"])
    assert abs(rec["fed"]["value"] - 4 * 3 / (rec["fed"]["ms_per_step"] * 3e-3)) < 1e-6 * rec["fed"]["value"]
    # a launcher environment that disagrees with --gpus is refused, not silently reinterpreted
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    res = subprocess.run(cmd, env=env2, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "WORLD_SIZE" in res.stderr


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `python bench.py --gpus 1 --steps K --warmup W` times the headline only (the side measurements run with
    --full), and --dump-outputs writes what the last timed step left: loss, weights after Adam, gradients, BatchNorm state —
    float, finite, under 64 MB, and the same on a second run with the same arguments (seeded inputs and weights)."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    full_only = ("fed", "allreduce_ms", "insitu_step_ms", "roofline", "roofline_hbm", "split_math", "by_batch", "configs",
                 "cpu_baseline")
    dumps = []
    for run in range(2):
        d = str(tmp_path / ("run%d" % run))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
               "--size", "128", "--dump-outputs", d]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, res.stdout
        rec = json.loads(lines[0])
        assert rec["steps"] == 3 and rec["unit"] == "img/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert abs(rec["value"] - 2 * 3 / (rec["ms_per_step"] * 3e-3)) < 1e-6 * rec["value"]
        assert [k for k in full_only if k in rec] == []
        files = sorted(os.listdir(d))
        assert files == ["grads.npy", "loss.npy", "params.npy", "state.npy"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
        out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
        assert out["loss"][0] == rec["config"]["final_loss"] and np.abs(out["grads"]).max() > 0
        dumps.append(out)
    for k, a in dumps[0].items():
        b = dumps[1][k]
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-6 * np.abs(a).max(), k


def test_data_parallel_step_with_a_one_rank_rccl_communicator_under_hipgraph():
    """the N-GPU train_on_batch launch for launch on ONE GPU — Model.distribute() with an RCCL
    communicator of one rank: device count of the sample weights, a one-float ncclAllReduce and a scale IN FRONT of the
    captured backward hipGraph, the gradient arena's ncclAllReduce BEHIND its replay, Adam with 1/world — on one stream,
    eager (step 1), capturing (step 2) and replaying (steps 3-4).  Round 5: nothing is left in front of the graph — the
    shard's count(w != 0) and loss sum ride in the arena's tail through the ONE all-reduce, the loss kernel divides by a
    fixed c0 and Adam multiplies by c0 / count_all on the device.  A sum over one rank is the identity; the scaling
    point moved, so weights and losses equal the plain single-process run to fp32 rounding instead of bit for bit."""
    import dl3_amd  # noqa: F401
    from dl3_amd.parallel import DataParallel
    from oracle import dl3_oracle as O
    from tests.test_gpu_model import _build, _load
    assert int(os.environ.get("WORLD_SIZE", "1")) == 1
    shape, classes, B = (96, 96, 3), 4, 3
    rng = np.random.default_rng(3)
    batches = []
    for _ in range(4):
        x = rng.integers(0, 256, (B,) + shape).astype(np.float32)
        y = rng.integers(0, classes + 1, (B, shape[0] * shape[1], 1)).astype(np.float32)
        sw = ((y[..., 0] < classes) * rng.uniform(0.5, 2.0, y.shape[:2])).astype(np.float32)
        batches.append((x, y, sw))

    def run(mode):
        """mode 'plain': the single-process engine; 'tail': the data-parallel engine (external_nnz) without a communicator;
        'rccl': Model.distribute() with a one-rank RCCL communicator"""
        model, params = _build("mobilenetv2", shape, classes, "deeplab")
        _load(model, params)
        dp = None
        kw = dict(dropout=False)
        if mode == "rccl":
            dp = DataParallel().attach_single_rank_rccl()
            assert dp.rccl_ranks() == 1
            model.distribute(dp)
        elif mode == "tail":
            kw["external_nnz"] = True
        losses, g1 = [], None
        for x, y, sw in batches:
            losses.append(model.train_on_batch(x, y, sw, **kw))
            if g1 is None:
                e = model._active
                g1 = e.grads.cpu().numpy().copy()
                if e.external_nnz:   # what Adam applied: arena x c0 / count_all
                    g1 = g1[:e.n_param] * np.float32(e.nnz_host / g1[e.tail])
                else:
                    g1 = g1[:e.n_param]
        eng = model._active
        assert eng.graph is not None, "the step was never captured"
        assert eng.external_nnz == (mode != "plain")
        torch.cuda.synchronize()
        w = eng.params.cpu().numpy().copy()
        st = eng.state.cpu().numpy().copy()
        if dp is not None:
            dp.close()
        return losses, w, st, g1

    la, wa, sa, ga = run("plain")
    lt, wt, st_, gt = run("tail")
    lb, wb, sb, gb = run("rccl")
    # the communicator and the captured all-reduce change NOTHING: a sum over one rank is the identity
    assert lt == lb and np.array_equal(wt, wb) and np.array_equal(st_, sb) and np.array_equal(gt, gb)
    # against the plain engine the scaling point moved (loss kernel / c0, Adam x c0 / count_all): first-step loss and
    # gradient agree to fp32 rounding.  (Later steps part like any two fp32 evaluations do under Adam: an element whose
    # gradient is below rounding noise moves by +-lr at random, DESIGN.md §4 — which is why rounds 1-4 could only assert
    # this test bit for bit, and why that is no longer possible.)
    err = float(np.linalg.norm(gb - ga) / np.linalg.norm(ga))
    print("one-rank RCCL step vs plain step: first-step loss %.9f / %.9f, gradient rel-L2 %.2e; losses %s / %s" % (
        la[0], lb[0], err, la, lb))
    assert abs(la[0] - lb[0]) < 2e-6 * abs(la[0]) and err < 1e-5
    # (three Adam steps later the two runs are two fp32 trajectories: 6.5e-3 apart on the driver box of round 5's collection)
    assert all(abs(a - b) < 3e-2 * abs(a) for a, b in zip(la, lb))
    assert len(set(la)) == 4

def test_data_parallel_step_has_no_host_round_trip():
    """the data-parallel step — captured forward/backward, ONE RCCL all-reduce of the arena (gradients +
    the shard's count(w != 0) + loss sum), Adam with the normalisation finished on the device, the loss handed back as a
    LazyLoss — under torch.cuda.set_sync_debug_mode("error"): any implicit host synchronisation raises.  (A world of one:
    what a one-GPU box can run of it.)"""
    import dl3_amd  # noqa: F401
    from dl3_amd.parallel import DataParallel
    from tests.test_gpu_model import _build, _load
    shape, classes, B = (64, 64, 3), 3, 2
    model, params = _build("mobilenetv2", shape, classes, "deeplab")
    _load(model, params)
    dp = DataParallel().attach_single_rank_rccl()
    eng = model._engine(B, True, dropout=False, external_nnz=True)
    rng = np.random.default_rng(9)
    x = rng.integers(0, 256, (B,) + shape).astype(np.float32)
    y = rng.integers(0, classes + 1, (B, shape[0] * shape[1])).astype(np.float32)
    sw = ((y < classes) * rng.uniform(0.5, 2.0, y.shape)).astype(np.float32)
    eng.set_input(x)
    eng.set_targets(y, sw)
    for _ in range(2):          # eager, then capture
        eng.fwd_bwd()
        dp.allreduce_grads(eng.grads)
        eng.adam(None, norm=True)
    torch.cuda.synchronize()
    assert eng.graph is not None
    handles = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            eng.fwd_bwd()
            dp.allreduce_grads(eng.grads)
            eng.adam(None, norm=True)
            handles.append(eng.loss_handle())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    vals = [float(h) for h in handles]
    assert all(np.isfinite(v) for v in vals) and len(set(vals)) == 3
    assert abs(vals[-1] - eng.loss_value()) < 1e-7 * abs(vals[-1])
    assert float(eng.grads[eng.tail].item()) == float((sw != 0).sum())
    dp.close()


# ---- round 6: fed batches under data parallelism -------------------------------------------------------
def _byte_batches(steps, B, shape, classes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        img = rng.integers(0, 256, (B,) + shape, dtype=np.uint8)
        lab = rng.integers(0, classes, (B, shape[0], shape[1]), dtype=np.uint8)
        lab[rng.uniform(size=lab.shape) < 0.1] = 255
        out.append((img, lab))
    return out


def test_device_feed_under_distribute_equals_train_on_batch_one_rank_rccl():
    """Model.fit_generator(device_feed=True) under Model.distribute() (utils.py:209-211 + :231-241): the fed loop — bytes
    over a copy stream, targets on the device, captured step, ONE arena all-reduce, Adam finishing the scale on the device —
    lands on the same weights, bit for bit, as train_on_batch on the host-side (X, Y, SW) of the same batches (a
    communicator of one rank: what a one-GPU box can run)."""
    import dl3_amd  # noqa: F401
    from dl3_amd.parallel import DataParallel
    from dl3_amd import utils as U
    from tests.test_gpu_model import _build, _load
    shape, classes, B, steps = (64, 64, 3), 3, 2, 4
    batches = _byte_batches(steps, B, shape, classes, 21)

    def run(fed):
        model, params = _build("mobilenetv2", shape, classes, "deeplab")
        _load(model, params)
        model.compile(optimizer=dict(lr=7e-4))
        dp = DataParallel().attach_single_rank_rccl()
        model.distribute(dp)
        if fed:
            losses = model.fit_generator(batches, steps_per_epoch=steps, device_feed=True, n_classes=classes)
        else:
            losses = []
            for img, lab in batches:
                y, sw = U.prepare_targets(lab, classes)
                losses.append(float(model.train_on_batch(img, y, sw)))
        eng = model._active
        assert eng.external_nnz and eng.graph is not None
        torch.cuda.synchronize()
        w = eng.params.cpu().numpy().copy()
        dp.close()
        return losses, w

    lf, wf = run(True)
    lh, wh = run(False)
    print("fed under distribute(): losses %s / host arrays %s" % (lf, lh))
    assert np.array_equal(wf, wh) and lf == lh


def _worker_fed(rank, world, port, out_dir, global_batch):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), DL3_DIST_BACKEND="gloo")
    torch.cuda.set_device(0)
    model = _model(seed=1 + rank)
    model.compile(optimizer=dict(lr=7e-4))
    model.distribute()
    steps = 3
    batches = _byte_batches(steps, GLOBAL_B, SHAPE, CLASSES, 33)
    if not global_batch:   # a generator sharded by rank: it yields this rank's rows only
        lo, hi = model._dp.shard(GLOBAL_B)
        batches = [(i[lo:hi], l[lo:hi]) for i, l in batches]
    losses = model.fit_generator(batches, steps_per_epoch=steps, device_feed=True, n_classes=CLASSES,
                                 global_batch=global_batch)
    eng = model._active
    assert eng.B == GLOBAL_B // world and eng.external_nnz
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "fed%d_%d.npz" % (int(global_batch), rank)), params=eng.params.cpu().numpy(),
             losses=np.array(losses))
    model._dp.close()


def _worker_fed_reference(rank, world, port, out_dir):
    """the same three steps through train_on_batch on host arrays of the GLOBAL batch (the path round 5 tested)"""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), DL3_DIST_BACKEND="gloo")
    torch.cuda.set_device(0)
    from dl3_amd import utils as U
    model = _model(seed=1 + rank)
    model.compile(optimizer=dict(lr=7e-4))
    model.distribute()
    losses = []
    for img, lab in _byte_batches(3, GLOBAL_B, SHAPE, CLASSES, 33):
        y, sw = U.prepare_targets(lab, CLASSES)
        losses.append(float(model.train_on_batch(img, y, sw)))
    eng = model._active
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "ref%d.npz" % rank), params=eng.params.cpu().numpy(), losses=np.array(losses))
    model._dp.close()


def test_device_feed_under_distribute_two_processes(tmp_path):
    """two ranks on one GPU (gloo data plane): fit_generator(device_feed=True) under distribute() with the generator
    yielding the GLOBAL batch (each rank stages its shard only) and with a generator already sharded by rank
    (global_batch=False) — both end on the weights of train_on_batch on the global batch, identical on the two ranks, and
    report the same global loss."""
    d = str(tmp_path)
    mp.spawn(_worker_fed_reference, args=(2, _free_port(), d), nprocs=2, join=True)
    for gb in (True, False):
        mp.spawn(_worker_fed, args=(2, _free_port(), d, gb), nprocs=2, join=True)
    ref = [np.load(os.path.join(d, "ref%d.npz" % r)) for r in (0, 1)]
    assert np.array_equal(ref[0]["params"], ref[1]["params"])
    for gb in (1, 0):
        fed = [np.load(os.path.join(d, "fed%d_%d.npz" % (gb, r))) for r in (0, 1)]
        assert np.array_equal(fed[0]["params"], fed[1]["params"]) and np.array_equal(fed[0]["losses"], fed[1]["losses"])
        assert np.array_equal(fed[0]["params"], ref[0]["params"]), "fed shards != train_on_batch on the global batch"
        assert np.array_equal(fed[0]["losses"], ref[0]["losses"])
