"""Executor: lowers a graph.Model into a static plan of libdl3.so launches (forward, loss, backward,
Adam) over HBM-resident buffers, and replays it — eagerly or as one captured hipGraph.

Design (MI355X-first):
  * one process per GPU; torch is used only for device memory, streams, graph capture and RCCL.
  * NHWC fp32.  A conv output is written ONCE as the raw pre-BatchNorm tensor; BatchNorm (+ReLU/ReLU6)
    of a producer is a per-channel (scale, shift, act) "view" applied on load by its consumers, so
    the 54 BN + 37 activation passes of the reference graph cost no HBM traffic.
  * BN batch statistics / BN-backward sums / weight gradients are deterministic partial reductions
    written by the producing kernel's epilogue and folded by tiny finalize kernels.
  * Concatenate is zero-copy: producers write channel slices of one buffer (ld = total channels).
  * gradients w.r.t. a buffer are accumulated by its consumers' bwd-data epilogues (mask -> add ->
    BN-backward partial sums), residual Adds are gradient aliases.
Reference call stack being replaced: Keras Model.predict / train_on_batch -> TF Session.run.
"""
import ctypes
import math
import os
import types

import numpy as np
import torch

from . import capi, regularizers
from .capi import ACT_NONE, ACT_RELU, ACT_RELU6, IMPL_AUTO, ptr
from .graph import check_focal, check_jaccard, check_mining, raw_pixels
from .head import Head

_ACT = {"relu": ACT_RELU, "relu6": ACT_RELU6}
V_SCALE, V_SHIFT, V_MEAN, V_INVSTD, V_CA, V_CB, V_CC, V_NEGMEAN = range(8)


def pixels_to_device(x, device, non_blocking=False):
    """raw 0-255 pixels (graph.raw_pixels) as a contiguous tensor on `device`: uint8 stays uint8 — decoded images cross
    PCIe as bytes and are widened by the kernel that reads them —, every other dtype becomes float32"""
    x = raw_pixels(x)
    if torch.is_tensor(x):
        t = x.to(device, non_blocking=non_blocking)
        return (t if t.dtype == torch.uint8 else t.to(torch.float32)).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device, non_blocking=non_blocking)


def flat_f32(a, device, non_blocking=False):
    """labels [B,HW,1] / sample weights [B,HW], a host array or a tensor, as a flat float32 tensor on `device`"""
    if torch.is_tensor(a):
        return a.reshape(-1).to(device, torch.float32, non_blocking=non_blocking)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))).to(device, non_blocking=non_blocking)


def argmax_rows(t, M, C):
    """dl3_argmax on the current stream: the first maximum of each row of the float32 device tensor t, read as [M,C]
    -> int32 [M] on t's device"""
    out = torch.empty(M, dtype=torch.int32, device=t.device)
    capi.call("dl3_argmax", ptr(t), out.data_ptr(), M, C, capi.stream())
    return out


_ARG_NAMES = {}


def arg_names(name):
    """the parameter names include/dl3.h gives entry point `name`, in order, without the trailing stream (parsed once
    per entry point)"""
    if name not in _ARG_NAMES:
        _ARG_NAMES[name] = tuple(a for _, a in capi.protos()[name][1][:-1])
    return _ARG_NAMES[name]


class Launch(tuple):
    """One recorded launch: (name, fn, args, ws_index).  args is the mutable list of the call's arguments in the header's
    order (the replay appends the stream); ws_index is the position of the scratch pointer the engine patches in once
    the scratch is sized, or None.  Arguments are read and patched by the names include/dl3.h gives them."""
    __slots__ = ()

    def _at(self, key):
        names = arg_names(self[0])
        if key not in names:
            raise ValueError("%s has no parameter %r; include/dl3.h names %s" % (self[0], key, ", ".join(names)))
        return names.index(key)

    def arg(self, key):
        return self[2][self._at(key)]

    def set(self, key, value):
        self[2][self._at(key)] = value


class Plan:
    """One launch sequence of an engine under the capture rule all of its plans share: the first counted run() calls
    `body` eagerly (module loading, allocator warm-up), the second captures it as one hipGraph and replays that, every
    later one replays.  With eng.use_graph off nothing is counted or captured.  A capture that raises switches use_graph
    off — for the whole engine: its other plans stop capturing too — and runs this call eagerly."""

    def __init__(self, eng, body):
        self.eng, self.body, self.calls, self.graph = eng, body, 0, None

    def run(self):
        if not self.eng.use_graph:
            return self.body()
        if self.calls >= 1 and self.graph is None:
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):   # records the launches; nothing executes until the replay below
                    self.body()
                self.graph = g
            except Exception as e:  # depends on the runtime
                print("dl3: hipGraph capture failed (%s); running eagerly" % e)
                self.eng.use_graph = False
                torch.cuda.synchronize()
                return self.body()
        if self.graph is not None:
            self.graph.replay()
        else:
            self.body()
        self.calls += 1


def _unbias_keras224(n, eps):
    """Keras 2.2.4 BatchNormalization.call on the TF 1.13 backend (the reference's environment):
    tf.nn.fused_batch_norm hands back the Bessel-corrected batch variance (n/(n-1)) and the layer multiplies it by
    sample_size / (sample_size - (1.0 + epsilon)) once more before the moving-average update."""
    return (n / (n - 1.0) if n > 1 else 1.0) * (n / (n - (1.0 + eps)) if n > 1.0 + eps else 1.0)


# moving_variance update factor on the biased batch variance (dl3_bn_finalize var_unbias), as a function of (n, eps)
BN_VARIANCE = {
    "keras224": _unbias_keras224,
    "bessel": lambda n, eps: n / (n - 1.0) if n > 1 else 1.0,   # tf.keras / plain FusedBatchNorm
    "biased": lambda n, eps: 1.0,
}


# tf.nn.fused_batch_norm (tensorflow/python/ops/nn_impl.py, TF 1.13) raises every epsilon to at least 1.001e-5 before the
# kernel sees it, and Keras 2.2.4 sends every 4-D BatchNormalization through it in both phases (training:
# K.normalize_batch_in_training -> _fused_normalize_batch_in_training; inference: K.batch_normalization ->
# fused_batch_norm(is_training=False)).  The 1e-5 layers of the ASPP / decoder (deeplabv3p.py:379,386,393-399,408,422-423,
# 427-429) therefore normalise with 1.001e-5.  The engine applies the floor where the Python wrapper does — in front of the
# kernels (dl3_bn_finalize / _direct / _frozen / _frozen_centered take the epsilon they are given); the moving-variance
# factor of BatchNormalization.call keeps the layer's own epsilon.
FUSED_BN_MIN_EPSILON = 1.001e-5


def fused_bn_epsilon(eps):
    eps = float(eps)
    return eps if eps > FUSED_BN_MIN_EPSILON else FUSED_BN_MIN_EPSILON


# BatchNorm over at most this many rows takes its batch statistics straight from the tensor (dl3_bn_finalize_direct)
SMALL_BN_ROWS = 4096


def _same_pads(size, k, stride, rate):
    out = -(-size // stride)
    total = max((out - 1) * stride + (k - 1) * rate + 1 - size, 0)
    return out, total // 2


# ------------------------------------------------------------------ physical channel counts
def stored_channels(c):
    """channels a tensor is STORED with.  A pixel row that is not a whole number of 128-byte lines makes every
    32-channel slab of the depthwise kernels straddle two lines: measured on MI355X, 16x64x64xC rate 2, forward /
    backward: C=728 4.03 / 3.26 TB/s, C=736 6.44 / 4.44 TB/s (tools/dw_rates.py align).  Xception's 728-channel tensors
    (entry_flow_block3 .. exit_flow_block1, 50+ depthwise layers) are therefore stored 736 wide: the 8 extra channels
    carry zero weights, zero gamma / beta, and stay exactly zero forward and backward.  Only when the padding costs
    <= 2 % traffic (144 -> 160 would cost 11 % and gains nothing net)."""
    p = (c + 31) // 32 * 32
    return p if (p - c) <= 0.02 * c else c


def plan_channels(model):
    """{id(tensor): physical channel count}: a Conv2D may widen its output (zero columns), every other layer
    propagates its input's width; producers that write slices of a Concatenate keep their logical width so that the
    slices stay adjacent"""
    nopad = set()
    for l in model._topo:
        if l.kind == "Concatenate":
            for t in l.inbound:
                p = t.layer
                while p.kind not in ("Conv2D", "DepthwiseConv2D", "Add", "InputLayer", "Subpixel", "Concatenate"):
                    p = p.inbound[0].layer
                nopad.add(id(p))
    phys = {}
    for l in model._topo:
        if l is model.input.layer:
            phys[id(l.output)] = l.output.shape[-1]
            continue
        cin = [phys[id(t)] for t in l.inbound]
        if l.kind == "Conv2D":
            f = l.cfg["filters"]
            # only 1x1 convolutions widen their output: the dense 3x3 lowering (Conv3Unit) sizes its kernel and buffers
            # from the logical filter count
            c = f if (id(l) in nopad or l.cfg["k"] != 1) else stored_channels(f)
        elif l.kind == "Subpixel":
            c = l.cfg["out_filters"]
        elif l.kind == "Concatenate":
            c = sum(cin)
        elif l.kind == "Add":
            if len(set(cin)) != 1:
                raise NotImplementedError("Add of tensors stored with different channel counts (%s)" % l.name)
            c = cin[0]
        else:  # same logical width as the input: same stored width; otherwise (none on the path) the logical one
            c = cin[0] if l.inbound[0].shape[-1] == l.output.shape[-1] else l.output.shape[-1]
        phys[id(l.output)] = c
    return phys


def device_shape(phys, l, name, hshape):
    """device shape of a weight: channel dimensions follow the stored width of the layer's input / output"""
    cin = phys[id(l.inbound[0])] if l.inbound else None
    cout = phys[id(l.output)]
    if name.endswith("/depthwise_kernel:0"):
        return (hshape[0], hshape[1], cin, 1)
    if name.endswith("/kernel:0"):
        if l.kind == "Subpixel":
            return (hshape[0], hshape[1], cin, hshape[3])
        return (hshape[0], hshape[1], cin, cout)
    if l.kind == "Subpixel":
        return tuple(hshape)
    return (cout,)  # bias, gamma, beta, moving statistics


class Buf:
    """One device tensor [N*H*W, ld] + its per-channel vectors + gradient accounting."""

    def __init__(self, eng, N, H, W, ld, name, requires_grad=True):
        self.eng, self.N, self.H, self.W, self.ld, self.name = eng, N, H, W, ld, name
        self.M = N * H * W
        self.t = eng.empty(self.M * ld)
        v = torch.zeros(8, ld, dtype=torch.float32)
        v[V_SCALE] = 1.0
        v[V_CA] = 1.0
        self.vec = v.to(eng.device)
        self.bns = []          # (bn_layer, c_off, C)
        self.requires_grad = requires_grad
        self.expected = 0      # gradient contributions to come (consumer units)
        self.done = 0
        self.grad = None       # tensor [M, ld]
        self.addend = None     # pending pass-through gradient (tensor [M, ld])
        self.nonneg = False
        self.centred = set()   # channel offsets of slices stored as y - moving_mean (PwUnit.set_output_offset)

    def vptr(self, row, off=0):
        return self.vec.data_ptr() + 4 * (row * self.ld + off)


class View:
    """A Keras tensor as the engine sees it: channel slice of a Buf, read as act(scale*x+shift)."""

    def __init__(self, buf, off, C, act=ACT_NONE, aff=False, pad=None, shape=None):
        self.buf, self.off, self.C, self.act, self.aff, self.pad = buf, off, C, act, aff, pad
        self.shape = shape or (buf.N, buf.H, buf.W, C)

    def derive(self, **kw):
        d = dict(buf=self.buf, off=self.off, C=self.C, act=self.act, aff=self.aff, pad=self.pad, shape=self.shape)
        d.update(kw)
        return View(**d)

    @property
    def ld(self):
        return self.buf.ld

    def p(self):
        return self.buf.t.data_ptr() + 4 * self.off

    def scale(self):
        return self.buf.vptr(V_SCALE, self.off) if self.aff else None

    def shift(self):
        return self.buf.vptr(V_SHIFT, self.off) if self.aff else None

    def xform(self):
        return (self.scale(), self.shift(), self.act)


class Engine:
    def __init__(self, model, batch, training, bn_mode="batch", dropout=True, seed=2, device=None, use_graph=True,
                 dw_impl=IMPL_AUTO, rank=None, bn_variance="keras224", external_nnz=False, opt_trainable=None, bn_update=None,
                 mining=None, jaccard=None, focal=None, l2=None):
        if not torch.cuda.is_available():
            raise capi.DL3Error("the dl3 engine needs a GPU (HIP device); there is no CPU fallback")
        self.lib = capi.lib()
        self.model, self.B, self.training = model, int(batch), bool(training)
        # {layer name: bool}: whose weights the optimizer updates (Keras: collected at compile()) / whose update ops run
        # (Keras: collected when the train function is built); None: the live `layer.trainable` (graph.Model._training_flags)
        self._opt_trainable = opt_trainable or {}
        self._bn_update = bn_update or {}
        self.bn_batch = self.training and bn_mode == "batch"
        self.dropout = bool(dropout) and self.training
        # Dropout mask = f(seed, step, element): every data-parallel rank draws its own masks, every step a new one
        self.rank = int(os.environ.get("RANK", "0")) if rank is None else int(rank)
        self.seed = (int(seed) + 0x632BE59BD9B4E019 * self.rank) & 0xFFFFFFFFFFFFFFFF
        if bn_variance not in BN_VARIANCE:
            raise ValueError("bn_variance must be one of %s" % sorted(BN_VARIANCE))
        self.bn_variance = bn_variance
        # data parallel: the loss normaliser count(w != 0) is the GLOBAL batch's (the reference's multi_gpu_model merges
        # the tower outputs and evaluates ONE loss, utils.py:209-211) — the host writes it before each step instead of
        # the in-graph dl3_count_nonzero of the local shard (Engine.set_nnz)
        self.external_nnz = bool(external_nnz)
        # hard-example mining: (top_k_percent_pixels, hard_example_mining_step) — the step trains on the k
        # largest per-pixel losses, k from the schedule and the device-side step counter; None / p == 1: today's plan
        self.mining = check_mining(mining) if training else None
        # soft-Jaccard term: the step minimises CE + jaccard * L_J; None / 0: today's plan
        self.jaccard = check_jaccard(jaccard) if training else None
        if self.jaccard and self.mining:
            raise ValueError("the soft-Jaccard loss and hard-example mining are separate losses and cannot be combined")
        if self.jaccard and self.external_nnz:
            raise ValueError("the soft-Jaccard loss cannot ride a data-parallel (external_nnz) engine: the optimizer "
                             "finishes ONE gradient scale from the all-reduced count, and the Jaccard term has another "
                             "normaliser")
        # focal loss: (gamma, alpha) — pixel-wise with the cross-entropy's normaliser, so it takes the
        # place of the loss launch in whichever form the head admits and rides a data-parallel engine unchanged;
        # None / gamma == 0 with alpha None or all ones: today's plan
        self.focal = check_focal(focal) if training else None
        if self.focal and (self.mining or self.jaccard):
            raise ValueError("the focal loss, hard-example mining and the soft-Jaccard loss are separate losses and cannot "
                             "be combined")
        # L2 weight regularisers: the table {weight name: l} Model.compile() collected, in its normal form
        # (regularizers.normal_form); the penalty launches sit behind the captured step, in front of the clip and the
        # update (l2_penalty).  None / empty: no launch, today's step
        self.l2 = regularizers.normal_form(l2) if training else None
        self._l2_eval = {}   # table -> device tables of l2_value (evaluation: value-only launches)
        self.device = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
        self.use_graph = use_graph
        self.fold_tail = True   # the loss kernel folds its gradient rows onto the low-resolution columns (the full-resolution dlogits never exist)
        self.dw_impl = dw_impl
        self.ops_prep, self.ops_fwd, self.ops_bwd = [], [], []
        # backward fork (round 3, opt-in: DL3_FORK=1): the 1x1-conv weight gradients are off the critical path until Adam —
        # they leave the backward chain as a second captured stream (event fork behind the launch that completes their dY,
        # one join at the end).  Measured SLOWER at every batch size (two 256-VGPR workgroups fill a CU), so
        # the default is one stream; kept because it is tested bit-identical and documents the experiment.
        self.poison = os.environ.get("DL3_POISON_SCRATCH", "0") == "1"
        # every weight-gradient slab fold of the backward pass in ONE launch at its end (DL3_BATCH_FOLDS=0: one
        # dl3_reduce_partials behind each weight-gradient launch, bit-identical — a test toggles it)
        self.batch_folds = os.environ.get("DL3_BATCH_FOLDS", "1") == "1"
        # ... of the folds whose partial rows are small: a deferred fold re-reads its slabs from HBM instead of the cache
        # they were just written through, which costs more than the launch it saves from ~12 MB on (Xception B=16 with
        # every fold deferred: 193.9 -> 196.4 ms)
        self.fold_defer_bytes = 8 << 20
        self.own_fold_ws_bytes = 0   # device memory of the deferred folds' own slab workspaces (reported by bench.py)
        self._folds = []
        # round 4: the weight-gradient launch of a BatchNorm'ed 1x1 convolution also writes dY = cA*g + cB*y + cC (it
        # assembles it anyway), and the bwd-data GEMM of the layer reads that ONE tensor (dl3_pwconv_bwd_weight_dy).  The
        # write is paid by the weight-gradient launch: cheap next to a wide X (project convolutions, +0.02-0.06 ms against
        # -0.3-0.7 ms of bwd-data at B=128) but not for an HBM-bound launch with a narrow X and a wide dY (16 -> 96 at
        # 256x256: +0.88 ms against -0.65): only where N <= K or K >= 96 (DL3_DY_MAT=0 disables)
        # (second look, same call: the criterion is the width of X against dY, not the width of dY: N <= K or K >= 96)
        self.dy_mat = os.environ.get("DL3_DY_MAT", "1") != "0"
        self.dy_mat_mink = 96
        # both gradients of an HBM-bound 1x1 convolution with a small weight matrix in one pass (dl3_pwconv_bwd_fused):
        # layers with at least DL3_FUSED_ROWS pixel rows (DL3_FUSED_BWD=0 disables)
        self.fused_bwd = os.environ.get("DL3_FUSED_BWD", "1") != "0"
        self.fused_min_rows = int(os.environ.get("DL3_FUSED_ROWS", "32768"))
        self.dy_buf = None
        self.fork = os.environ.get("DL3_FORK", "0") in ("1", "2")
        # DL3_FORK=2 (experiment): only the weight gradient that can run next to an HBM-bound depthwise backward launch
        # leaves the chain, and the chain's next GEMM waits for it: matrix-bound and HBM-bound kernels overlap, two GEMMs never do
        self.fork_pairs = os.environ.get("DL3_FORK", "0") == "2"
        self._join_before = set()   # id(op record): the main stream waits for the side stream before this launch
        self.bn_sites = []
        self.add_of_buf = {}        # id(Add output Buf) -> AddUnit
        self.prestat = {}           # id(Buf) -> (dpart, P, ld): BatchNorm-backward sums already reduced by a producer's epilogue
        self._side = set()          # id(op record) of the launches that run on the side stream
        self._side_stream = None
        self._fork_events = []
        self.side_scratch_bytes = 0
        self._scratch_users, self._side_scratch_users = [], []   # launches whose `workspace` is the shared scratch
        self.units = []
        self.views = {}
        self.bufs = []
        self.scratch_bytes = 0
        self.iteration = 0
        # the main plan: the whole step (fwd_bwd) of a training engine, the forward pass of an inference engine
        self._main = Plan(self, self._run_main)
        self._keep = []
        self.drop_step = torch.zeros(1, dtype=torch.int64, device=self.device)  # device-side step number (dropout)
        # device-side count of the steps taken (the mining schedule's s: launch arguments are frozen inside the hipGraph)
        self.mine_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._plan_channels()
        self._build_params()
        self._lower()
        if self.training:
            self._lower_backward()
            if self.dropout:
                self.op(self.ops_bwd, "dl3_counter_add", self.drop_step.data_ptr(), 1)
            if self.mining:
                self.op(self.ops_bwd, "dl3_counter_add", self.mine_step.data_ptr(), 1)
        self.scratch = self.empty(max(self.scratch_bytes // 4, 4))
        for rec in self._scratch_users:
            rec.set("workspace", self.scratch.data_ptr())
        if self._side_scratch_users:  # the side stream's launches are ordered among themselves: one workspace of their own
            self.side_scratch = self.empty(max(self.side_scratch_bytes // 4, 4))
            for rec in self._side_scratch_users:
                rec.set("workspace", self.side_scratch.data_ptr())
        self.dirty = True

    # ------------------------------------------------------------------ memory
    def empty(self, n):
        t = torch.empty(int(n), dtype=torch.float32, device=self.device)
        if self.poison:   # DL3_POISON_SCRATCH=1 (test aid): a launch that reads scratch nobody wrote turns the loss into NaN
            t.fill_(float("nan"))
        self._keep.append(t)
        return t

    def zeros(self, n):
        t = torch.zeros(int(n), dtype=torch.float32, device=self.device)
        self._keep.append(t)
        return t

    def _plan_channels(self):
        self.phys = plan_channels(self.model)

    def _dshape(self, l, name, hshape):
        return device_shape(self.phys, l, name, hshape)

    @staticmethod
    def _pad_to(name, w, dshape):
        w = np.asarray(w, np.float32)
        if tuple(w.shape) == tuple(dshape):
            return w
        out = np.full(dshape, 1.0 if name.endswith("/moving_variance:0") else 0.0, np.float32)
        out[tuple(slice(0, n) for n in w.shape)] = w
        return out

    def _build_params(self):
        """Flat arenas: trainable parameters (kernels, biases, gamma, beta) | state (moving statistics and the
        weights of non-trainable layers).  One RCCL all-reduce and one Adam launch cover the whole model."""
        self.slots = {}
        self.hshape = {}
        np_, ns = 0, 0
        for l in self.model.layers:
            for name, w in l.weights.items():
                dshape = self._dshape(l, name, w.shape)
                size = int(np.prod(dshape))
                n = (size + 3) // 4 * 4
                self.hshape[name] = tuple(w.shape)
                if self._opt_trainable.get(l.name, l.trainable) and "/moving_" not in name:
                    self.slots[name] = ("p", np_, size, dshape, l)
                    np_ += n
                else:
                    self.slots[name] = ("s", ns, size, dshape, l)
                    ns += n
        self.n_param = np_
        self.params = self.zeros(max(np_, 4))
        self.state = self.zeros(max(ns, 4))
        # [count(w != 0) of the shard, loss sum of the shard, 0, 0] ride behind the gradients in the arena exchange
        # (data-parallel engines, Engine.train_step)
        self.tail = (max(np_, 4) + 3) // 4 * 4
        if self.training:
            self.grads = self.zeros(self.tail + 4)
            # optimizer slots 0 / 1: Adam's m / v; SGD's momentum buffer and RMSprop's accumulator live in slot 0
            self.adam_m = self.zeros(max(np_, 4))
            self.adam_v = self.zeros(max(np_, 4))
            # the global gradient norm of clipnorm (dl3_grad_sumsq): per-workgroup partials and the 8-byte result
            ws = int(self.lib.dl3_grad_sumsq_workspace_bytes(max(np_, 4)))
            self.sumsq_ws = torch.zeros((ws + 7) // 8, dtype=torch.float64, device=self.device)
            self.grad_sumsq = torch.zeros(1, dtype=torch.float64, device=self.device)
            self.dummy_grad = self.zeros(4096)
            self._l2 = self._l2_tables(self.l2) if self.l2 else None
        self.sync_all_to_device()

    def _arena(self, kind):
        return self.params if kind == "p" else self.state

    # ------------------------------------------------------------------ L2 weight regularisers
    def _l2_tables(self, table):
        """dl3_l2_penalty's device-resident run tables (regularizers.build_runs) over the parameter and the state arena,
        their partial-sum workspaces and the result: out = [parameter-arena value, the same as a float, state-arena value,
        the same as a float]; an arena without a regularised weight has no table and its value stays 0"""
        tabs = dict(out=torch.zeros(4, dtype=torch.float64, device=self.device), arenas=[])
        for kind in "ps":
            runs, coef, tiles = regularizers.build_runs(self.slots, table, kind)
            if not len(coef):
                tabs["arenas"].append(None)
                continue
            ws = int(self.lib.dl3_l2_penalty_workspace_bytes(tiles))
            tabs["arenas"].append(dict(
                runs=torch.from_numpy(runs).to(self.device), coef=torch.from_numpy(coef).to(self.device), S=len(coef),
                tiles=tiles, ws=torch.zeros((ws + 7) // 8, dtype=torch.float64, device=self.device)))
        return tabs

    def _l2_launch(self, tabs, grad_scale=1.0, denom=None, grads=False):
        """the penalty launches: parameter arena first (grads: with the gradient addend onto self.grads), then the state
        arena, whose weights the optimizer does not update — value only"""
        stream = torch.cuda.current_stream().cuda_stream
        for i, (a, arena) in enumerate(zip(tabs["arenas"], (self.params, self.state))):
            if a is None:
                continue
            g = ptr(self.grads) if grads and i == 0 else None
            capi.call("dl3_l2_penalty", ptr(arena), g, a["runs"].data_ptr(), a["coef"].data_ptr(), a["S"], a["tiles"],
                      grad_scale if g else 1.0, denom if g else None, tabs["out"].data_ptr() + 16 * i, a["ws"].data_ptr(),
                      a["ws"].numel() * 8, stream)

    @staticmethod
    def _l2_sum(out):
        """the penalty from a host copy of `out`: parameter arena + state arena, in double"""
        return float(out[0]) + float(out[2])

    def l2_penalty(self, grad_scale=1.0):
        """between the backward pass (and the all-reduce, where there is one) and opt_step: the penalty of the weights as
        they are BEFORE the update, and 2*l*w onto the gradient arena, divided by the scale opt_step(grad_scale) is about
        to multiply the arena by — on an external_nnz engine normaliser / count_all from the arena tail.  The clip that
        follows sees the gradient of the total loss.  Nothing regularised: no launch."""
        if not self.l2:
            return
        denom = None
        if self.external_nnz:
            grad_scale, denom = self.nnz_host, self.grads.data_ptr() + 4 * self.tail
        self._l2_launch(self._l2, grad_scale, denom, grads=True)

    def l2_value(self, table):
        """the penalty of `table` ({weight name: l} or its normal form) at the resident weights, for evaluation: value-only
        launches over both arenas and one read"""
        table = regularizers.normal_form(table)
        if not table:
            return 0.0
        if table not in self._l2_eval:
            self._l2_eval[table] = self._l2_tables(table)
        tabs = self._l2_eval[table]
        self._l2_launch(tabs)
        return self._l2_sum(tabs["out"].cpu())

    def wptr(self, name):
        kind, off, _, _, _ = self.slots[name]
        return self._arena(kind).data_ptr() + 4 * off

    def gptr(self, name, size=0):
        """gradient slot of a weight; non-trainable weights get a throw-away slot"""
        kind, off, n, _, _ = self.slots[name]
        if kind == "p":
            return self.grads.data_ptr() + 4 * off
        if n > self.dummy_grad.numel():
            self.dummy_grad = self.zeros(n)
        return self.dummy_grad.data_ptr()

    def trainable(self, name):
        return self.slots[name][0] == "p"

    def sync_all_to_device(self):
        hp = np.zeros(self.params.numel(), np.float32)
        hs = np.zeros(self.state.numel(), np.float32)
        for name, (kind, off, n, shp, l) in self.slots.items():
            (hp if kind == "p" else hs)[off:off + n] = self._pad_to(name, l.weights[name], shp).reshape(-1)
        self.params.copy_(torch.from_numpy(hp))
        self.state.copy_(torch.from_numpy(hs))
        self.dirty = True

    def sync_all_to_host(self):
        hp = self.params.cpu().numpy()
        hs = self.state.cpu().numpy()
        for name, (kind, off, n, shp, l) in self.slots.items():
            l.weights[name] = self._unpad(name, (hp if kind == "p" else hs)[off:off + n].reshape(shp))

    def sync_layer_to_host(self, layer):
        for name in layer.weights:
            kind, off, n, shp, _ = self.slots[name]
            layer.weights[name] = self._unpad(name, self._arena(kind)[off:off + n].cpu().numpy().reshape(shp))

    def sync_layer_to_device(self, layer):
        for name, w in layer.weights.items():
            kind, off, n, shp, _ = self.slots[name]
            self._arena(kind)[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(self._pad_to(name, w, shp).reshape(-1))))
        self.dirty = True

    def _unpad(self, name, arr):
        """device layout -> the Keras shape of the weight (drops the zero channels of _cp)"""
        return arr[tuple(slice(0, n) for n in self.hshape[name])].copy()

    def activate(self):
        """make this engine the one that layer.get_weights()/set_weights() talk to"""
        for l in self.model.layers:
            l._engine = self

    # ------------------------------------------------------------------ op recording
    def op(self, lst, name, *args, ws=None, side=False):
        """record the launch name(*args, stream) at the end of lst.  The argument count is checked against include/dl3.h
        here, while lowering.  side: the launch may leave the backward chain (see self.fork).  ws=nbytes: it takes the
        shared scratch — the side stream's where it goes there — through the parameter the header calls `workspace`
        (the call site passes 0 there; the pointer is patched in once the scratch's size is known)"""
        names = arg_names(name)
        if len(args) != len(names):
            raise TypeError("%s takes %d arguments in front of the stream (include/dl3.h), %d were recorded"
                            % (name, len(names), len(args)))
        side = side and self.fork
        rec = Launch((name, getattr(self.lib, name), list(args), None if ws is None else names.index("workspace")))
        lst.append(rec)
        if side:
            self._side.add(id(rec))
        if ws is not None and side:
            self.side_scratch_bytes = max(self.side_scratch_bytes, int(ws))
            self._side_scratch_users.append(rec)
        elif ws is not None:
            self.scratch_bytes = max(self.scratch_bytes, int(ws))
            self._scratch_users.append(rec)
        return rec

    def defer_fold(self, P, n):
        return self.batch_folds and 4 * int(P) * int(n) <= self.fold_defer_bytes

    def fold(self, src_ptr, P, n, dst_ptr):
        """dst[n] = sum over the P partial rows at src: now, or with every other fold in one launch (self.batch_folds)"""
        if self.defer_fold(P, n):
            self._folds.append((int(src_ptr), int(dst_ptr), int(P), int(n)))
        else:
            self.op(self.ops_bwd, "dl3_reduce_partials", src_ptr, P, n, dst_ptr)

    def run_ops_forked(self, lst):
        """lst with the launches marked in self._side on a second stream: each one waits for the event recorded on the
        main stream at its position in the plan (everything it reads is complete there and is never written again within
        the step), the main stream joins the side stream at the end.  Under hipGraph capture this becomes a parallel
        branch of the graph."""
        main = torch.cuda.current_stream()
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        side = self._side_stream
        mst, sst = main.cuda_stream, side.cuda_stream
        pending = True  # the main stream has moved on since the side stream last synchronised with it
        nev = 0
        for rec in lst:
            name, fn, args, _ = rec
            if id(rec) in self._join_before:
                main.wait_stream(side)
            if id(rec) in self._side:
                if pending:
                    if nev == len(self._fork_events):
                        self._fork_events.append(torch.cuda.Event())
                    ev = self._fork_events[nev]
                    nev += 1
                    ev.record(main)
                    side.wait_event(ev)
                    pending = False
                rc = fn(*args, sst)
            else:
                rc = fn(*args, mst)
                pending = True
            if rc != 0:
                capi.check(rc, name)
        main.wait_stream(side)

    def transpose(self, src_ptr, dst, rows, cols):
        """queue dst[cols][rows] = src[rows][cols]^T for the batched transpose at the head of the backward pass"""
        self._transposes.append((int(src_ptr), dst, int(rows), int(cols)))

    def run_ops(self, lst):
        st = torch.cuda.current_stream().cuda_stream
        for name, fn, args, _ in lst:
            rc = fn(*args, st)
            if rc != 0:
                capi.check(rc, name)

    # ------------------------------------------------------------------ forward lowering
    def _lower(self):
        m = self.model
        topo = m._topo
        self.consumers = {}
        for l in topo:
            for t in (l.inbound if l is not m.input.layer else []):
                self.consumers.setdefault(id(t), []).append(l)
        self.placement = {}
        self.concat_bufs = {}
        self.bcast_resize = {}   # id(ResizeBilinear layer) -> the Concatenate it feeds as a per-image constant
        self.bcast_src = {}      # id(concat Buf) -> (View of the 1x1 source, channels)
        for l in topo:
            if l.kind == "Concatenate":
                self._place_concat(l)
        self.unit_of_buf = {}
        for l in topo:
            getattr(self, "_lo_" + l.kind)(l)
        out = self.views[id(m.output)]
        self.out_view = out
        self._check_centred_consumers()

    def _check_centred_consumers(self):
        """a slice stored as y - mean (centred frozen BatchNorm) must never be read raw: every unit input that touches it
        has to be an affine view (the view carries the matching scale / shift)"""
        for u in self.units:
            for w in (getattr(u, "inv", None), getattr(u, "a", None), getattr(u, "b", None)):
                if w is None or not w.buf.centred:
                    continue
                hit = any(off < w.off + w.C and w.off < off + C for _, off, C in w.buf.bns if off in w.buf.centred)
                if hit and not w.aff:
                    raise RuntimeError("unit %s reads the centred tensor %s raw" % (type(u).__name__, w.buf.name))

    def _producer_of(self, t):
        l = t.layer
        while l.kind in ("BatchNormalization", "Activation") and l.cfg.get("fn") != "softmax":
            l = l.inbound[0].layer
        return l

    def _bcast_input(self, l):
        """the first input of Concatenate l if it is the bilinear 'resize' of a 1x1 map — a per-image constant, e.g. the
        ASPP image-pooling branch (deeplabv3p.py:375-382) — and the Concatenate feeds exactly one 1x1 convolution: that
        branch is then never materialised; the convolution adds its contribution once per image (PwUnit img_add)"""
        t = l.inbound[0]
        p = self._producer_of(t)
        cs = self.consumers.get(id(l.output), [])
        if (p.kind == "ResizeBilinear" and p is t.layer and tuple(p.inbound[0].shape[:2]) == (1, 1) and len(l.inbound) > 1
                and len(cs) == 1 and cs[0].kind == "Conv2D" and cs[0].cfg["k"] == 1 and cs[0].cfg["stride"] == 1
                and len(self.consumers.get(id(t), [])) == 1):
            return p
        return None

    def _place_concat(self, l):
        H, W, C = l.output.shape
        bc = self._bcast_input(l)
        if bc is not None:
            self.bcast_resize[id(bc)] = l
            C -= l.inbound[0].shape[2]
        buf = Buf(self, self.B, H, W, C, l.name)
        self.bufs.append(buf)
        self.concat_bufs[id(l)] = buf
        off = 0
        for t in l.inbound:
            if bc is not None and t is l.inbound[0]:
                continue
            p = self._producer_of(t)
            ok = (p.kind in ("Conv2D",) and p.cfg["k"] == 1 and p.cfg["stride"] == 1) or p.kind == "ResizeBilinear"
            if p.kind == "Dropout" or not ok:
                raise NotImplementedError("Concatenate input produced by %s (%s) is not on the path" % (p.name, p.kind))
            self.placement[id(p)] = (buf, off)
            off += t.shape[2]

    def _new_out(self, l, H, W, C):
        """output buffer of a producing layer: a concat slice if placed, else a fresh Buf"""
        if id(l) in self.placement:
            buf, off = self.placement[id(l)]
            return buf, off
        buf = Buf(self, self.B, H, W, C, l.name)
        self.bufs.append(buf)
        return buf, 0

    def _in(self, l, i=0):
        return self.views[id(l.inbound[i])]

    def _consume(self, view):
        if view.buf.requires_grad:
            view.buf.expected += 1

    def _bn_follows(self, l):
        cs = self.consumers.get(id(l.output), [])
        return len(cs) == 1 and cs[0].kind == "BatchNormalization"

    def _want_stat(self, l, rows):
        """does the convolution's epilogue reduce BatchNorm partial sums?  (small tensors: dl3_bn_finalize_direct)"""
        return self.bn_batch and self._bn_follows(l) and rows > SMALL_BN_ROWS

    def _stat_buf(self, P, C):
        return self.empty(P * C * 2)

    # ---- layers ---------------------------------------------------------------------
    def _lo_InputLayer(self, l):
        H, W, C = l.output.shape
        self.xbuf = Buf(self, self.B, H, W, C, "input", requires_grad=False)
        self.bufs.append(self.xbuf)
        self.views[id(l.output)] = View(self.xbuf, 0, C)

    def _lo_Prescale(self, l):
        v = self._in(l)
        assert v.buf is self.xbuf and not v.aff
        vec = v.buf.vec.cpu()
        vec[V_SCALE] = 1.0 / 127.5
        vec[V_SHIFT] = -1.0
        v.buf.vec.copy_(vec)
        self.views[id(l.output)] = v.derive(aff=True)

    def _lo_ZeroPadding2D(self, l):
        v = self._in(l)
        (pt, pb), (pl, pr) = l.cfg["pad"]
        assert v.pad is None
        self.views[id(l.output)] = v.derive(pad=(pt, pl))

    def _lo_Activation(self, l):
        v = self._in(l)
        fn = l.cfg["fn"]
        if fn == "softmax":
            return self._lo_softmax(l, v)
        if v.act != ACT_NONE:
            # relu(relu(x)) == relu(x), relu(relu6(x)) == relu6(x), relu6(relu(x)) == relu6(x) — values and gradient
            # masks alike (Xception: entry_flow_block1 re-applies ReLU to an already rectified tensor)
            act = ACT_RELU6 if ACT_RELU6 in (v.act, _ACT[fn]) else ACT_RELU
            self.views[id(l.output)] = v.derive(act=act)
            return
        self.views[id(l.output)] = v.derive(act=_ACT[fn])

    def _lo_Reshape(self, l):
        self.views[id(l.output)] = self._in(l)

    def _lo_BatchNormalization(self, l):
        v = self._in(l)
        unit = self.unit_of_buf.get((id(v.buf), v.off))
        if v.aff or v.act != ACT_NONE or unit is None or unit.bn is not None:
            raise NotImplementedError("BatchNormalization %s must directly follow a convolution" % l.name)
        unit.bn = l
        C = v.C
        n = l.name
        v.buf.bns.append((l, v.off, C))
        if self.bn_batch:
            # Keras 2.2.x collects no updates from a non-trainable layer: a frozen BatchNormalization still normalises
            # with the batch statistics in the training phase, but its moving statistics stay as loaded
            upd = self._bn_update.get(l.name, l.trainable)
            if v.buf.M <= SMALL_BN_ROWS:
                # few rows (the image-pooling branch: one row per image): two-pass statistics straight from the tensor
                self.op(self.ops_fwd, "dl3_bn_finalize_direct", v.p(), v.ld, v.buf.M, C,
                        self.wptr(n + "/gamma:0"), self.wptr(n + "/beta:0"), fused_bn_epsilon(l.cfg["eps"]), l.cfg["momentum"],
                        BN_VARIANCE[self.bn_variance](float(v.buf.M), float(l.cfg["eps"])),
                        v.buf.vptr(V_SCALE, v.off), v.buf.vptr(V_SHIFT, v.off), v.buf.vptr(V_MEAN, v.off),
                        v.buf.vptr(V_INVSTD, v.off), self.wptr(n + "/moving_mean:0") if upd else None,
                        self.wptr(n + "/moving_variance:0") if upd else None)
                self.views[id(l.output)] = v.derive(aff=True)
                return
            self.bn_sites.append((len(self.ops_fwd), l, v.buf, v.off, C, unit))  # (index in ops_fwd, ...): diagnostics
            self.op(self.ops_fwd, "dl3_bn_finalize", ptr(unit.stat), unit.P, C, C, float(v.buf.M),
                    self.wptr(n + "/gamma:0"), self.wptr(n + "/beta:0"), fused_bn_epsilon(l.cfg["eps"]), l.cfg["momentum"],
                    BN_VARIANCE[self.bn_variance](float(v.buf.M), float(l.cfg["eps"])),
                    v.buf.vptr(V_SCALE, v.off), v.buf.vptr(V_SHIFT, v.off), v.buf.vptr(V_MEAN, v.off),
                    v.buf.vptr(V_INVSTD, v.off), self.wptr(n + "/moving_mean:0") if upd else None,
                    self.wptr(n + "/moving_variance:0") if upd else None)
        elif isinstance(unit, PwUnit) and unit.bias is None:
            # moving statistics, 1x1 convolution in front (round 4): the GEMM's free bias slot takes -mean, the tensor holds
            # y - mean and consumers read scale*(y - mean) + beta — the reference's own gamma*(x - mean)/sqrt(var + eps) +
            # beta instead of scale*y + (beta - mean*scale), whose shift carries half an ulp of |mean*scale| into every
            # element (dl3_bn_frozen_centered)
            negm = v.buf.vptr(V_NEGMEAN, v.off)
            self.op(self.ops_prep, "dl3_bn_frozen_centered", self.wptr(n + "/gamma:0"), self.wptr(n + "/beta:0"),
                    self.wptr(n + "/moving_mean:0"), self.wptr(n + "/moving_variance:0"), fused_bn_epsilon(l.cfg["eps"]), C,
                    v.buf.vptr(V_SCALE, v.off), v.buf.vptr(V_SHIFT, v.off), v.buf.vptr(V_MEAN, v.off),
                    v.buf.vptr(V_INVSTD, v.off), negm)
            unit.set_output_offset(negm)   # (the buffer holds y - mean from here on: Buf.centred)
        else:
            self.op(self.ops_prep, "dl3_bn_frozen", self.wptr(n + "/gamma:0"), self.wptr(n + "/beta:0"),
                    self.wptr(n + "/moving_mean:0"), self.wptr(n + "/moving_variance:0"), fused_bn_epsilon(l.cfg["eps"]), C,
                    v.buf.vptr(V_SCALE, v.off), v.buf.vptr(V_SHIFT, v.off), v.buf.vptr(V_MEAN, v.off),
                    v.buf.vptr(V_INVSTD, v.off))
        self.views[id(l.output)] = v.derive(aff=True)

    def _lo_Conv2D(self, l):
        v = self._in(l)
        if l.cfg["k"] == 3:
            return self._lo_conv3x3(l, v)
        if l.cfg["stride"] != 1:
            # Xception shortcut (deeplabv3p.py:143-145): compact the sampled pixels, then the ordinary GEMM
            st = l.cfg["stride"]
            Ho, Wo = l.output.shape[0], l.output.shape[1]
            cbuf = Buf(self, self.B, Ho, Wo, v.C, l.name + "_sub")
            self.bufs.append(cbuf)
            self.units.append(SubsampleUnit(self, v, View(cbuf, 0, v.C), st))
            v = View(cbuf, 0, v.C)
        Ho, Wo, N = v.shape[1], v.shape[2], self.phys[id(l.output)]
        buf, off = self._new_out(l, Ho, Wo, N)
        assert id(l) in self.placement or buf.ld == N, (l.name, buf.ld, N)  # an own buffer is exactly as wide as stored
        if id(v.buf) in self.bcast_src:
            # Concatenate([broadcast of a 1x1 map, per-pixel branches]) -> 1x1 convolution: rows 0..Cb-1 of the kernel meet a
            # per-image constant: a GEMM of B rows whose result is added once per image; the other rows run per pixel
            sv, Cb = self.bcast_src[id(v.buf)]
            if v.off != 0 or v.C != v.buf.ld:
                raise NotImplementedError("convolution over a slice of a Concatenate with a broadcast input")
            ib = Buf(self, self.B, 1, 1, N, l.name + "_per_image")
            self.bufs.append(ib)
            pu = PwUnit(self, l, sv, View(ib, 0, N), want_stat=False, wrow0=0, use_bias=False)
            self.units.append(pu)
            u = PwUnit(self, l, v, View(buf, off, N), want_stat=self._want_stat(l, buf.M), wrow0=Cb, img_add=ib)
            u.img_unit = pu
        else:
            u = PwUnit(self, l, v, View(buf, off, N), want_stat=self._want_stat(l, buf.M))
        self._register(u, buf, off)
        self.views[id(l.output)] = View(buf, off, N)

    def _lo_Subpixel(self, l):
        v = self._in(l)
        r, co = l.cfg["r"], l.cfg["out_filters"]
        k = l.cfg["k"]
        if l.cfg["stride"] != 1:
            raise NotImplementedError("Subpixel with strides != 1 (%s)" % l.name)
        if k != 1:
            # subpixel.py:42-58: any kernel_size.  The k x k taps of the input are gathered side by side (dl3_conv_taps_fwd)
            # and the Keras kernel [k][k][Cin][F], read as a [k*k*Cin][F] matrix, drives the same GEMM as the 1x1 case
            v = self._taps(l, v, k)
        Ho, Wo, N = v.shape[1], v.shape[2], l.cfg["filters"]
        buf = Buf(self, self.B, Ho, Wo, N, l.name)
        self.bufs.append(buf)
        u = PwUnit(self, l, v, View(buf, 0, N), want_stat=False)
        self._register(u, buf, 0)
        obuf = Buf(self, self.B, Ho * r, Wo * r, co, l.name + "_shift")
        self.bufs.append(obuf)
        s = ShuffleUnit(self, View(buf, 0, N), View(obuf, 0, co), r, co)
        self.units.append(s)
        self.views[id(l.output)] = View(obuf, 0, co)

    def _taps(self, l, v, k):
        N_, H, W, C = v.shape
        if l.cfg["padding"] == "same":
            Ho, pt = _same_pads(H, k, 1, 1)
            Wo, pl = _same_pads(W, k, 1, 1)
        else:
            Ho, Wo, pt, pl = H - k + 1, W - k + 1, 0, 0
        cbuf = Buf(self, self.B, Ho, Wo, k * k * C, l.name + "_taps")
        self.bufs.append(cbuf)
        out = View(cbuf, 0, k * k * C)
        self.units.append(TapsUnit(self, v, out, k, pt, pl))
        return out

    def _lo_conv3x3(self, l, v):
        N_, H, W, Cin = v.shape
        s = l.cfg["stride"]
        if l.cfg["padding"] == "same":
            Ho, pt = _same_pads(H, 3, s, 1)
            Wo, pl = _same_pads(W, 3, s, 1)
        else:
            pt, pl = v.pad or (0, 0)
            Ho, Wo = l.output.shape[0], l.output.shape[1]
        assert self.phys[id(l.output)] == l.cfg["filters"], "dense 3x3 outputs are stored at their logical width"
        buf, off = self._new_out(l, Ho, Wo, l.cfg["filters"])
        u = Conv3Unit(self, l, v, View(buf, off, l.cfg["filters"]), s, pt, pl,
                      want_stat=self._want_stat(l, buf.M))
        self._register(u, buf, off)
        self.views[id(l.output)] = View(buf, off, l.cfg["filters"])

    def _lo_DepthwiseConv2D(self, l):
        v = self._in(l)
        N_, H, W, C = v.shape
        if v.off != 0 or v.ld != C:
            raise NotImplementedError("depthwise conv on a channel slice (%s)" % l.name)
        if C % 4:   # (dw_check in csrc/dwconv.hip refuses it at the first launch: say so while lowering)
            raise NotImplementedError("depthwise conv over %d channels (%s): the kernels take multiples of 4" % (C, l.name))
        s, r = l.cfg["stride"], l.cfg["rate"]
        if l.cfg["padding"] == "same":
            Ho, pt = _same_pads(H, 3, s, r)
            Wo, pl = _same_pads(W, 3, s, r)
        else:
            pt, pl = v.pad or (0, 0)
            Ho, Wo = l.output.shape[0], l.output.shape[1]
        buf, off = self._new_out(l, Ho, Wo, C)
        u = DwUnit(self, l, v, View(buf, off, C), s, r, pt, pl, want_stat=self._want_stat(l, buf.M))
        self._register(u, buf, off)
        self.views[id(l.output)] = View(buf, off, C)

    def _register(self, u, buf, off):
        self.units.append(u)
        self.unit_of_buf[(id(buf), off)] = u

    def _lo_Add(self, l):
        a, b = self._in(l, 0), self._in(l, 1)
        H, W, C = l.output.shape
        C = self.phys[id(l.output)]
        buf = Buf(self, self.B, H, W, C, l.name)
        self.bufs.append(buf)
        self.units.append(AddUnit(self, a, b, View(buf, 0, C)))
        self.add_of_buf[id(buf)] = self.units[-1]
        self.views[id(l.output)] = View(buf, 0, C)

    def _lo_Concatenate(self, l):
        buf = self.concat_bufs[id(l)]
        acts = set()
        for t in l.inbound:
            v = self.views[id(t)]
            if v is None and id(buf) in self.bcast_src:
                sv = self.bcast_src[id(buf)][0]
                if sv.act != ACT_NONE:
                    acts.add(sv.act)
                continue
            if v.buf is not buf:
                raise NotImplementedError("concat input %s was not placed" % t.layer.name)
            if v.act != ACT_NONE:
                acts.add(v.act)
            elif not (v.buf.nonneg_slices.get(v.off, False) if hasattr(v.buf, "nonneg_slices") else False):
                raise NotImplementedError("concat input without activation must be known non-negative")
        if len(acts) > 1:
            raise NotImplementedError("concat inputs with different activations")
        act = acts.pop() if acts else ACT_NONE
        self.views[id(l.output)] = View(buf, 0, buf.ld, act=act, aff=True)

    def _lo_AveragePooling2D(self, l):
        v = self._in(l)
        C = v.C
        buf = Buf(self, self.B, 1, 1, C, l.name)
        self.bufs.append(buf)
        self.units.append(GapUnit(self, v, View(buf, 0, C)))
        self.views[id(l.output)] = View(buf, 0, C)

    def _lo_ResizeBilinear(self, l):
        v = self._in(l)
        if id(l) in self.bcast_resize:
            cat = self.bcast_resize[id(l)]
            self.bcast_src[id(self.concat_bufs[id(cat)])] = (v, v.C)
            self.views[id(l.output)] = None  # never materialised (Engine._bcast_input)
            return
        Ho, Wo = l.cfg["size"]
        buf, off = self._new_out(l, Ho, Wo, v.C)
        nonneg = v.act in (ACT_RELU, ACT_RELU6) or v.buf.nonneg
        if buf.ld != v.C:
            if not hasattr(buf, "nonneg_slices"):
                buf.nonneg_slices = {}
            buf.nonneg_slices[off] = nonneg
        else:
            buf.nonneg = nonneg
        self.units.append(ResizeUnit(self, v, View(buf, off, v.C), Ho, Wo))
        self.views[id(l.output)] = View(buf, off, v.C)

    def _lo_Dropout(self, l):
        v = self._in(l)
        if not (self.dropout and l.cfg["rate"] > 0):
            self.views[id(l.output)] = v
            return
        N_, H, W, C = v.shape
        buf = Buf(self, self.B, H, W, C, l.name)
        buf.nonneg = v.act in (ACT_RELU, ACT_RELU6)
        self.bufs.append(buf)
        self.units.append(MaterializeUnit(self, v, View(buf, 0, C), l.cfg["rate"], self.seed))
        self.views[id(l.output)] = View(buf, 0, C)

    def _lo_softmax(self, l, v):
        N_, H, W, C = v.shape[0], v.buf.H, v.buf.W, v.C
        if v.aff or v.act != ACT_NONE or v.off != 0 or v.ld != C:
            raise NotImplementedError("softmax expects materialised logits")
        self.logits_view = v
        # the head's form, decided here and nowhere else (head.py): the last launch only spreads materialised
        # low-resolution logits (resize) / the Subpixel convolution's contiguous output (phase shift) into v
        last = self.units[-1] if self.units else None
        form = "plain"
        if (last is not None and last.outv.buf is v.buf and not last.inv.aff and last.inv.act == ACT_NONE
                and last.inv.off == 0 and self.ops_fwd):
            if isinstance(last, ResizeUnit) and last.inv.ld == C and self.ops_fwd[-1][0] == "dl3_resize_bilinear_fwd":
                form = "bilinear"
            elif (isinstance(last, ShuffleUnit) and last.inv.ld == last.co * last.r * last.r
                  and self.ops_fwd[-1][0] == "dl3_phase_shift"):
                form = "shuffle"
        self.head = Head(self.B, v, form, last, self.ops_fwd[-1]) if form != "plain" else Head(self.B, v)
        # training: what the loss (and the mining front) reads.  A fused form drops its launch from the forward plan — the
        # full-resolution logits are never written; logits() runs it on demand
        self.loss_head = self._loss_head() if self.training else None
        if self.training and self.loss_head.op is not None:
            self.ops_fwd.pop()
        M = v.buf.M
        self.probs = self.empty(M * C)
        self.out_shape = (self.B,) + tuple(l.output.shape)
        if self.training:
            self._alloc_targets()
            self.nnz = self.zeros(4)
            if self.external_nnz:
                # data parallel: the loss kernel divides by a FIXED normaliser c0 (pixels per image: the same on every
                # rank, whatever the shard), the shard's count(w != 0) and its loss sum land in the arena's tail, the ONE
                # all-reduce of the step sums them with the gradients, and Adam finishes the scale c0 / count_all on the
                # device (dl3_adam_step_norm): no all-reduce in front of the step, no host round trip behind it
                self.nnz_host = float(M // self.B)
                self.nnz.fill_(self.nnz_host)
                self.loss = self.grads[self.tail + 1:self.tail + 2]
            else:
                self.loss = self.zeros(4)
            v.buf.expected += 1
        self.views[id(l.output)] = v

    def _alloc_targets(self):
        """labels / sample weights of the resident batch (set_targets)"""
        M = self.logits_view.buf.M
        self.labels, self.sweights = self.zeros(M), self.zeros(M)

    def _loss_head(self):
        """the training loss's admission rule: the fused kernels take at most 32 classes; the Subpixel one also reads its
        source as a plain contiguous tensor and writes that buffer's gradient itself — only with a single consumer and no
        BatchNorm on it, where its shape query accepts (DL3_FUSE_SHUFFLE=0: never)"""
        h = self.head
        ok = h.v.C <= 32
        if self.jaccard:
            # this loss's own rule (§16): its kernels hold a pixel's logits in registers and come in two forms — a
            # bilinear head is read as `bilinear`, everything else (the Subpixel head included) as `plain`
            if not ok:
                raise ValueError("the soft-Jaccard loss takes at most 32 classes, this head has %d" % h.v.C)
            return h if h.form == "bilinear" else h.plain
        if self.focal and not ok:   # (§18: the forms of the cross-entropy, no generic kernel above 32 classes)
            raise ValueError("the focal loss takes at most 32 classes, this head has %d" % h.v.C)
        if ok and h.form == "shuffle":
            ok = (os.environ.get("DL3_FUSE_SHUFFLE", "1") != "0" and h.src.buf.expected == 1 and not h.src.buf.bns
                  and self.lib.dl3_shuffle_xent_partials(*h.dims("loss")) > 0)
        return h if ok else h.plain

    # ------------------------------------------------------------------ backward lowering
    def _prune_gradients(self):
        """which buffers need a gradient at all: those computed from at least one TRAINABLE parameter.  With every layer
        trainable that is everything but the image; with the notebook's fine-tuning (json 147-155: `l.trainable = False`
        up to `concat_projection`) it is the tail only, and the backward pass below it — the whole backbone and the ASPP
        branches — is never lowered: no data gradient would reach a trainable weight through it (round 4; before, the
        frozen layers merely skipped their weight gradients).  DL3_PRUNE_BWD=0 restores that."""
        if os.environ.get("DL3_PRUNE_BWD", "1") == "0":
            return
        for b in self.bufs:
            b.requires_grad = False
        for u in self.units:   # forward order: producers before consumers
            ins = [w.buf for w in (getattr(u, "inv", None), getattr(u, "a", None), getattr(u, "b", None)) if w is not None]
            if getattr(u, "img_add", None) is not None:
                ins.append(u.img_add)
            own = False
            if isinstance(u, _ConvBase):
                names = [u.wname()] + ([u.bias] if getattr(u, "bias", None) else [])
                if u.bn is not None:
                    names += [u.bn.name + "/gamma:0", u.bn.name + "/beta:0"]
                own = any(self.trainable(n) for n in names)
            if own or any(b.requires_grad for b in ins):
                u.outv.buf.requires_grad = True   # (a Concatenate buffer: any of its producers)

    MINING_OPS = ("dl3_pixel_xent_plain", "dl3_pixel_xent_bilinear", "dl3_pixel_xent_shuffle", "dl3_topk_threshold",
                  "dl3_mine_weights")
    MINE_WS_COUNT = 4   # S_COUNT of the workspace enum in csrc/mine.hip: the kept pixels as an integer (32-bit words)

    def _lower_mining(self, M, C, count_dst):
        """the mining front of the loss kernel: v, (k, tau), (w', n').  -> the pointer the loss kernel takes as weights"""
        p, S = self.mining
        self.mine_v, self.mine_w = self.empty(M), self.zeros(M)
        self.mine_tau = self.zeros(4)
        self.mine_k = torch.zeros(4, dtype=torch.int32, device=self.device)
        nws = int(self.lib.dl3_topk_workspace_bytes(M))
        self.mine_ws = torch.zeros(nws // 4, dtype=torch.int32, device=self.device)
        self.op(self.ops_fwd, *self.loss_head.launch("pixel_xent", labels=ptr(self.labels), w=ptr(self.sweights),
                                               out=ptr(self.mine_v)))
        self.op(self.ops_fwd, "dl3_topk_threshold", ptr(self.mine_v), M, p, S, self.mine_step.data_ptr(),
                self.mine_ws.data_ptr(), nws, self.mine_k.data_ptr(), ptr(self.mine_tau))
        self.op(self.ops_fwd, "dl3_mine_weights", ptr(self.mine_v), ptr(self.sweights), ptr(self.mine_tau),
                self.mine_k.data_ptr(), ptr(self.mine_w), count_dst, self.mine_ws.data_ptr(), M)
        return ptr(self.mine_w)

    def mining_record(self):
        """(v, w', tau, k, n') of the last step, read back (test-facing): the per-pixel losses [B*H*W], the mined weights,
        the threshold, the number of pixels asked for and the number kept"""
        if not self.mining:
            raise ValueError("mining_record: this engine was lowered without mining")
        torch.cuda.current_stream().synchronize()
        ws = self.mine_ws.cpu().numpy()
        return (self.mine_v.cpu().numpy(), self.mine_w.cpu().numpy(), float(self.mine_tau[0].item()),
                int(self.mine_k[0].item()), int(ws[self.MINE_WS_COUNT]))

    FOCAL_OPS = ("dl3_focal_xent", "dl3_upsample_focal_xent", "dl3_upsample_focal_xent_fold", "dl3_shuffle_focal_xent")

    def _focal_args(self, C):
        """alpha and gamma of the focal loss launch: the class weights uploaded once (a scalar broadcast; None: a null
        pointer), gamma frozen in the launch"""
        gamma, alpha = self.focal
        self.focal_alpha = None
        if alpha is not None:
            if len(alpha) not in (1, C):
                raise ValueError("the focal loss got %d class weights for a head of %d classes" % (len(alpha), C))
            self.focal_alpha = self.zeros(C)
            self.focal_alpha.copy_(torch.tensor(np.broadcast_to(np.asarray(alpha, np.float32), (C,)).copy()))
        return dict(alpha=ptr(self.focal_alpha), gamma=gamma)

    JACCARD_OPS = ("dl3_jaccard_sums_plain", "dl3_jaccard_sums_bilinear", "dl3_jaccard_coef", "dl3_softmax_xent_jaccard",
                   "dl3_upsample_softmax_xent_jaccard")

    def _lower_jaccard(self, h, wsrc, g):
        """the loss launches of CE + lambda * L_J: per-image sums from the source the loss kernel reads, the coefficient
        table and lambda * L_J (an extra row of the loss partials, so that the one fold below returns the sum), then the
        loss kernel with the Jaccard half added to the full-resolution gradient g.  lambda is the only frozen value."""
        B, HW, C = h.sizes["images"]
        P = self.lib.dl3_jaccard_partials(B, HW)
        # doubles live in the float arena's buffers, two floats each (8-byte aligned: every allocation is)
        self.jac_part, self.jac_sums, self.jac_stats = self.zeros(2 * B * P * 3 * C), self.zeros(2 * B * C * 3), self.zeros(8)
        self.jac_coef = self.zeros(B * C * 2)
        self.lossP = self.lib.dl3_jaccard_loss_partials(B, HW)
        self.loss_part = self.zeros(self.lossP + 1)
        self.op(self.ops_fwd, *h.launch("jaccard_sums", labels=ptr(self.labels), w=ptr(self.sweights),
                                  out=ptr(self.jac_part)))
        self.op(self.ops_fwd, "dl3_jaccard_coef", ptr(self.jac_part), P, B, C, self.jaccard, ptr(self.jac_sums),
                ptr(self.jac_coef), ptr(self.jac_stats), ptr(self.loss_part, self.lossP))
        self.op(self.ops_fwd, *h.launch("jaccard_loss", labels=ptr(self.labels), w=wsrc, nnz=ptr(self.nnz),
                                  coef=ptr(self.jac_coef), lam=self.jaccard, grad=ptr(g), part=ptr(self.loss_part)))
        self.op(self.ops_fwd, "dl3_reduce_partials", ptr(self.loss_part), self.lossP + 1, 1, ptr(self.loss))

    def jaccard_record(self):
        """(sums [B,C,3] float64 (I, S, Y), coef [B,C,2] float32 (A, Bc), L_J, cross-entropy) of the last step, read back
        (test-facing); the cross-entropy is the loss partials' own sum, the step's loss is it plus lambda * L_J"""
        if not self.jaccard:
            raise ValueError("jaccard_record: this engine was lowered without the soft-Jaccard loss")
        torch.cuda.current_stream().synchronize()
        B, HW, C = self.loss_head.sizes["images"]
        part = self.loss_part.cpu().numpy()
        return (self.jac_sums.view(torch.float64).cpu().numpy().reshape(B, C, 3),
                self.jac_coef.cpu().numpy().reshape(B, C, 2), float(self.jac_stats.view(torch.float64)[0].item()),
                float(part[:self.lossP].astype(np.float64).sum()))

    def _lower_backward(self):
        self._prune_gradients()
        v = self.logits_view
        buf = v.buf
        M, C = buf.M, v.C
        # loss + dlogits (first and only contribution to the logits buffer)
        count_dst = (self.grads.data_ptr() + 4 * self.tail) if self.external_nnz else ptr(self.nnz)
        if self.mining:
            # three launches in place of the count: per-pixel losses v from the source the loss kernel below reads, k
            # and the k-th largest v, then the mined weights w' and their count n' where count(w != 0) goes today
            wsrc = self._lower_mining(M, C, count_dst)
        else:
            self.op(self.ops_fwd, "dl3_count_nonzero", ptr(self.sweights), M, count_dst)
            wsrc = ptr(self.sweights)
        h = self.loss_head
        # the full-resolution gradient never exists where a row of it fits the LDS: the loss kernel folds each output row
        # onto the low-resolution columns, the resize unit's backward folds the rows
        # (the focal kernel keeps alpha, 32 floats, beside the row)
        fold = h.form == "bilinear" and self.fold_tail and (
            ((buf.W + 2 * h.src.buf.W) * C + 2 * buf.W) * 4 + (128 if self.focal else 0) <= 65536)
        if self.jaccard:
            # the full-resolution gradient in the logits buffer, whatever the head: the resize unit's ordinary backward
            # (the phase shift's) takes it from there — no folded, no shuffle-fused form of this loss
            buf.grad = g = self.empty(M * buf.ld)
            self._lower_jaccard(h, wsrc, g)
        elif h.form == "shuffle":     # the gradient of the Subpixel convolution's output, in its unshuffled layout
            h.src.buf.grad = g = self.empty(h.src.buf.M * h.src.buf.ld)
            self.lossP = self.lib.dl3_shuffle_xent_partials(*h.dims("loss"))
        elif fold:
            h.folded = g = self.empty(self.B * buf.H * h.src.buf.W * C)
            self.lossP = self.lib.dl3_xent_fold_partials(self.B, buf.H)
        else:
            buf.grad = g = self.empty(M * buf.ld)
            self.lossP = self.lib.dl3_rows_partials(M)
        if not self.jaccard:
            self.loss_part = self.zeros(self.lossP)
            # the focal loss: the same form, grid and partials, its own entry point with alpha and gamma on top
            family, extra = ("focal_loss", self._focal_args(C)) if self.focal else ("loss", {})
            self.op(self.ops_fwd, *h.launch(family, fold, labels=ptr(self.labels), w=wsrc, nnz=ptr(self.nnz), grad=ptr(g),
                                      part=ptr(self.loss_part), **extra))
            self.op(self.ops_fwd, "dl3_reduce_partials", ptr(self.loss_part), self.lossP, 1, ptr(self.loss))
        buf.done = 1
        assert buf.expected == 1
        # weight transposes for bwd-data, then the units in reverse
        self._transposes = []
        first_bwd = len(self.ops_bwd)
        # one buffer holds the materialised dY of whichever 1x1 convolution is being differentiated (written by its
        # weight-gradient launch, read by its bwd-data launch right behind it on the same stream)
        n = max([u.M * u.N for u in self.units if isinstance(u, PwUnit) and u.dy_mat_ok()] or [0])
        if n:
            self.dy_buf = self.empty(n)
        for u in reversed(self.units):
            if u.outv.buf.requires_grad:   # (else: no trainable parameter at or above this unit)
                u.bwd()
        if self._transposes:
            # every W -> WT of the backward pass in ONE launch at its start (54 tiny launches otherwise)
            rows, t0 = [], 0
            for src, dst, r, c in self._transposes:
                tx = (c + 31) // 32
                rows.append([src, dst.data_ptr(), r, c, t0, tx])
                t0 += tx * ((r + 31) // 32)
            self._tdesc = torch.tensor(rows, dtype=torch.int64, device=self.device)
            self._keep.append(self._tdesc)
            self.ops_bwd.insert(first_bwd, self.op([], "dl3_transpose_batched", self._tdesc.data_ptr(), len(rows), t0))
        if self._folds:
            # (the slabs were written by launches on either stream: the fold sits behind the join at the end of the list)
            rows, b0 = [], 0
            for src, dst, P, n in self._folds:
                rows.append([src, dst, P, n, b0])
                b0 += self.lib.dl3_reduce_partials_blocks(P, n)
            self._fdesc = torch.tensor(rows, dtype=torch.int64, device=self.device)
            self._keep.append(self._fdesc)
            rec = self.op(self.ops_bwd, "dl3_reduce_partials_batched", self._fdesc.data_ptr(), len(rows), b0)
            if self.fork:
                self._join_before.add(id(rec))
        if self.fork_pairs:
            self._pair_wgrads_with_depthwise()
        self._check_dy_adjacency()
        assert not self.prestat, "BatchNorm-backward sums reduced early but never folded"
        for b in self.bufs:
            if b.requires_grad and b.expected and b.done != b.expected:
                raise RuntimeError("gradient accounting broken for buffer %s (%d/%d)" % (b.name, b.done, b.expected))

    def _check_dy_adjacency(self):
        """ONE buffer holds the materialised dY of whichever 1x1 convolution is being differentiated: between the launch
        that writes it (dl3_pwconv_bwd_weight_dy) and the layer's bwd-data launch that reads it, no other launch may write
        it — i.e. no second dl3_pwconv_bwd_weight_dy — and both must sit on the same stream (any future
        reordering of ops_bwd would otherwise corrupt gradients silently)"""
        if self.dy_buf is None:
            return
        dy = ptr(self.dy_buf)
        pending = None
        for rec in self.ops_bwd:
            if rec[0] == "dl3_pwconv_bwd_weight_dy":
                assert pending is None, "two dY writers without the first one's reader in between"
                assert rec.arg("dy_out") == dy and id(rec) not in self._side, "dY written off the main stream / into another buffer"
                pending = [rec.arg(k) for k in "MKN"]
            elif rec[0] == "dl3_pwconv_bwd_data" and rec.arg("g") == dy:
                assert pending == [rec.arg(k) for k in "MKN"], ("bwd-data reads a dY another layer wrote", pending)
                pending = None
        assert pending is None, "a materialised dY was never read"

    def _pair_wgrads_with_depthwise(self):
        """DL3_FORK=2: every depthwise backward launch takes the nearest earlier 1x1 weight gradient with it (moved to just
        in front of it, on the side stream); every other weight gradient stays in the chain; the next 1x1 GEMM of the chain
        waits for the side stream."""
        ops = self.ops_bwd
        side_all = [r for r in ops if id(r) in self._side]
        paired = set()
        j = 0
        while j < len(ops):
            if ops[j][0] == "dl3_dwconv3x3_bwd":
                i = j - 1
                while i >= 0 and not (ops[i][0] == "dl3_pwconv_bwd_weight" and id(ops[i]) in self._side and id(ops[i]) not in paired):
                    if ops[i][0] == "dl3_dwconv3x3_bwd":
                        i = -1
                        break
                    i -= 1
                if i >= 0:
                    rec = ops.pop(i)
                    ops.insert(j - 1, rec)   # directly in front of the depthwise launch (behind it measured no gain at all)
                    paired.add(id(rec))
            j += 1
        for p, rec in enumerate(ops):
            if id(rec) in paired:
                k = p + 1
                while k < len(ops) and (id(ops[k]) in paired or not ops[k][0].startswith("dl3_pwconv_")):
                    k += 1
                if k < len(ops):
                    self._join_before.add(id(ops[k]))
        for r in side_all:
            if id(r) not in paired:
                self._side.discard(id(r))

    # ---- gradient contribution protocol ---------------------------------------------
    def contrib_kernel(self, buf):
        """A kernel is about to write its contribution into buf.grad.  Returns (gout, add, last)."""
        add = None
        if buf.grad is None:
            buf.grad = self.empty(buf.M * buf.ld)
            if buf.addend is not None:
                add, buf.addend = buf.addend, None
        else:
            add = buf.grad
        buf.done += 1
        return buf.grad, add, buf.done == buf.expected

    def finish_bn_bwd(self, buf, dpart, P, ldc):
        """after the last contribution: fold the BN-backward partials of every BN living in this buffer"""
        for bn, off, C in buf.bns:
            n = bn.name
            self.op(self.ops_bwd, "dl3_bn_bwd_finalize", dpart.data_ptr() + 4 * 2 * off, P, ldc, C, float(buf.M),
                    self.wptr(n + "/gamma:0"), buf.vptr(V_MEAN, off), buf.vptr(V_INVSTD, off),
                    1 if self.bn_batch else 0, buf.vptr(V_CA, off), buf.vptr(V_CB, off), buf.vptr(V_CC, off),
                    self.gptr(n + "/gamma:0"), self.gptr(n + "/beta:0"))

    def contrib_elementwise(self, buf, view, gin, ldgin, gin_div=1, gin_scale=1.0, drop=(0.0, 0)):
        """contribution through dl3_grad_finish: gout = mask_view(gin) + existing; handles stats when last"""
        if view.off != 0 or view.C != buf.ld:
            raise NotImplementedError("element-wise gradient into a channel slice")
        k = GradSink(self, view, self.lib.dl3_rows_partials(buf.M))
        self.op(self.ops_bwd, "dl3_grad_finish", gin, ldgin, gin_div, gin_scale, k.out, buf.ld, k.add, buf.ld, k.x, buf.ld,
                k.scale, k.shift, view.act, k.mean, k.invstd, ptr(k.dpart), buf.M, buf.ld, drop[0], drop[1],
                self.drop_step.data_ptr() if drop[0] > 0 else None)
        k.finish()

    def contrib_passthrough(self, buf, view, g):
        """Add backward: the gradient tensor g (same [M, C] shape, ld == C) flows unchanged into buf"""
        if not buf.requires_grad:
            return
        if view.act != ACT_NONE or view.off != 0 or view.C != buf.ld or g.numel() != buf.M * buf.ld:
            return self.contrib_elementwise(buf, view, ptr(g), view.C)
        if buf.grad is None and buf.addend is None and buf.done == 0:
            buf.done += 1
            if buf.expected == 1:
                buf.grad = g  # alias
                if buf.bns and id(buf) in self.prestat:
                    # the kernel that completed g already reduced sum(g), sum(g * x_hat) of THIS BatchNorm in its epilogue
                    dpart, P, ld = self.prestat.pop(id(buf))
                    self.finish_bn_bwd(buf, dpart, P, ld)
                elif buf.bns:
                    P = self.lib.dl3_rows_partials(buf.M)
                    dpart = self.empty(P * buf.ld * 2)
                    self.op(self.ops_bwd, "dl3_grad_finish", ptr(g), buf.ld, 1, 1.0, ptr(g), buf.ld, None, 0,
                            ptr(buf.t), buf.ld, None, None, ACT_NONE, buf.vptr(V_MEAN), buf.vptr(V_INVSTD),
                            ptr(dpart), buf.M, buf.ld, 0.0, 0, None)
                    self.finish_bn_bwd(buf, dpart, P, buf.ld)
            else:
                buf.addend = g
            return
        self.contrib_elementwise(buf, view, ptr(g), buf.ld)

    def alias_stats_target(self, ibuf):
        """ibuf is the output of a residual Add whose gradient is about to be completed by a GEMM epilogue.  The Add's
        backward hands that very tensor on, unchanged, to its inputs; for an input that is a BatchNorm'ed convolution
        output with no other consumer (the project conv of the block, deeplabv3p.py:194-201) the BatchNorm-backward sums
        over the gradient can be reduced right there instead of by a separate dl3_grad_finish pass over g and y
        (round 3).  Returns that input's Buf or None."""
        add = self.add_of_buf.get(id(ibuf))
        if add is None:
            return None
        hits = [v for v in (add.a, add.b)
                if v.buf.requires_grad and v.buf.bns and v.buf.expected == 1 and v.buf.done == 0 and v.buf.grad is None
                and v.buf.addend is None and v.act == ACT_NONE and v.off == 0 and v.C == v.buf.ld == ibuf.ld
                and v.buf.M == ibuf.M and len(v.buf.bns) == 1 and v.buf.bns[0][1] == 0 and v.buf.bns[0][2] == v.buf.ld]
        return hits[0].buf if len(hits) == 1 else None

    def grad_operand(self, out_view):
        """(g, ldg, yraw, ldy, cA, cB, cC) of a conv whose output is out_view"""
        buf = out_view.buf
        g = buf.grad.data_ptr() + 4 * out_view.off
        has_bn = any(off == out_view.off for _, off, _ in buf.bns)
        if has_bn:
            return (g, buf.ld, out_view.p(), buf.ld, buf.vptr(V_CA, out_view.off), buf.vptr(V_CB, out_view.off),
                    buf.vptr(V_CC, out_view.off))
        return (g, buf.ld, None, 0, None, None, None)

    # ------------------------------------------------------------------ running
    def _prep(self):
        if self.dirty:
            self.run_ops(self.ops_prep)
            self.dirty = False

    def set_input(self, x):
        """raw 0-255 pixels [B,H,W,3]: float32 (the reference's arrays), or uint8 (decoded images as they come from
        cv2.imread) — those cross PCIe as bytes and are widened on the device"""
        self.xbuf.t.copy_(pixels_to_device(x, self.device, non_blocking=True).reshape(-1))

    @property
    def graph(self):
        """the captured hipGraph of the main plan; None until its second call has captured it"""
        return self._main.graph

    def _run_main(self):
        self.run_ops(self.ops_fwd)
        if self.training:
            self._run_bwd()

    def forward(self):
        """forward launch sequence; the inference engine replays it as one hipGraph from the second call on (68
        launches of a few microseconds each: at batch 1 the Python/ctypes launch path costs more than the kernels).
        A training engine's plan is the whole step (fwd_bwd): its forward() stays eager and does not count as a call"""
        self._prep()
        if self.training:
            self.run_ops(self.ops_fwd)
        else:
            self._main.run()

    def probs_device(self):
        """forward() on the resident input, then the head's softmax: probabilities [B,H,W,C] on the device, a view of
        self.probs (valid until the next call)"""
        self.forward()
        v = self.logits_view
        capi.call("dl3_softmax_fwd", ptr(v.buf.t), ptr(self.probs), v.buf.M, v.C, capi.stream())
        return self.probs.view(self.B, v.buf.H, v.buf.W, v.C)

    def predict(self, x):
        assert not self.training
        self.set_input(x)
        return self.probs_device().cpu().numpy().reshape(self.out_shape)

    def logits(self):
        v = self.logits_view
        if self.training and self.loss_head.op is not None:
            self.run_ops([self.loss_head.op])  # a fused training tail never materialises them
        return v.buf.t.cpu().numpy().reshape(self.B, v.buf.H, v.buf.W, v.C)

    def argmax(self, host=True):
        """int32 masks [B,H,W]: a numpy array, or with host=False the device tensor"""
        v = self.logits_view
        out = argmax_rows(v.buf.t, v.buf.M, v.C).reshape(self.B, v.buf.H, v.buf.W)
        return out.cpu().numpy() if host else out

    def set_targets(self, y, sw=None, fill_weights=True):
        """labels [B,HW,1] (void = classes) and temporal sample weights [B,HW]; numpy arrays or device tensors (e.g. the
        output of utils.prepare_targets, which then never leaves the GPU).  On an inference engine the buffers belong to
        the evaluation plan (evaluate_batch), whose tail takes `no weights` as a NULL pointer (fill_weights=False)."""
        M = self.logits_view.buf.M
        if not self.training:
            self._eval_setup()
        yt = flat_f32(y, self.device, non_blocking=True)
        assert yt.numel() == M, (yt.numel(), M)
        self.labels.copy_(yt)
        if sw is not None:
            self.sweights.copy_(flat_f32(sw, self.device, non_blocking=True))
        elif fill_weights:
            # Keras without sample weights: plain mean over all B*HW pixels; void rows contribute zero loss and zero
            # gradient through the one-hot (utils.py:129), not through a weight
            capi.call("dl3_fill", ptr(self.sweights), 1.0, M, capi.stream())

    def count_nnz(self):
        """count(w != 0) of the resident sample weights (device count, one scalar read back)"""
        tmp = torch.zeros(4, dtype=torch.float32, device=self.device)
        capi.call("dl3_count_nonzero", ptr(self.sweights), self.logits_view.buf.M, ptr(tmp),
                  torch.cuda.current_stream().cuda_stream)
        return float(tmp[0].item())

    def set_nnz(self, value):
        """external_nnz engines: the FIXED normaliser the loss kernel divides by (default: pixels per image); the
        optimizer multiplies it back and divides by the global count (train_step).  Tests use it to give engines of
        different batch sizes one common normaliser."""
        assert self.external_nnz
        self.nnz_host = float(value)
        capi.call("dl3_fill", ptr(self.nnz), float(value), 1, torch.cuda.current_stream().cuda_stream)

    def loss_value(self):
        """the loss of the last step as a float (one device read): sum(l*w) / count(w != 0) — over the GLOBAL batch on a
        data-parallel engine, from the arena tail the all-reduce summed.  On an engine with L2 regularisers plus the penalty
        the last l2_penalty() call wrote — the weights train_step started from; zero before the first call, and not
        refreshed by fwd_bwd() alone — read in the same copy (the floats widen exactly) and added in double"""
        t = self.grads[self.tail:self.tail + 2] if self.external_nnz else self.loss[0:1]
        if self.l2:
            t = torch.cat([t.double(), self._l2["out"]])
        t = t.cpu()
        data = float(t[1]) * self.nnz_host / max(float(t[0]), 1e-20) if self.external_nnz else float(t[0])
        return data + self._l2_sum(t[-4:]) if self.l2 else data

    def loss_handle(self):
        """the same without the read: a LazyLoss that fetches when (if) somebody looks at it (the penalty: that of the last
        l2_penalty() call, cloned like the loss)"""
        pen = self._l2["out"].clone() if self.l2 else None
        if not self.external_nnz:
            return LazyLoss(self.loss[0:1].clone(), None, 1.0, pen)
        t = self.grads[self.tail:self.tail + 2].clone()
        return LazyLoss(t[1:2], t[0:1], self.nnz_host, pen)

    def seg_counts(self, y):
        """after forward(): per-image, per-class pixel counts [B,3,C] of the argmax mask against labels y
        (dl3_argmax + dl3_seg_counts on the device; utils.Jaccard_from_counts turns them into the metric)"""
        v = self.logits_view
        pred = argmax_rows(v.buf.t, v.buf.M, v.C)
        yt = flat_f32(y, self.device)
        assert yt.numel() == v.buf.M, (yt.numel(), v.buf.M)
        counts = torch.empty(self.B, 3, v.C, dtype=torch.int32, device=self.device)
        capi.call("dl3_seg_counts", pred.data_ptr(), yt.data_ptr(), self.B, v.buf.M // self.B, v.C, counts.data_ptr(),
                  capi.stream())
        return counts.cpu().numpy()

    # ------------------------------------------------------------------ evaluation plan
    def _eval_setup(self):
        """the evaluation plan of an inference engine: the forward op list minus the final resize / phase-shift launch
        (`ops_fwd` itself stays as it is: predict / logits() / argmax() keep using it) plus the evaluation tail
        (dl3_eval_tail_*), which turns the low-resolution logits and the labels into loss sums, counts, confusion matrix
        and mask — neither full-resolution logits nor probabilities are written.  Any other graph (and C > 32) keeps its
        whole forward plan and ends in the plain form on the materialised logits."""
        ev = getattr(self, "_eval", None)
        if ev is not None:
            return ev
        if self.training:
            raise RuntimeError("Engine.evaluate_batch needs an inference engine (training=False)")
        M, C, B = self.logits_view.buf.M, self.logits_view.C, self.B

        def partials(h):
            return getattr(self.lib, h.entry("eval_tail")[0] + "_partials")(*h.dims("eval_tail"))
        # the evaluation tail's admission rule: the fused kernel's own limits (C <= 32, LDS staging) — its *_partials
        # query answers 0 for a shape it refuses
        h = self.head if partials(self.head) > 0 else self.head.plain
        P = partials(h)
        if P <= 0:
            raise capi.DL3Error("dl3_eval_tail_plain does not support %d classes" % C)
        # labels / weights of the batch (set_targets), the tail's own buffers and ONE record of its results:
        # loss_sum double[B] | nnz int32[B] | counts int32[B][3][C]
        self._alloc_targets()
        rec_bytes = (8 * B + 4 * B + 4 * B * 3 * C + 15) // 16 * 16
        self._eval = ev = types.SimpleNamespace(
            head=h, plans={}, n=0, rec_bytes=rec_bytes, part=self.empty(2 * B * P),
            mask=torch.empty(M, dtype=torch.int32, device=self.device),
            rec=torch.zeros(rec_bytes, dtype=torch.uint8, device=self.device),
            results=torch.zeros(8, rec_bytes, dtype=torch.uint8, device=self.device))
        return ev

    def _ops_before(self, h):
        """the forward op list in front of a kernel that reads head h: without the launch that materialises the
        full-resolution logits where h is a fused form (`ops_fwd` itself stays as it is)"""
        return self.ops_fwd[:-1] if h.op is not None else list(self.ops_fwd)

    def eval_op_names(self, confusion=None, mask=False):
        """the launch names of the evaluation plan (tests: no final resize / phase shift / softmax in it)"""
        return [rec[0] for rec in self._eval_plan(confusion, True, mask)[1]]

    def _eval_plan(self, confusion, weighted, mask):
        """(Plan, launch list) of one (confusion pointer, weighted, mask) variant"""
        ev = self._eval_setup()
        key = (0 if confusion is None else confusion.data_ptr(), bool(weighted), bool(mask))
        if key not in ev.plans:
            B, C = self.B, self.logits_view.C
            if confusion is not None and (confusion.dtype != torch.int64 or confusion.numel() != C * C
                                          or not confusion.is_contiguous() or confusion.device != self.device):
                raise ValueError("confusion must be a contiguous int64 [%d,%d] tensor on %s" % (C, C, self.device))
            base = ev.rec.data_ptr()
            ops = self._ops_before(ev.head)
            self.op(ops, *ev.head.launch(
                "eval_tail", labels=ptr(self.labels), w=ptr(self.sweights) if weighted else None, part=ptr(ev.part),
                loss=base, nnz=base + 8 * B, counts=base + 12 * B, confusion=None if confusion is None else confusion.data_ptr(),
                mask=ev.mask.data_ptr() if mask else None))
            # (confusion rides along so that the tensor behind the captured pointer stays alive)
            ev.plans[key] = (Plan(self, lambda: self.run_ops(ops)), ops, confusion)
        return ev.plans[key][:2]

    def evaluate_batch(self, x, y, sw=None, confusion=None, mask=False):
        """forward + evaluation tail on (x, y, sw), everything on the device: the batch's loss sums, count(w != 0) and
        dl3_seg_counts' counts land in the next record of a device buffer that `read_evaluation()` fetches ONCE per pass.
        confusion: a contiguous int64 [C,C] device tensor the batch is ADDED to (the caller zeroes it); mask=True returns
        the int32 masks [B,H,W] as a device tensor (valid until the next call).  Each (confusion, weighted, mask) variant
        is replayed as a hipGraph of its own from its second call on.
        The host waits for the stream to drain before it enqueues (the trap recorded in train_step: a graph replay
        behind a pageable device-to-host copy)."""
        plan, _ = self._eval_plan(confusion, sw is not None, mask)
        ev = self._eval
        torch.cuda.current_stream().synchronize()
        self.set_input(x)
        self.set_targets(y, sw, fill_weights=False)
        self._prep()
        plan.run()
        if ev.n == ev.results.shape[0]:
            grown = torch.zeros(2 * ev.n, ev.rec_bytes, dtype=torch.uint8, device=self.device)
            grown[:ev.n].copy_(ev.results)
            ev.results = grown
        ev.results[ev.n].copy_(ev.rec)
        ev.n += 1
        if mask:
            v = self.logits_view
            return ev.mask.reshape(self.B, v.buf.H, v.buf.W)
        return None

    def discard_evaluation(self):
        """forget the records written since the last read_evaluation() (a pass that starts over)"""
        self._eval_setup().n = 0

    def read_evaluation(self):
        """the records written since the last read, in ONE device-to-host copy behind a host-side stream synchronisation:
        (loss_sum [n,B] float64, nnz [n,B] int32, counts [n,B,3,C] int32); the record counter starts over"""
        ev = self._eval_setup()
        n, B, C = ev.n, self.B, self.logits_view.C
        torch.cuda.current_stream().synchronize()
        raw = ev.results[:n].cpu().numpy() if n else np.zeros((0, ev.rec_bytes), np.uint8)
        ev.n = 0
        loss = np.ascontiguousarray(raw[:, :8 * B]).view(np.float64).reshape(n, B)
        nnz = np.ascontiguousarray(raw[:, 8 * B:12 * B]).view(np.int32).reshape(n, B)
        counts = np.ascontiguousarray(raw[:, 12 * B:12 * B + 12 * B * C]).view(np.int32).reshape(n, B, 3, C)
        return loss, nnz, counts

    # ------------------------------------------------------------------ CRF unary plan (softmax unary)
    def _crf_ops(self, U_ptr, scale, clip, form=None):
        """the plan behind crf_unary: like the evaluation plan, the forward op list minus the final resize / phase-shift
        launch where that launch only spreads materialised low-resolution logits, ending in dl3_crf_unary_bilinear /
        _shuffle on those; any other graph — or form="plain" — keeps its whole forward plan and ends in dl3_crf_unary_plain
        on the head's logits.  No softmax launch either way, and no admission rule: the kernels take every shape."""
        if self.training:
            raise RuntimeError("Engine.crf_unary needs an inference engine (training=False)")
        if form not in (None, "plain", self.head.form):
            raise ValueError("this head has no %r form (it is %r)" % (form, self.head.form))
        h = self.head.plain if form == "plain" else self.head
        ops = self._ops_before(h)
        self.op(ops, *h.launch("crf_unary", U=U_ptr, scale=0.0 if scale is None else float(scale),
                               clip=0.0 if clip is None else float(clip)))
        return ops

    def crf_unary_op_names(self, form=None):
        """the launch names of the CRF unary plan (tests: which form, and no final resize / phase shift / softmax)"""
        return [rec[0] for rec in self._crf_ops(None, None, 1e-5, form)]

    def crf_unary(self, U=None, scale=None, clip=1e-5, form=None):
        """forward pass on the resident input (set_input) straight into the dense CRF's unary energies: U [B,C,N] float32
        on the device (allocated when not given), unary_from_softmax(softmax(logits), scale, clip) of the full-resolution
        logits — which, like the probabilities, are not written where the head ends in a resize or a phase shift."""
        C, N = self.logits_view.C, self.logits_view.buf.M // self.B
        if U is None:
            U = torch.empty(self.B, C, N, dtype=torch.float32, device=self.device)
        elif (not torch.is_tensor(U) or U.dtype != torch.float32 or tuple(U.shape) != (self.B, C, N)
              or not U.is_contiguous() or U.device != self.device):
            raise ValueError("U must be a contiguous float32 [%d,%d,%d] tensor on %s" % (self.B, C, N, self.device))
        self._prep()
        self.run_ops(self._crf_ops(U.data_ptr(), scale, clip, form))
        return U

    def crf_mask(self, images, scale=None, clip=1e-5):
        """crf_unary + dl3_crf_inference (utils.CRF_PARAMS) with `images` [B,H,W,3] as the CRF's image: the MAP class ids,
        int32 [B,H,W] on the device.  A single-class model has nothing to infer."""
        from . import crf
        from .utils import CRF_PARAMS
        v = self.logits_view
        if v.C > crf.MAX_LABELS:
            raise capi.DL3Error("crf_mask: %d classes; the device kernels take at most %d labels" % (v.C, crf.MAX_LABELS))
        if v.C == 1:
            return torch.zeros(self.B, v.buf.H, v.buf.W, dtype=torch.int32, device=self.device)
        im = crf.images_u8(images, self.device)
        if tuple(im.shape) != (self.B, v.buf.H, v.buf.W, 3):
            raise ValueError("images must be [%d,%d,%d,3], got %r" % (self.B, v.buf.H, v.buf.W, tuple(im.shape)))
        MAP, _, _ = crf.inference(im, self.crf_unary(None, scale, clip), CRF_PARAMS["iterations"])
        return MAP.reshape(self.B, v.buf.H, v.buf.W)

    def fwd_bwd(self):
        """forward + loss + backward on the resident batch (the benchmarked hot path): the main plan"""
        self._prep()
        self._main.run()

    def _run_bwd(self):
        if self.fork and self._side:
            self.run_ops_forked(self.ops_bwd)
        else:
            self.run_ops(self.ops_bwd)

    _RULES = {
        "adam": (capi.OPT_ADAM, dict(lr=7e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=1e-6)),   # the notebook's values
        "sgd": (capi.OPT_SGD, dict(lr=0.01, momentum=0.0, decay=0.0, nesterov=False)),
        "rmsprop": (capi.OPT_RMSPROP, dict(lr=0.001, rho=0.9, epsilon=1e-7, decay=0.0)),
    }

    def opt_step(self, opt=None, grad_scale=1.0, norm=None):
        """one optimizer step over the parameter arena.  opt: the compiled description dict(rule='adam' | 'sgd' |
        'rmsprop', hyper={...}, clipnorm=, clipvalue=) (graph.Model._opt_desc), or — Engine.adam's argument — the plain
        Adam hyper-parameter dict / None.  [TF-semantics: Keras 2.2.4 get_updates, from memory] lr = lr / (1 + decay * it)
        with `it` the iteration count BEFORE the increment; Adam folds the bias correction sqrt(1-b2^t)/(1-b1^t), t = it + 1,
        into lr_t.  An unclipped Adam is dl3_adam_step / dl3_adam_step_norm; every other case is dl3_opt_step, with
        dl3_grad_sumsq in front of it when clipnorm is set (the global norm stays on the device).
        norm (the default on data-parallel / external_nnz engines, and the only valid choice there): the gradient scale is
        finished on the device, normaliser / count_all from the arena tail; grad_scale is ignored.
        An external_nnz engine's loss kernel divides by the FIXED c0, so a step with a host scale and without norm would
        silently apply grad * scale / c0 instead of grad / count_all: refused."""
        if norm is None:
            norm = self.external_nnz
        if self.external_nnz and not norm:
            raise ValueError("Engine.adam(norm=False) on an external_nnz (data-parallel) engine: its gradients are "
                             "normalised by a fixed constant and must be finished by dl3_adam_step_norm")
        if not (opt and "rule" in opt):
            opt = dict(rule="adam", hyper=opt)
        rule = opt["rule"]
        if rule not in self._RULES:
            raise ValueError("Engine.opt_step: unknown rule %r (known: %s)" % (rule, sorted(self._RULES)))
        rid, defaults = self._RULES[rule]
        o = dict(defaults)
        o.update(opt.get("hyper") or {})
        clipnorm, clipvalue = float(opt.get("clipnorm") or 0.0), float(opt.get("clipvalue") or 0.0)
        it = self.iteration
        t = it + 1
        lr_t = o["lr"] / (1.0 + o["decay"] * it)
        if rule == "adam":
            lr_t = lr_t * math.sqrt(1.0 - o["beta_2"] ** t) / (1.0 - o["beta_1"] ** t)
        if norm:
            assert self.external_nnz
            grad_scale, denom = self.nnz_host, self.grads.data_ptr() + 4 * self.tail
        else:
            denom = None
        stream = torch.cuda.current_stream().cuda_stream
        if rule == "adam" and not clipnorm and not clipvalue:
            if norm:
                capi.call("dl3_adam_step_norm", ptr(self.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                          self.n_param, lr_t, o["beta_1"], o["beta_2"], o["epsilon"], grad_scale, denom, stream)
            else:
                capi.call("dl3_adam_step", ptr(self.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                          self.n_param, lr_t, o["beta_1"], o["beta_2"], o["epsilon"], grad_scale, stream)
        else:
            if clipnorm:
                # the norm of what the optimizer updates: [0, n_param) — the arena's padding holds exact zeros
                capi.call("dl3_grad_sumsq", ptr(self.grads), self.n_param, self.grad_sumsq.data_ptr(),
                          self.sumsq_ws.data_ptr(), self.sumsq_ws.numel() * 8, stream)
            c0, c1 = {"adam": (o.get("beta_1"), o.get("beta_2")), "sgd": (o.get("momentum"), 0.0),
                      "rmsprop": (o.get("rho"), 0.0)}[rule]
            h = capi.OptHyper(lr_t, c0, c1, o.get("epsilon", 0.0), grad_scale, clipnorm, clipvalue,
                              int(bool(o.get("nesterov", False))))
            capi.call("dl3_opt_step", ptr(self.params), ptr(self.grads), ptr(self.adam_m),
                      ptr(self.adam_v) if rule == "adam" else None, self.n_param, rid, ctypes.byref(h), denom,
                      self.grad_sumsq.data_ptr() if clipnorm else None, stream)
        self.iteration += 1
        self.dirty = True

    def adam(self, opt=None, grad_scale=1.0, norm=None):
        """Keras Adam with decay (notebook cell 2): lr_t = lr/(1+decay*it) * sqrt(1-b2^t)/(1-b1^t); opt_step with the
        plain hyper-parameter dict (None: the notebook's values)"""
        self.opt_step(opt, grad_scale, norm)

    def adopt_optimizer_state(self, other):
        """continue another training engine's optimizer (same model, other batch size): Adam moments, iteration count
        and the dropout step move device-to-device; the flat layouts are identical by construction"""
        if other is self or not (self.training and other.training):
            return
        if other.adam_m.numel() != self.adam_m.numel() or other.n_param != self.n_param:
            raise RuntimeError("optimizer state layouts differ (engines of two different compile() calls?)")
        self.adam_m.copy_(other.adam_m)
        self.adam_v.copy_(other.adam_v)
        self.drop_step.copy_(other.drop_step)
        # the mining ramp continues with the optimizer's clock (an engine lowered without mining did not count its steps)
        if other.mining:
            self.mine_step.copy_(other.mine_step)
        else:
            self.mine_step.fill_(int(other.iteration))
        self.iteration = other.iteration

    def train_step(self, x, y, sw=None, opt=None, comm=None, lazy=False):
        """one step on (x, y, sw).  Data parallel (external_nnz): ONE loss over the global batch,
        L = sum_all(l*w) / count_all(w != 0) — every rank differentiates sum_shard(l*w) / c0, the all-reduce sums
        gradients, counts and loss sums, Adam applies c0 / count_all on the device: nothing in front of the captured
        step, one collective behind it, no host read.  lazy: the loss comes back as a LazyLoss (no device read).
        The host waits for the stream to drain before it enqueues the step: a replay of the captured step enqueued
        behind a pageable device-to-host copy of ~100 KB or more (any `.cpu()` / `.numpy()` read-back between two steps)
        computed a wrong step on the MI355X runtime (tests/test_gpu_augment.py::test_host_read_back_between_steps); an
        event wait on the stream did not help, a host-side stream synchronisation does.  The next batch is prepared on
        the host before this call, so that work still overlaps the previous step."""
        torch.cuda.current_stream().synchronize()
        self.set_input(x)
        self.set_targets(y, sw)
        self.fwd_bwd()
        if self.external_nnz:
            if comm is not None:
                comm.allreduce_grads(self.grads)
            self.l2_penalty()
            self.opt_step(opt, norm=True)
        else:
            scale = 1.0
            if comm is not None:
                scale = comm.allreduce_grads(self.grads)
            self.l2_penalty(scale)
            self.opt_step(opt, scale)
        return self.loss_handle() if lazy else self.loss_value()

    def grad_of(self, name):
        kind, off, n, shp, _ = self.slots[name]
        assert kind == "p"
        return self._unpad(name, self.grads[off:off + n].cpu().numpy().reshape(shp))


class GradSink:
    """A kernel is about to write the data gradient of view `inv`, and its epilogue can reduce P partial rows: the one
    place that knows what it needs to be told about that buffer (the six bwd-data sites take their arguments from here).
    out / add: output and addend pointers at the view's channel offset; scale / shift: the mask's, where the view has an
    activation; x: the forward input, where the mask or the sums need it; sx / sld / mean / invstd / dpart: what the
    BatchNorm-backward sums ride along on — against the input's own BatchNorm when this contribution is the last, or
    (alias=True: the caller's epilogue can) against the BatchNorm the gradient reaches unchanged through the residual
    Add whose output this is (Engine.alias_stats_target, .tgt); finish(): fold the sums, or park them for that Add."""
    out = add = x = scale = shift = sx = mean = invstd = dpart = tgt = None
    sld, stat = 0, False

    def __init__(self, eng, inv, P, alias=False):
        self.eng, self.buf, self.P = eng, inv.buf, P
        buf, off = inv.buf, inv.off
        if not buf.requires_grad:   # nothing to write (a kernel that computes another gradient in the same launch)
            return
        gout, add, last = eng.contrib_kernel(buf)
        whole = off == 0 and inv.C == buf.ld
        self.stat = last and bool(buf.bns)
        if self.stat and not whole:
            raise NotImplementedError("BN-backward statistics through a channel slice")
        if not whole and add is not gout:
            # this launch would write ONE slice of a gradient buffer nobody has written yet, and the next contribution
            # takes the whole buffer as its addend: the other slices would be read before anything was stored in them
            raise NotImplementedError("first gradient contribution into a channel slice of a shared buffer")
        self.out = gout.data_ptr() + 4 * off
        self.add = None if add is None else add.data_ptr() + 4 * off
        if inv.act != ACT_NONE:
            self.scale, self.shift = inv.scale(), inv.shift()
        if inv.act != ACT_NONE or self.stat:
            self.x = inv.p()
        if alias and last and not self.stat and whole:
            self.tgt = eng.alias_stats_target(buf)
        sbuf = self.tgt if self.tgt is not None else (buf if self.stat else None)
        if sbuf is not None:   # (a whole view either way: every offset is 0)
            self.sx, self.sld, self.mean, self.invstd = ptr(sbuf.t), sbuf.ld, sbuf.vptr(V_MEAN), sbuf.vptr(V_INVSTD)
            self.dpart = eng.empty(P * sbuf.ld * 2)

    def finish(self):
        if self.tgt is not None:
            self.eng.prestat[id(self.tgt)] = (self.dpart, self.P, self.tgt.ld)
        elif self.stat:
            self.eng.finish_bn_bwd(self.buf, self.dpart, self.P, self.buf.ld)


class LazyLoss:
    """the loss of one step, still on the device: num [* scale / den] [+ the L2 penalty of the step, l2: the clone of
    Engine._l2_tables' out], read (one synchronising copy each) only when somebody converts it — Model.fit / fit_generator
    collect these and read them once per epoch instead of stalling every step"""

    def __init__(self, num, den, scale, l2=None):
        self._num, self._den, self._scale, self._value, self._l2 = num, den, scale, None, l2

    def __float__(self):
        if self._value is None:
            n = float(self._num.cpu()[0])
            self._value = n if self._den is None else n * self._scale / max(float(self._den.cpu()[0]), 1e-20)
            if self._l2 is not None:
                self._value += Engine._l2_sum(self._l2.cpu())
            self._num = self._den = self._l2 = None
        return self._value

    def __repr__(self):
        return repr(float(self))

    def __format__(self, spec):
        return format(float(self), spec)

    def __array__(self, dtype=None, copy=None):
        return np.asarray(float(self), dtype=dtype)


# ======================================================================================
# units
# ======================================================================================


class _ConvBase:
    def __init__(self, eng, layer, inv, outv, want_stat):
        self.eng, self.layer, self.inv, self.outv = eng, layer, inv, outv
        self.bn = None
        self.stat, self.P = None, 0
        self.want_stat = want_stat
        eng._consume(inv)

    def wname(self):
        return self.layer.name + "/kernel:0"


class PwUnit(_ConvBase):
    """Conv2D 1x1 (+bias): dl3_pwconv_fwd / _bwd_weight / _bwd_data.
    wrow0: first row of the layer's [K_total][N] kernel this unit multiplies with (its K = inv.C rows from there);
    img_add: Buf [B,1,1,N] added per image (dl3_pwconv_fwd_add) — together they split a convolution over a Concatenate
    whose first input is the broadcast of a 1x1 map (the ASPP image-pooling branch) into a per-image GEMM of B rows and
    a per-pixel GEMM over the remaining channels (Engine._lo_Conv2D)."""

    def __init__(self, eng, layer, inv, outv, want_stat, wrow0=0, img_add=None, use_bias=True):
        super().__init__(eng, layer, inv, outv, want_stat)
        self.M, self.K, self.N = inv.buf.M, inv.C, outv.C
        self.wrow0, self.img_add = int(wrow0), img_add
        self.bias = layer.name + "/bias:0" if (layer.cfg["use_bias"] and use_bias) else None
        if want_stat:
            self.P = eng.lib.dl3_pwconv_partials(self.M, self.K, self.N)
            self.stat = eng.empty(self.P * self.N * 2)
        s, t, a = inv.xform()
        w = eng.wptr(self.wname()) + 4 * self.wrow0 * self.N
        if img_add is None and not want_stat and inv.buf.H == 1 and inv.buf.W == 1:
            # one row per image (the ASPP image-pooling branch and its share of concat_projection): accumulated in double
            # (dl3_pwconv_fwd_rows) — the result is added to every pixel of the map, its rounding error is coherent
            self.fwd_rec = eng.op(eng.ops_fwd, "dl3_pwconv_fwd_rows", inv.p(), inv.ld, s, t, a, w,
                                  eng.wptr(self.bias) if self.bias else None, outv.p(), outv.ld, self.M, self.K, self.N,
                                  None, 0, 1)
        elif img_add is None:
            self.fwd_rec = eng.op(eng.ops_fwd, "dl3_pwconv_fwd", inv.p(), inv.ld, s, t, a, w,
                                  eng.wptr(self.bias) if self.bias else None, outv.p(), outv.ld, self.M, self.K, self.N,
                                  ptr(self.stat))
        else:
            assert img_add.M == eng.B and img_add.ld == self.N and self.M % eng.B == 0
            eng._consume(View(img_add, 0, self.N))
            self.fwd_rec = eng.op(eng.ops_fwd, "dl3_pwconv_fwd_add", inv.p(), inv.ld, s, t, a, w,
                                  eng.wptr(self.bias) if self.bias else None, outv.p(), outv.ld, self.M, self.K, self.N,
                                  ptr(self.stat), ptr(img_add.t), self.N, self.M // eng.B)

    def set_output_offset(self, neg_offset_ptr):
        """donate the GEMM's free bias slot (a BatchNorm'ed Conv2D has use_bias=False) to -moving_mean: the output tensor
        then holds y - mean, and ONLY affine consumers (scale * stored + beta) may read it — the slice is recorded in
        Buf.centred and Engine._check_centred_consumers refuses a raw view of it"""
        # a convolution with a per-image term (concat_projection: deeplabv3p.py:402-406) subtracts the mean THERE — the
        # few-row GEMM accumulates in double, so addend - mean is rounded once and the per-pixel epilogue adds one number
        # instead of (acc - mean) + addend, whose first step cancels against a mean that contains the addend's average
        rec = self.fwd_rec
        iu = getattr(self, "img_unit", None)
        if iu is not None and iu.fwd_rec[0] == "dl3_pwconv_fwd_rows":
            rec = iu.fwd_rec
        assert rec[0] in ("dl3_pwconv_fwd", "dl3_pwconv_fwd_add", "dl3_pwconv_fwd_rows") and rec.arg("bias") is None and self.bias is None
        rec.set("bias", neg_offset_ptr)
        self.outv.buf.centred.add(self.outv.off)

    def _bwd_img_add(self, g, ldg, y, ldy, cA, cB, cC):
        """gradient of the per-image addend: S[img, n] = sum over the image's pixels of dY[m, n], dY = cA*g + cB*y + cC
        (two per-image column sums with the coefficients folded in, then their sum)"""
        eng, N, B = self.eng, self.N, self.eng.B
        HW = self.M // B
        ab = self.img_add
        gout, add, last = eng.contrib_kernel(ab)
        assert add is None and last and not ab.bns
        if cA is None:
            eng.op(eng.ops_bwd, "dl3_gap_fwd", g, ldg, None, None, ACT_NONE, ptr(gout), B, HW, N, 1.0)
            return
        sg, sy, zero = eng.empty(B * N), eng.empty(B * N), eng.zeros(N)
        eng.op(eng.ops_bwd, "dl3_gap_fwd", g, ldg, cA, cC, ACT_NONE, ptr(sg), B, HW, N, 1.0)
        eng.op(eng.ops_bwd, "dl3_gap_fwd", y, ldy, cB, ptr(zero), ACT_NONE, ptr(sy), B, HW, N, 1.0)
        eng.op(eng.ops_bwd, "dl3_affine_add", ptr(sg), N, None, None, ACT_NONE, ptr(sy), N, None, None, ACT_NONE,
               ptr(gout), N, B, N, 0.0, 0, None)

    def dy_mat_ok(self):
        """(decided ONCE per unit: the buffer sizing in _lower_backward and bwd() must agree)"""
        if getattr(self, "_dy_ok", None) is None:
            self._dy_ok = bool(self._dy_mat_rule())
        return self._dy_ok

    def _dy_mat_rule(self):
        """does the weight-gradient launch of this convolution also write dY for its bwd-data launch?  (its output is
        BatchNorm'ed — otherwise dY is g itself —, it has a weight gradient to compute and data gradient to hand on, the
        backward fork is off — the two launches must stay ordered on one stream — and the shape rule of Engine.dy_mat holds)"""
        eng, outv = self.eng, self.outv
        has_bn = any(off == outv.off for _, off, _ in outv.buf.bns)
        return (has_bn and eng.dy_mat and (self.N <= self.K or self.K >= eng.dy_mat_mink) and self.N % 4 == 0
                and not self.fused_ok()
                and not eng.fork and not self.bias and eng.trainable(self.wname()) and self.inv.buf.requires_grad)

    def fused_ok(self):
        if getattr(self, "_fused_ok", None) is None:
            self._fused_ok = bool(self._fused_rule())
        return self._fused_ok

    def _fused_rule(self):
        """both gradients in one pass (dl3_pwconv_bwd_fused): a small weight matrix, many pixel rows, a trainable kernel
        without bias, a data gradient to hand on, whole aligned tensors on both sides"""
        eng, inv, outv = self.eng, self.inv, self.outv
        if not (eng.fused_bwd and not eng.fork and self.img_add is None and not self.bias and self.wrow0 == 0
                and self.M >= eng.fused_min_rows and eng.trainable(self.wname()) and inv.buf.requires_grad
                and inv.ld % 4 == 0 and inv.off % 4 == 0 and outv.ld % 4 == 0 and outv.off % 4 == 0):
            return False
        sup = eng.lib.dl3_pwconv_bwd_fused_supported(self.M, self.K, self.N)
        # (2: any epilogue; 1 — K > 64 —: no residual addend and sums against the forward input only, i.e. an input with
        # one consumer that is not a bare residual Add output)
        ib = inv.buf
        return sup == 2 or (sup == 1 and ib.expected == 1 and (bool(ib.bns) or id(ib) not in eng.add_of_buf))

    def _bwd_fused(self):
        eng, inv, outv = self.eng, self.inv, self.outv
        M, K, N = self.M, self.K, self.N
        g, ldg, y, ldy, cA, cB, cC = eng.grad_operand(outv)
        s, t, a = inv.xform()
        ibuf = inv.buf
        wT = eng.empty(K * N)
        eng.transpose(eng.wptr(self.wname()), wT, K, N)
        S = eng.lib.dl3_pwconv_bwd_fused_splits(M, K, N)
        ws = eng.lib.dl3_pwconv_bwd_fused_workspace(M, K, N)
        k = GradSink(eng, inv, S, alias=a == ACT_NONE)
        own = eng.empty(ws // 4 + 4)
        eng.own_fold_ws_bytes += ws + 16
        eng.op(eng.ops_bwd, "dl3_pwconv_bwd_fused", inv.p(), inv.ld, s, t, a, g, ldg, y, ldy, cA, cB, cC, ptr(wT), None,
               k.out, ibuf.ld, k.add, ibuf.ld, k.sx, k.sld, k.mean, k.invstd, ptr(k.dpart), M, K, N, ptr(own), ws)
        if eng.defer_fold(S, K * N):
            eng.fold(ptr(own), S, K * N, eng.gptr(self.wname()))
        else:
            eng.op(eng.ops_bwd, "dl3_reduce_partials", ptr(own), S, K * N, eng.gptr(self.wname()))
        k.finish()

    def bwd(self):
        if self.fused_ok():
            return self._bwd_fused()
        eng, inv, outv = self.eng, self.inv, self.outv
        M, K, N = self.M, self.K, self.N
        g, ldg, y, ldy, cA, cB, cC = eng.grad_operand(outv)
        s, t, a = inv.xform()
        wsrc = eng.wptr(self.wname()) + 4 * self.wrow0 * N
        dy = ptr(eng.dy_buf) if (cA is not None and self.dy_mat_ok()) else None
        if eng.trainable(self.wname()) or (self.bias and eng.trainable(self.bias)):
            ws = eng.lib.dl3_pwconv_bwd_weight_workspace(M, K, N)
            S = eng.lib.dl3_pwconv_bwd_weight_splits(M, K, N, 1 if cA else 0)
            fn, tail = ("dl3_pwconv_bwd_weight_dy", (dy, N)) if dy else ("dl3_pwconv_bwd_weight", ())
            if eng.defer_fold(S, K * N) and not self.bias and eng.trainable(self.wname()):
                # the launch leaves its [S][K][N] slabs in a workspace of its own; folded at the end of the pass
                own = eng.empty(ws // 4 + 4)
                eng.own_fold_ws_bytes += ws + 16
                eng.op(eng.ops_bwd, fn, inv.p(), inv.ld, s, t, a, g, ldg, y, ldy, cA, cB, cC,
                       None, None, M, K, N, ptr(own), ws, *tail, side=True)
                eng.fold(ptr(own), S, K * N, eng.gptr(self.wname()) + 4 * self.wrow0 * N)
            else:
                eng.op(eng.ops_bwd, fn, inv.p(), inv.ld, s, t, a, g, ldg, y, ldy, cA, cB, cC,
                       eng.gptr(self.wname()) + (4 * self.wrow0 * N if eng.trainable(self.wname()) else 0),
                       eng.gptr(self.bias) if self.bias else None, M, K, N, 0, ws, *tail, ws=ws, side=True)
        if dy:
            # from here on the layer's gradient operand is the one tensor the weight-gradient launch just wrote
            g, ldg, y, ldy, cA, cB, cC = dy, N, None, 0, None, None, None
        if self.img_add is not None:
            self._bwd_img_add(g, ldg, y, ldy, cA, cB, cC)
        ibuf = inv.buf
        if not ibuf.requires_grad:
            return
        wT = eng.empty(K * N)
        eng.transpose(wsrc, wT, K, N)
        # alias: with no mask and no BatchNorm on a residual Add's output the epilogue's forward-input slot is free — it
        # takes the sums of the BatchNorm this gradient reaches unchanged through the Add
        k = GradSink(eng, inv, eng.lib.dl3_pwconv_partials(M, N, K), alias=a == ACT_NONE)
        eng.op(eng.ops_bwd, "dl3_pwconv_bwd_data", g, ldg, y, ldy, cA, cB, cC, ptr(wT), k.out, ibuf.ld, k.x or k.sx, inv.ld,
               k.scale, k.shift, a, k.add, ibuf.ld, 1, 1.0, k.mean, k.invstd, ptr(k.dpart), M, K, N)
        k.finish()


class DwUnit(_ConvBase):
    """DepthwiseConv2D 3x3: dl3_dwconv3x3_fwd / dl3_dwconv3x3_bwd (fused data+weight gradient)"""

    def __init__(self, eng, layer, inv, outv, stride, rate, pt, pl, want_stat):
        super().__init__(eng, layer, inv, outv, want_stat)
        N, H, W, C = inv.shape
        Ho, Wo = outv.buf.H, outv.buf.W
        self.geom = (eng.B, H, W, C, stride, rate, pt, pl, Ho, Wo)
        self.P = eng.lib.dl3_dwconv3x3_partials(eng.B, H, W, C, stride, rate, Ho, Wo, eng.dw_impl)
        if want_stat:
            self.stat = eng.empty(self.P * C * 2)
        s, t, a = inv.xform()
        eng.op(eng.ops_fwd, "dl3_dwconv3x3_fwd", inv.p(), s, t, a, eng.wptr(self.wname()), outv.p(), *self.geom,
               ptr(self.stat), eng.dw_impl)

    def wname(self):
        return self.layer.name + "/depthwise_kernel:0"

    def bwd(self):
        eng, inv, outv = self.eng, self.inv, self.outv
        C = inv.C
        g, ldg, y, ldy, cA, cB, cC = eng.grad_operand(outv)
        assert ldg == C
        s, t, a = inv.xform()
        wpart = eng.empty(self.P * 9 * C)
        B_, H, W, _, stride, rate, pt, pl, Ho, Wo = self.geom
        # alias: a launch that completes the gradient of a residual Add's output (Xception's `sum` shortcuts) takes the sums
        # of the BatchNorm it reaches unchanged through the Add along (round 4; PwUnit.bwd does the same for MobileNetV2's
        # blocks) instead of a dl3_grad_finish pass over g and y
        k = GradSink(eng, inv, self.P, alias=(stride == 1 and Ho == H and Wo == W and pt == rate and pl == rate
                                              and eng.dw_impl in (IMPL_AUTO, capi.IMPL_MARCH)))
        if k.tgt is not None:
            eng.op(eng.ops_bwd, "dl3_dwconv3x3_bwd_sx", g, y, cA, cB, cC, inv.p(), s, t, a, eng.wptr(self.wname()),
                   k.out, k.add, k.sx, k.mean, k.invstd, ptr(k.dpart), ptr(wpart), *self.geom, eng.dw_impl)
        else:
            eng.op(eng.ops_bwd, "dl3_dwconv3x3_bwd", g, y, cA, cB, cC, inv.p(), s, t, a, eng.wptr(self.wname()),
                   k.out, k.add, k.mean, k.invstd, ptr(k.dpart), ptr(wpart), *self.geom, eng.dw_impl)
        eng.fold(ptr(wpart), self.P, 9 * C, eng.gptr(self.wname()))
        k.finish()


class Conv3Unit(_ConvBase):
    """dense Conv2D 3x3 (stem)"""

    def __init__(self, eng, layer, inv, outv, stride, pt, pl, want_stat):
        super().__init__(eng, layer, inv, outv, want_stat)
        N, H, W, Cin = inv.shape
        Ho, Wo, Cout = outv.buf.H, outv.buf.W, outv.C
        if inv.off != 0 or inv.ld != Cin or outv.off != 0 or outv.ld != Cout:
            raise NotImplementedError("dense 3x3 conv on channel slices")
        self.geom = (eng.B, H, W, Cin, Cout, stride, pt, pl, Ho, Wo)
        # 32/64-channel tensors (xception entry_flow_conv1_2, 32 -> 64): the im2col-free matrix-pipe kernels (taps
        # gathered straight into the MFMA operand); the 3-channel stem convs have their own MFMA kernels behind
        # dl3_conv3x3_fwd
        self.gemm = bool(eng.lib.dl3_conv3x3_mfma_supported(Cin, Cout))
        s, t, a = inv.xform()
        if self.gemm:
            self.P = eng.lib.dl3_conv3x3_mfma_partials(eng.B, Ho, Wo)
            if want_stat:
                self.stat = eng.empty(self.P * Cout * 2)
            eng.op(eng.ops_fwd, "dl3_conv3x3_mfma_fwd", inv.p(), s, t, a, eng.wptr(self.wname()), outv.p(), *self.geom,
                   ptr(self.stat))
            return
        self.P = eng.lib.dl3_conv3x3_partials(eng.B, Ho, Wo, Cout)
        if want_stat:
            self.stat = eng.empty(self.P * Cout * 2)
        eng.op(eng.ops_fwd, "dl3_conv3x3_fwd", inv.p(), s, t, a, eng.wptr(self.wname()), outv.p(), *self.geom,
               ptr(self.stat))

    def _bwd_gemm(self):
        eng, inv, outv = self.eng, self.inv, self.outv
        B, H, W, Cin, Cout, stride, pt, pl, Ho, Wo = self.geom
        g, ldg, y, ldy, cA, cB, cC = eng.grad_operand(outv)
        assert ldg == Cout and (y is None or ldy == Cout)
        s, t, a = inv.xform()
        if eng.trainable(self.wname()):
            ws = eng.lib.dl3_conv3x3_mfma_bwd_weight_workspace(*self.geom[:6], Ho, Wo)
            eng.op(eng.ops_bwd, "dl3_conv3x3_mfma_bwd_weight", inv.p(), s, t, a, g, y, cA, cB, cC,
                   eng.gptr(self.wname()), *self.geom, 0, ws, ws=ws)
        ibuf = inv.buf
        if not ibuf.requires_grad:
            return
        wT = eng.empty(9 * Cin * Cout)
        eng.transpose(eng.wptr(self.wname()), wT, 9 * Cin, Cout)
        k = GradSink(eng, inv, eng.lib.dl3_conv3x3_mfma_partials(B, H, W))
        eng.op(eng.ops_bwd, "dl3_conv3x3_mfma_bwd_data", g, y, cA, cB, cC, ptr(wT), k.out, k.x, k.scale, k.shift, a, k.add,
               k.mean, k.invstd, ptr(k.dpart), *self.geom)
        k.finish()

    def bwd(self):
        if self.gemm:
            return self._bwd_gemm()
        eng, inv, outv = self.eng, self.inv, self.outv
        B, H, W, Cin, Cout, stride, pt, pl, Ho, Wo = self.geom
        g, ldg, y, ldy, cA, cB, cC = eng.grad_operand(outv)
        s, t, a = inv.xform()
        if eng.trainable(self.wname()):
            wpart = eng.empty(self.P * 9 * Cin * Cout)
            eng.op(eng.ops_bwd, "dl3_conv3x3_bwd_weight", inv.p(), s, t, a, g, y, cA, cB, cC, ptr(wpart), *self.geom)
            eng.fold(ptr(wpart), self.P, 9 * Cin * Cout, eng.gptr(self.wname()))
        ibuf = inv.buf
        if not ibuf.requires_grad:
            return
        k = GradSink(eng, inv, eng.lib.dl3_conv3x3_partials(B, H, W, Cin))
        eng.op(eng.ops_bwd, "dl3_conv3x3_bwd_data", g, y, cA, cB, cC, eng.wptr(self.wname()), k.out, k.x, k.scale, k.shift, a,
               k.add, k.mean, k.invstd, ptr(k.dpart), *self.geom)
        k.finish()


class AddUnit:
    """Add (deeplabv3p.py:147-149,:201): out = T(a) + T(b); backward = gradient aliases"""

    def __init__(self, eng, a, b, outv):
        self.eng, self.a, self.b, self.outv = eng, a, b, outv
        eng._consume(a)
        eng._consume(b)
        sa, ta, aa = a.xform()
        sb, tb, ab = b.xform()
        eng.op(eng.ops_fwd, "dl3_affine_add", a.p(), a.ld, sa, ta, aa, b.p(), b.ld, sb, tb, ab, outv.p(), outv.ld,
               outv.buf.M, outv.C, 0.0, 0, None)

    def bwd(self):
        g = self.outv.buf.grad
        for v in (self.a, self.b):
            self.eng.contrib_passthrough(v.buf, v, g)


class MaterializeUnit:
    """Dropout(0.1) in training mode (deeplabv3p.py:410): out = T(x) * keepmask/(1-rate)"""

    def __init__(self, eng, inv, outv, rate, seed):
        self.eng, self.inv, self.outv, self.rate, self.seed = eng, inv, outv, rate, seed
        eng._consume(inv)
        s, t, a = inv.xform()
        eng.op(eng.ops_fwd, "dl3_affine_add", inv.p(), inv.ld, s, t, a, None, 0, None, None, ACT_NONE, outv.p(),
               outv.ld, outv.buf.M, outv.C, rate, seed, eng.drop_step.data_ptr())

    def bwd(self):
        g = self.outv.buf.grad
        self.eng.contrib_elementwise(self.inv.buf, self.inv, ptr(g), self.outv.ld, drop=(self.rate, self.seed))


class GapUnit:
    """global AveragePooling2D (deeplabv3p.py:375)"""

    def __init__(self, eng, inv, outv):
        self.eng, self.inv, self.outv = eng, inv, outv
        eng._consume(inv)
        s, t, a = inv.xform()
        self.HW = inv.buf.H * inv.buf.W
        eng.op(eng.ops_fwd, "dl3_gap_fwd", inv.p(), inv.ld, s, t, a, outv.p(), eng.B, self.HW, inv.C, 1.0 / self.HW)

    def bwd(self):
        g = self.outv.buf.grad
        if not self.inv.buf.requires_grad:
            return
        self.eng.contrib_elementwise(self.inv.buf, self.inv, ptr(g), self.outv.ld, gin_div=self.HW,
                                     gin_scale=1.0 / self.HW)


class ResizeUnit:
    """Lambda(tf.image.resize_bilinear) (deeplabv3p.py:382,:418,:439; utils.py:190)"""

    def __init__(self, eng, inv, outv, Ho, Wo):
        self.eng, self.inv, self.outv = eng, inv, outv
        eng._consume(inv)
        s, t, a = inv.xform()
        self.dims = (eng.B, inv.buf.H, inv.buf.W, Ho, Wo, inv.C)
        eng.op(eng.ops_fwd, "dl3_resize_bilinear_fwd", inv.p(), inv.ld, s, t, a, outv.p(), outv.ld, *self.dims)

    def bwd(self):
        eng, inv, outv = self.eng, self.inv, self.outv
        ibuf = inv.buf
        if not ibuf.requires_grad:
            return
        B, Hi, Wi, Ho, Wo, C = self.dims
        if eng.loss_head.unit is self and eng.loss_head.folded is not None:
            # fused training tail: the loss kernel already folded the output columns (dl3_upsample_softmax_xent_fold)
            gout, add, last = eng.contrib_kernel(ibuf)
            eng.op(eng.ops_bwd, "dl3_resize_bilinear_bwd_rows", ptr(eng.loss_head.folded), ptr(gout), ibuf.ld, B, Hi, Wi, Ho, C,
                   1 if add is not None else 0)
            if add is not None and add is not gout:
                raise NotImplementedError("resize backward with a foreign addend")
            return
        g = outv.buf.grad.data_ptr() + 4 * outv.off
        plain = inv.act == ACT_NONE and not ibuf.bns and inv.off == 0 and inv.C == ibuf.ld
        if Hi == 1 and Wi == 1:
            # a 1x1 source is a broadcast: its transpose is the per-image column sum
            tmp = eng.empty(B * C)
            eng.op(eng.ops_bwd, "dl3_gap_fwd", g, outv.ld, None, None, ACT_NONE, ptr(tmp), B, Ho * Wo, C, 1.0)
            eng.contrib_elementwise(ibuf, inv, ptr(tmp), C)
        elif plain:
            gout, add, last = eng.contrib_kernel(ibuf)
            ws = eng.lib.dl3_resize_bilinear_bwd_workspace(B, Hi, Wi, Ho, Wo, C)
            eng.op(eng.ops_bwd, "dl3_resize_bilinear_bwd", g, outv.ld, ptr(gout), ibuf.ld, B, Hi, Wi, Ho, Wo,
                   C, 1 if add is not None else 0, 0, ws, ws=ws)
            if add is not None and add is not gout:
                raise NotImplementedError("resize backward with a foreign addend")
        else:
            tmp = eng.empty(ibuf.M * C)
            ws = eng.lib.dl3_resize_bilinear_bwd_workspace(B, Hi, Wi, Ho, Wo, C)
            eng.op(eng.ops_bwd, "dl3_resize_bilinear_bwd", g, outv.ld, ptr(tmp), C, B, Hi, Wi, Ho, Wo, C, 0,
                   0, ws, ws=ws)
            eng.contrib_elementwise(ibuf, inv, ptr(tmp), C)


class ShuffleUnit:
    """Subpixel._phase_shift (subpixel.py:77-88)"""

    def __init__(self, eng, inv, outv, r, co):
        self.eng, self.inv, self.outv, self.r, self.co = eng, inv, outv, r, co
        eng._consume(inv)
        eng.op(eng.ops_fwd, "dl3_phase_shift", inv.p(), outv.p(), eng.B, inv.buf.H, inv.buf.W, co, r, 0)

    def bwd(self):
        eng, inv = self.eng, self.inv
        if eng.loss_head.unit is self:   # the loss kernel wrote the gradient in the unshuffled layout already
            assert inv.buf.grad is not None and not inv.buf.bns
            inv.buf.done += 1
            return
        gout, add, last = eng.contrib_kernel(inv.buf)
        assert add is None and not inv.buf.bns
        eng.op(eng.ops_bwd, "dl3_phase_shift", ptr(self.outv.buf.grad), ptr(gout), eng.B, inv.buf.H, inv.buf.W,
               self.co, self.r, 1)


class TapsUnit:
    """k x k taps of T(x) side by side in front of the GEMM of a Subpixel with kernel_size > 1 (subpixel.py:42-58)"""

    def __init__(self, eng, inv, outv, k, pt, pl):
        self.eng, self.inv, self.outv = eng, inv, outv
        eng._consume(inv)
        s, t, a = inv.xform()
        self.dims = (eng.B, inv.buf.H, inv.buf.W, inv.C, k, pt, pl, outv.buf.H, outv.buf.W)
        eng.op(eng.ops_fwd, "dl3_conv_taps_fwd", inv.p(), inv.ld, s, t, a, outv.p(), *self.dims)

    def bwd(self):
        eng, inv = self.eng, self.inv
        if not inv.buf.requires_grad:
            return
        tmp = eng.empty(inv.buf.M * inv.C)
        eng.op(eng.ops_bwd, "dl3_conv_taps_bwd", ptr(self.outv.buf.grad), ptr(tmp), *self.dims)
        eng.contrib_elementwise(inv.buf, inv, ptr(tmp), inv.C)


class SubsampleUnit:
    """row/column sampling in front of a strided 1x1 convolution (Xception shortcuts, deeplabv3p.py:143-145)"""

    def __init__(self, eng, inv, outv, stride):
        self.eng, self.inv, self.outv, self.stride = eng, inv, outv, stride
        eng._consume(inv)
        s, t, a = inv.xform()
        self.dims = (eng.B, inv.buf.H, inv.buf.W, inv.C, stride, outv.buf.H, outv.buf.W)
        eng.op(eng.ops_fwd, "dl3_subsample_fwd", inv.p(), inv.ld, s, t, a, outv.p(), *self.dims)

    def bwd(self):
        eng, inv = self.eng, self.inv
        if not inv.buf.requires_grad:
            return
        tmp = eng.empty(inv.buf.M * inv.C)
        eng.op(eng.ops_bwd, "dl3_subsample_bwd", ptr(self.outv.buf.grad), ptr(tmp), *self.dims)
        eng.contrib_elementwise(inv.buf, inv, ptr(tmp), inv.C)
