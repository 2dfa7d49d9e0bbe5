"""The engine's lowering, recorded: a fixed list of plans lowered on the CPU (no GPU needed: tests/test_host.py::_dry_engine)
and written down in a canonical form, so that "the lowering still produces the same launches over the same buffers" is an
equality of hashes.

A plan is ops_prep + ops_fwd + ops_bwd of a training engine; of an inference engine ops_fwd, the evaluation plan's launch
list (weighted + mask, and unweighted without mask) and the CRF-unary launch list.  Per launch: the name, every scalar
argument verbatim, every pointer argument (capi.protos() says which) as [allocation, byte offset, allocation bytes], the
workspace slot, and whether the launch is in _side / _join_before.  Allocations are numbered in order of first use, NULL and
None are one value; the pointer columns of the batched transpose / fold descriptors follow in the same numbering.  A buffer
sized differently, a shifted offset, a reordered launch or a changed alias change the record; the order in which Python
happened to allocate does not.  A pointer inside no tensor the engine holds is an error.

tests/golden/engine_plans.json holds per plan the SHA-256 of its canonical JSON, the launch count and the launch-name counts;
tests/test_plan_record_host.py compares.  A pull request that changes a plan on purpose re-records it:

  python tools/plan_record.py                # rewrites tests/golden/engine_plans.json
  python tools/plan_record.py --check        # exit 1 (and the name-count difference) where a plan differs from the golden
  python tools/plan_record.py --full F.json  # the whole records, for diffing two trees (not committed)
  ... [NAME ...]                             # only the named plans (--check / --full)"""
import bisect
import collections
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_plans.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ------------------------------------------------------------------------------------------------ the plans
def _deeplab(backbone, size, classes, OS=16):
    from dl3_amd.deeplabv3p import Deeplabv3
    return Deeplabv3(weights=None, input_shape=(size, size, 3), classes=classes, backbone=backbone, OS=OS)


def _subpixel(backbone, size, classes):
    from dl3_amd.utils import SegModel
    return SegModel(image_size=(size, size)).create_seg_model("subpixel", n=classes, backbone=backbone)


def _act_only(size=64, cin=8, classes=21):
    """tests/test_host.py::_act_only_logits_model: a head that ends in neither a resize nor a phase shift"""
    from dl3_amd import graph as G
    inp = G.Input(shape=(size, size, cin))
    x = G.Conv2D(256, 1, name="c0")(inp)
    x = G.Activation("relu")(x)
    x = G.Conv2D(classes, 1, use_bias=True, name="logits")(x)
    x = G.Reshape((size * size, -1))(x)
    x = G.Activation("softmax", name="pred_mask")(x)
    return G.Model(inp, x, name="act_only_logits")


def _fine_tune(backbone, size, classes):
    """the notebook's fine-tuning freeze: every layer before concat_projection with trainable = False"""
    m = _deeplab(backbone, size, classes)
    live = False
    for l in m.layers:
        live = live or l.name == "concat_projection"
        l.trainable = live
    return m


SMALL = collections.OrderedDict([
    ("mnv2_deeplab_c5", lambda: _deeplab("mobilenetv2", 64, 5)),
    ("mnv2_subpixel_c5", lambda: _subpixel("mobilenetv2", 64, 5)),
    ("xception_subpixel_c3", lambda: _subpixel("xception", 64, 3)),
    ("mnv2_deeplab_c40", lambda: _deeplab("mobilenetv2", 64, 40)),
    ("act_only_c21", _act_only),
])


def plans():
    """[(name, model builder, batch, training, Engine keywords, environment)]"""
    out = []
    for m, build in SMALL.items():
        for mining in (None, (0.25, 100)):
            for ext in (False, True):
                name = "train64/%s%s%s" % (m, "/mined" if mining else "", "/external_nnz" if ext else "")
                out.append((name, build, 2, True, dict(mining=mining, external_nnz=ext), {}))
    for m, build in SMALL.items():
        out.append(("infer64/" + m, build, 2, False, {}, {}))
    out += [
        ("train512/mnv2_deeplab_c32_b1", lambda: _deeplab("mobilenetv2", 512, 32), 1, True, {}, {}),
        ("train512/mnv2_deeplab_c21_b128", lambda: _deeplab("mobilenetv2", 512, 21), 128, True, {}, {}),
        ("train512/mnv2_deeplab_c21_b2", lambda: _deeplab("mobilenetv2", 512, 21), 2, True, {}, {}),
        ("train512/mnv2_subpixel_c21_b16", lambda: _subpixel("mobilenetv2", 512, 21), 16, True, {}, {}),
        ("train256/xception_os8_c21_b1", lambda: _deeplab("xception", 256, 21, OS=8), 1, True, {}, {}),
        ("knob64/subpixel_FUSE_SHUFFLE=0", SMALL["mnv2_subpixel_c5"], 2, True, {}, {"DL3_FUSE_SHUFFLE": "0"}),
    ]
    for env in ("DL3_FORK=1", "DL3_FORK=2", "DL3_DY_MAT=0", "DL3_FUSED_BWD=0", "DL3_FUSED_ROWS=1024", "DL3_BATCH_FOLDS=0",
                "DL3_PRUNE_BWD=0"):
        out.append(("knob64/" + env, SMALL["mnv2_deeplab_c5"], 2, True, {}, dict([env.split("=")])))
    out.append(("knob64/bn_frozen", SMALL["mnv2_deeplab_c5"], 2, True, dict(bn_mode="frozen"), {}))
    out.append(("knob64/fine_tune", lambda: _fine_tune("mobilenetv2", 64, 5), 2, True, {}, {}))
    return out


# ------------------------------------------------------------------------------------------------ lowering on the CPU
def lower(build, batch, training, kw, env):
    import torch
    import dl3_amd  # noqa: F401
    from dl3_amd import capi, graph as G
    from dl3_amd.engine import Engine
    capi.lib()
    saved = {k: os.environ.get(k) for k in env}
    avail, cur = torch.cuda.is_available, torch.cuda.current_device
    torch.cuda.is_available, torch.cuda.current_device = (lambda: True), (lambda: 0)
    os.environ.update(env)
    try:
        G.clear_session(seed=7)
        return Engine(build(), batch=batch, training=training, device="cpu", **kw)
    finally:
        torch.cuda.is_available, torch.cuda.current_device = avail, cur
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def sections(eng):
    """[(section name, launch list)] of an engine.  The one place that knows how the evaluation and CRF-unary lists are
    reached."""
    if eng.training:
        return [("prep", eng.ops_prep), ("fwd", eng.ops_fwd), ("bwd", eng.ops_bwd)]
    return [("fwd", eng.ops_fwd), ("eval_weighted_mask", eng._eval_plan(None, True, True)[1]),
            ("eval", eng._eval_plan(None, False, False)[1]), ("crf_unary", eng._crf_ops(None, None, 1e-5))]


# ------------------------------------------------------------------------------------------------ the canonical record
def _tensors(root):
    """every torch tensor reachable from the engine: _keep, the Bufs and units, the arenas, the mining / evaluation / CRF
    state, the counters — found by walking the engine's own objects"""
    import torch
    seen, found, stack = set(), [], [root]
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if torch.is_tensor(o):
            found.append(o)
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            stack.extend(o)
        elif isinstance(o, types.SimpleNamespace) or type(o).__module__.startswith("dl3_amd.") and hasattr(o, "__dict__"):
            if type(o).__module__ != "dl3_amd.graph":   # (the Keras-side graph holds host weights only)
                stack.extend(vars(o).values())
    return found


class _Allocations:
    def __init__(self, eng):
        spans = {}
        for t in _tensors(eng):
            s = t.untyped_storage()
            if s.nbytes():
                spans[s.data_ptr()] = max(spans.get(s.data_ptr(), 0), s.nbytes())
        self.starts = sorted(spans)
        self.sizes = [spans[s] for s in self.starts]
        self.number = {}

    def norm(self, p, what):
        if not p:
            return None
        i = bisect.bisect_right(self.starts, p) - 1
        if i < 0 or p >= self.starts[i] + self.sizes[i]:
            raise RuntimeError("%s: pointer %#x lies in no tensor the engine holds" % (what, p))
        n = self.number.setdefault(self.starts[i], len(self.number))
        return [n, p - self.starts[i], self.sizes[i]]


def _scalar(v):
    if isinstance(v, bool) or v is None:
        return v
    if isinstance(v, int):
        return int(v)
    return float(v)


def record(eng):
    from dl3_amd import capi
    protos = capi.protos()
    secs = sections(eng)       # (an inference engine allocates its evaluation state when first asked for that plan)
    A = _Allocations(eng)
    rec = collections.OrderedDict()
    for sec, ops in secs:
        rows = []
        for i, op in enumerate(ops):
            name, _, args, ws = op
            types_ = [t for t, _ in protos[name][1]][:-1]   # (the trailing stream is the replay's; Engine.op checked the count)
            vals = [A.norm(a, "%s[%d] %s arg %d" % (sec, i, name, j)) if t.endswith("*") else _scalar(a)
                    for j, (t, a) in enumerate(zip(types_, args))]
            rows.append([name, vals, ws, id(op) in eng._side, id(op) in eng._join_before])
        rec[sec] = rows
    for d in ("_tdesc", "_fdesc"):   # [src, dst, ...] per row
        t = getattr(eng, d, None)
        rec[d] = [] if t is None else [[A.norm(r[0], d), A.norm(r[1], d)] + r[2:] for r in t.tolist()]
    sizes = dict(scratch_bytes=eng.scratch_bytes, side_scratch_bytes=eng.side_scratch_bytes,
                 own_fold_ws_bytes=eng.own_fold_ws_bytes, lossP=getattr(eng, "lossP", None), n_param=eng.n_param,
                 params=eng.params.numel(), state=eng.state.numel())
    if eng.training:
        sizes.update(grads=eng.grads.numel(), tail=eng.tail, adam_m=eng.adam_m.numel(), adam_v=eng.adam_v.numel())
    rec["sizes"] = sizes
    return rec


def summary(rec):
    names = collections.Counter(r[0] for sec, rows in rec.items() if sec not in ("_tdesc", "_fdesc", "sizes") for r in rows)
    text = json.dumps(rec, sort_keys=False, separators=(",", ":"))
    return dict(sha256=hashlib.sha256(text.encode()).hexdigest(), launches=sum(names.values()), names=dict(sorted(names.items())))


def compare(name, want, got):
    """"" where plan `name` equals its golden entry, else what differs"""
    if want == got:
        return ""
    if want is None:
        return "%s: not in the golden file" % name
    a, b = want["names"], got["names"]
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)}
    return "%s: recorded %s (%d launches), now %s (%d launches); launch names (recorded, now): %s" % (
        name, want["sha256"][:12], want["launches"], got["sha256"][:12], got["launches"], diff or "equal")


def run(only=()):
    """{plan name: (summary, whole record)}"""
    out = collections.OrderedDict()
    for name, build, batch, training, kw, env in plans():
        if only and name not in only:
            continue
        rec = record(lower(build, batch, training, kw, env))
        out[name] = (summary(rec), rec)
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    full = argv.pop(argv.index("--full") + 1) if "--full" in argv else None
    flags = {a for a in argv if a.startswith("--")}
    got = run([a for a in argv if not a.startswith("--")])
    if full:
        json.dump({k: v[1] for k, v in got.items()}, open(full, "w"), indent=0)
    if "--check" in flags:
        gold = json.load(open(GOLDEN))
        bad = [compare(k, gold.get(k), v[0]) for k, v in got.items() if gold.get(k) != v[0]]
        print("\n".join(bad) if bad else "%d plans equal the recorded ones" % len(got))
        sys.exit(1 if bad else 0)
    if not full:
        json.dump({k: v[0] for k, v in got.items()}, open(GOLDEN, "w"), indent=0, sort_keys=True)
        print("%s: %d plans, %d bytes" % (os.path.relpath(GOLDEN, ROOT), len(got), os.path.getsize(GOLDEN)))
