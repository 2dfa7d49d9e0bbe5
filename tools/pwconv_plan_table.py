"""The 1x1-convolution planner's decision table: for a list of layer shapes (M rows, K -> N channels) one line each with every
answer the library's host-side queries give — no GPU needed.

  route0..route4   dl3_pwconv_route(dir, M, K, N), dir 0-4, in the layer's orientation
  fwd_impl         dl3_pwconv_fwd_impl(M, K, N)
  part_fwd/_bwd    dl3_pwconv_partials(M, K, N) / (M, N, K): the forward / bwd-data GEMM's statistic partial rows
  wgrad_ws         dl3_pwconv_bwd_weight_workspace(M, K, N), bytes
  splits1/2        dl3_pwconv_bwd_weight_splits(M, K, N, 0 / 1)

tests/golden/pwconv_plan_table.json is this table for default_shapes() under the default knobs, and
tests/golden/pwconv_plan_table_knobs.json the tables of the benchmarked B=128 / B=2 plans under KNOB_SETTINGS, both recorded
from the library BEFORE the planner (csrc/pwplan.h) replaced the hand-kept copies of the dispatch; tests/test_host.py
recomputes both from the built library and compares every field.  A pull request that moves a route, a grid or a buffer size
on purpose re-records them:

  python tools/pwconv_plan_table.py                 # rewrites both golden files from the built library
  python tools/pwconv_plan_table.py --shapes F.json # the rows for the [[M, K, N], ...] in F.json, as JSON on stdout"""
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pwconv_plan_table.json")
GOLDEN_KNOBS = os.path.join(ROOT, "tests", "golden", "pwconv_plan_table_knobs.json")
FIELDS = ["M", "K", "N", "route0", "route1", "route2", "route3", "route4", "fwd_impl", "part_fwd", "part_bwd", "wgrad_ws",
          "splits1", "splits2"]
KNOB_SETTINGS = (["DL3_WS2=0", "DL3_NARROW=0", "DL3_COLSPLIT=0", "DL3_WGRAD_ROW=0"] + ["DL3_GEMM_CFG=%d" % i for i in range(7)] +
                 ["DL3_GEMM_MATH=split"])
EDGE_ROWS = (1024, 8192, 16384, 32768, 65536, 98304, 131072)
# (K, N) of the layers each route family serves, in the layer's orientation; both orientations where bwd-data has a route
EDGE_KN = {
    "ws_hbm": [(32, 16), (16, 96), (96, 24), (24, 144), (144, 24), (144, 32), (32, 192), (192, 32)],
    "ws_mfma": [(160, 960), (160, 320), (96, 576), (96, 192), (64, 384), (64, 128), (960, 160), (576, 96), (384, 64), (320, 160)],
    "narrow": [(256, 21), (256, 32), (256, 2), (256, 33)],
    "ksplit": [(384, 96), (256, 144), (196, 132), (192, 64), (2048, 160)],
    "colsplit": [(256, 608), (608, 256), (736, 736), (512, 864)],
    "wgrad_row": [(80, 448), (160, 328), (96, 128)],
    "prefetch": [(96, 48), (320, 96), (192, 32)],
    "unaligned": [(30, 21), (32, 21), (728, 728)],
}


def lib():
    path = os.environ.get("DL3_LIBPATH") or os.path.join(ROOT, "keras-segmentation-deeplab-v3.1_amd", "libdl3.so")
    L = ctypes.CDLL(path)
    for name, n in (("dl3_pwconv_route", 4), ("dl3_pwconv_fwd_impl", 3), ("dl3_pwconv_partials", 3),
                    ("dl3_pwconv_bwd_weight_workspace", 3), ("dl3_pwconv_bwd_weight_splits", 4)):
        f = getattr(L, name)
        f.argtypes = [ctypes.c_int] * n
        f.restype = ctypes.c_size_t if name.endswith("workspace") else ctypes.c_int
    return L


def rows_for(shapes, L=None):
    L = L or lib()
    return [[M, K, N] + [L.dl3_pwconv_route(d, M, K, N) for d in range(5)] +
            [L.dl3_pwconv_fwd_impl(M, K, N), L.dl3_pwconv_partials(M, K, N), L.dl3_pwconv_partials(M, N, K),
             L.dl3_pwconv_bwd_weight_workspace(M, K, N), L.dl3_pwconv_bwd_weight_splits(M, K, N, 0),
             L.dl3_pwconv_bwd_weight_splits(M, K, N, 1)] for M, K, N in shapes]


PW_LAUNCHES = ("dl3_pwconv_fwd", "dl3_pwconv_fwd_add", "dl3_pwconv_fwd_rows", "dl3_pwconv_bwd_data", "dl3_pwconv_bwd_weight",
               "dl3_pwconv_bwd_weight_dy")


def plan_shapes(backbone, B, size=512, OS=16, head="deeplab"):
    """every distinct (M, K, N) of the 1x1-convolution launches of a training plan, lowered without a GPU (the engine only
    records launches and asks the library's sizing queries while it lowers: tests/test_host.py _dry_engine)"""
    import torch
    sys.path.insert(0, ROOT)
    import dl3_amd  # noqa: F401
    from dl3_amd import capi, graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    from dl3_amd.engine import Engine
    from dl3_amd.utils import SegModel
    capi.lib()   # (loaded before torch.cuda claims to be available: it initialises the GPU only where there is one)
    torch.cuda.is_available = lambda: True
    torch.cuda.current_device = lambda: 0
    G.clear_session()
    if head == "deeplab":
        m = Deeplabv3(weights=None, input_shape=(size, size, 3), classes=21, backbone=backbone, OS=OS)
    else:
        m = SegModel(image_size=(size, size)).create_seg_model(head, n=21, backbone=backbone)
    e = Engine(m, batch=B, training=True, device="cpu")
    return sorted({tuple(op.arg(k) for k in "MKN") for op in e.ops_fwd + e.ops_bwd if op[0] in PW_LAUNCHES})


def test_shapes():
    """(M, K, N) of every case tuple in the 1x1-convolution tests of tests/test_gpu_ops.py: the top-level blocks that mention
    pwconv, and the case lists those blocks name"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_ops.py")).read()
    blocks = [b.strip() for b in re.split(r"\n\n\n+", text)]
    pw = [b for b in blocks if "pwconv" in b]
    named = {m.group(1) for b in pw for m in re.finditer(r"\b([A-Z][A-Z0-9_]+)\b", b)}
    pw += [b for b in blocks if re.match(r"([A-Z0-9_]+) = ", b) and re.match(r"([A-Z0-9_]+) = ", b).group(1) in named]
    out = set()
    for b in pw:
        for m in re.finditer(r"\(\s*(\d[\d +*]*?),\s*(\d+),\s*(\d+)\s*[,)]", b):
            M = eval(m.group(1), {"__builtins__": {}})   # (digits, + and * only: the pattern admits nothing else)
            out.add((M, int(m.group(2)), int(m.group(3))))
    return sorted(out)


def bench_shapes():
    """the benchmarked plan (MobileNetV2, 512 x 512) at B=128 and B=2: the shapes of the knob tables"""
    return sorted(set(plan_shapes("mobilenetv2", 128)) | set(plan_shapes("mobilenetv2", 2)))


def default_shapes():
    s = set()
    for B in (2, 4, 8, 16, 24, 32, 64, 128):
        s |= set(plan_shapes("mobilenetv2", B))
    s |= set(plan_shapes("mobilenetv2", 128, head="subpixel"))
    s |= set(plan_shapes("xception", 1, size=256, OS=8)) | set(plan_shapes("xception", 16, OS=8))
    s |= set(plan_shapes("xception", 16, OS=16))
    s |= set(test_shapes())
    for pairs in EDGE_KN.values():
        s |= {(M + d, K, N) for K, N in pairs for M in EDGE_ROWS for d in (-1, 0, 1)}
    return sorted(s)


def dump(path, obj_rows, extra=None):
    """one compact line per shape"""
    head = dict(extra or {}, fields=FIELDS)
    with open(path, "w") as f:
        f.write("{" + ", ".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in head.items()) + ', "rows": ')
        if isinstance(obj_rows, dict):
            f.write("{\n" + ",\n".join("%s: [\n%s]" % (json.dumps(k), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
                                        for k, rows in obj_rows.items()) + "}}\n")
        else:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in obj_rows) + "]}\n")


def knob_rows(setting, shapes, tmp):
    """the table under one knob setting, from a fresh process (four of the knobs are read once per process)"""
    with open(tmp, "w") as f:
        json.dump([list(s) for s in shapes], f)
    name, val = setting.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DL3_") or k == "DL3_LIBPATH"}
    env[name] = val
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--shapes", tmp], env=env, capture_output=True, text=True,
                         check=True)
    return json.loads(res.stdout)


if __name__ == "__main__":
    if "--shapes" in sys.argv:
        shapes = json.load(open(sys.argv[sys.argv.index("--shapes") + 1]))
        print(json.dumps(rows_for(shapes)))
        sys.exit(0)
    import tempfile
    rows = rows_for(default_shapes())
    dump(GOLDEN, rows)
    bs = bench_shapes()
    with tempfile.TemporaryDirectory() as d:
        dump(GOLDEN_KNOBS, {s: knob_rows(s, bs, os.path.join(d, "shapes.json")) for s in KNOB_SETTINGS})
    print("%s: %d shapes, %d bytes; %s: %d settings x %d shapes, %d bytes" % (
        os.path.relpath(GOLDEN, ROOT), len(rows), os.path.getsize(GOLDEN), os.path.relpath(GOLDEN_KNOBS, ROOT),
        len(KNOB_SETTINGS), len(bs), os.path.getsize(GOLDEN_KNOBS)))
