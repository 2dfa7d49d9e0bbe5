"""CPU checks of the case table of tests/test_gpu_pwconv.py (tests/pwconv_cases.py): every case still gets the plan it was
written for — asked of the planner itself through tools/pwplan_probe.cpp, a host program that includes csrc/pwplan.h —, the
library's sizing and route queries agree with that plan, the exactness conditions behind the == comparisons hold, and every
kernel instantiation the launchers can name is named by a case."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pwconv_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "keras-segmentation-deeplab-v3.1_amd")
ROUTE_OF = {"stream": 0, "lds": 0, "wgrad": 0, "ws": 1, "ws2": 2, "ksplit": 3, "wgrad_row": 4, "flat": 5, "narrowk": 5, "wgrad_narrow": 5}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tools/pwplan_probe.cpp built with the host compiler: run(specs, env) -> one parsed JSON answer per spec, from a fresh
    process whose DL3_* environment is exactly `env` (four of the planner's knobs are read once per process)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pwplan_probe") / "pwplan_probe")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "pwplan_probe.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(specs, env=()):
        e = {k: v for k, v in os.environ.items() if not k.startswith("DL3_")}
        e.update(dict(env))
        out = []
        for i in range(0, len(specs), 500):
            r = subprocess.run([exe] + list(specs[i:i + 500]), env=e, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out += [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(specs)
        return out

    return run


@pytest.fixture(scope="module")
def plans(probe):
    """{case id: the probe's answer} for every case that goes through plan_gemm / plan_wgrad, one process per knob setting"""
    groups = {}
    for c in C.CASES:
        if C.probe_spec(c):
            groups.setdefault(C.knob_env(c), []).append(c)
    out = {}
    for env, cases in groups.items():
        for c, p in zip(cases, probe([C.probe_spec(c) for c in cases], env)):
            out[c.id] = p
    return out


@pytest.fixture(scope="module")
def L():
    path = os.environ.get("DL3_LIBPATH") or os.path.join(PKG, "libdl3.so")
    lib = ctypes.CDLL(path)
    for name, n in (("dl3_pwconv_route", 4), ("dl3_pwconv_fwd_impl", 3), ("dl3_pwconv_partials", 3),
                    ("dl3_pwconv_bwd_weight_workspace", 3), ("dl3_pwconv_bwd_weight_splits", 4),
                    ("dl3_pwconv_bwd_fused_supported", 3), ("dl3_pwconv_bwd_fused_splits", 3), ("dl3_pwconv_bwd_fused_workspace", 3)):
        f = getattr(lib, name)
        f.argtypes = [ctypes.c_int] * n
        f.restype = ctypes.c_size_t if name.endswith("workspace") else ctypes.c_int
    return lib


@pytest.fixture
def no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("DL3_") and k != "DL3_LIBPATH"]:
        monkeypatch.delenv(k)


def test_table_is_well_formed():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids)) and set(ids) == set(C.PLANS)
    for c in C.CASES:
        assert c.entry in ("fwd", "bwd_data", "bwd_weight", "fused") and c.form in ("none", "affine", "act", "affine+act"), c.id
        assert (c.act in (1, 2)) == c.form.endswith("act") and c.add in (0, 1, 2) and 0 < c.wd <= 1, c.id
        assert c.entry != "fwd" or not (c.two or c.dy_out or c.dbias or c.slabs), c.id
        assert c.entry == "fwd" or not c.bias, c.id
        assert c.entry in ("bwd_weight", "fused") or not (c.dy_out or c.dbias or c.slabs), c.id
        assert not (c.dbias and (c.two or c.slabs)), c.id                       # (include/dl3.h: dbias needs dw and a plain dY)
        assert c.entry == "fused" or c.stats in (True, False), c.id
        assert c.entry != "bwd_weight" or not c.add, c.id
        assert c.entry != "fused" or (c.add in (0, 1) and not C.misaligned(c) and not c.lay), c.id
        for item in c.lay:
            assert item == ("mis",) or (item[0] in ("x", "g", "y", "dx", "dy") and item[1] % 4 == 0 and item[2] % 4 == 0), c.id
        # a case above a row threshold sits on the threshold itself plus a ragged tail (below one 32-row tile twice over)
        # (the older tests' own shapes, C.OLD, stay as they are)
        if c.M >= 8192 and not c.id.startswith(("ws-32x172-1250", "fused-more", "real-fused", "old-")):
            assert min(c.M - t for t in (8192, 16384, 32768, 65536, 98304, 131072) if c.M >= t) < 72, c.id


def test_every_case_gets_the_plan_it_declares(plans):
    """a retuned threshold or cost model fails the case here instead of moving it to another kernel unseen"""
    got = {c.id: C.describe(c, plans.get(c.id)) for c in C.CASES}
    bad = {i: (C.PLANS[i], got[i]) for i in got if got[i] != C.PLANS[i]}
    assert not bad, "declared plan, planner's plan: %s" % bad


def test_split_math_cases_run_split_math():
    """a case that asks for split math is declared on a split-math instantiation (the 32-row stream tiles, cfg 5 / 6, keep the
    f32 MFMA whatever the knob says: such a case would hold an f32 kernel to the split-math bar), and no other case is"""
    for c in C.CASES:
        if c.entry != "fused":
            assert C.runs_split_math(c) == C.split_math(c), (c.id, C.PLANS[c.id])
    real = [c for c in C.REAL if C.runs_split_math(c)]
    assert {c.entry for c in real} >= {"fwd", "bwd_data", "bwd_weight"}
    assert any(" two " in C.PLANS[c.id] + " " for c in real) and any(" pre " in C.PLANS[c.id] + " " for c in real)


# the tile edges each kernel's text distinguishes (rows, columns, reduction against the tile; weight gradient: K and N against the
# tile, M against the 16-row stage; fused: 32-blocks and the 32-row stage).  The weight-stationary kernels are instantiated per K.
EDGES = {"stream": "MNK", "lds": "MNK", "ksplit": "MNK", "ws": "MN", "ws2": "MN", "flat": "M", "narrowk": "M", "wgrad": "KNM",
         "wgrad_row": "KNM", "wgrad_narrow": "M", "fused1": "KNM", "fused2": "KNM"}


def test_whole_and_ragged_tiles_are_both_declared():
    """per kernel: a case whose last row / column / K tile is whole and one where it is ragged; fewer rows than one stage for the
    weight-gradient and fused kernels — among the EXACT cases, where a wrong tail cannot hide"""
    seen = {}
    for c in C.CASES:
        if not c.exact:
            continue
        for part in C.PLANS[c.id].split(" + "):
            words = part.split()
            seen.setdefault(words[0], set()).update(w for w in words[1:] if w[:2] in ("M=", "M<", "N=", "N<", "K=", "K<"))
    assert set(seen) == set(EDGES)
    for kernel, dims in EDGES.items():
        for dim in dims:
            assert {dim + "=", dim + "<"} <= seen[kernel], (kernel, dim, sorted(seen[kernel]))
    assert "M<16" in seen["wgrad"] and "M<32" in seen["fused1"] and "M<32" in seen["fused2"]


def test_library_queries_agree_with_the_probe(probe, plans, L, no_knobs):
    """dl3_pwconv_route, _fwd_impl, _partials, _bwd_weight_splits and _workspace of the built library are the probe's answers for
    every shape of the table, and they hold every case's own launch: its partial rows, slabs and column-sum rows"""
    shapes = sorted({(c.M, c.K, c.N) for c in C.CASES})
    for (M, K, N), q in zip(shapes, probe(["q:%d:%d:%d" % s for s in shapes])):
        assert [L.dl3_pwconv_route(d, M, K, N) for d in range(5)] == q["route"], (M, K, N)
        assert L.dl3_pwconv_fwd_impl(M, K, N) == q["fwd_impl"], (M, K, N)
        assert (L.dl3_pwconv_partials(M, K, N), L.dl3_pwconv_partials(M, N, K)) == (q["partials"], q["partials_bwd"]), (M, K, N)
        assert L.dl3_pwconv_bwd_weight_workspace(M, K, N) == q["workspace"], (M, K, N)
        assert [L.dl3_pwconv_bwd_weight_splits(M, K, N, t) for t in (0, 1)] == q["splits"], (M, K, N)
    for c in C.CASES:
        p = plans.get(c.id)
        if c.entry == "fwd":
            assert p["rows"] <= L.dl3_pwconv_partials(c.M, c.K, c.N), c.id
        elif c.entry == "bwd_data":
            assert p["rows"] <= L.dl3_pwconv_partials(c.M, c.N, c.K), c.id
        elif c.entry == "bwd_weight":
            assert 4 * (p["slabs"] * c.K * c.N + p["colsum_rows"] * c.N) <= L.dl3_pwconv_bwd_weight_workspace(c.M, c.K, c.N), c.id
            if c.slabs:   # the caller folds dl3_pwconv_bwd_weight_splits slabs
                assert p["slabs"] == L.dl3_pwconv_bwd_weight_splits(c.M, c.K, c.N, int(c.two)), c.id
        else:
            kb, nb = -(-c.K // 32), -(-c.N // 32)
            assert L.dl3_pwconv_bwd_fused_supported(c.M, c.K, c.N) == (2 if c.K <= 64 else 1) and kb * nb <= 6, c.id
            S = L.dl3_pwconv_bwd_fused_splits(c.M, c.K, c.N)
            assert S >= 1 and L.dl3_pwconv_bwd_fused_workspace(c.M, c.K, c.N) == 4 * S * c.K * c.N, c.id


def route_dir(c):
    """the dir of dl3_pwconv_route whose canonical operand form is the case's (None: the diagnostic has none for it)"""
    if C.misaligned(c) or c.knobs or c.entry == "fused":
        return None
    if c.entry == "fwd":
        return None if c.add else 0
    if c.entry == "bwd_data":
        if c.two or c.add:
            return None
        return 1 if (c.stats and c.act) else (3 if not c.stats and not c.act else None)
    return 2 if c.two else (None if c.slabs else 4)


def test_route_diagnostic_names_the_declared_kernel(L, no_knobs):
    n = 0
    for c in C.CASES:
        d = route_dir(c)
        if d is None:
            continue
        kernel = C.PLANS[c.id].split()[0]
        want = ROUTE_OF[kernel]
        if d == 3 and want != 5:
            want = 0   # (dir 3 answers for the logits layer only: include/dl3.h)
        assert L.dl3_pwconv_route(d, c.M, c.K, c.N) == want, c.id
        n += 1
    assert n >= 40


@pytest.mark.parametrize("case", [c for c in C.CASES if c.exact], ids=lambda c: c.id)
def test_exactness_conditions(case):
    """the sums of absolute terms behind every == of the GPU file stay below 2**24 (fp32 holds every partial sum exactly), and the
    fp32 reference equals the float64 one where that is cheap to evaluate"""
    d = C.draw(case)
    r = C.reference(case, d)
    for name, value, limit in C.conditions(case, d, r):
        assert value < limit, (case.id, name, value, limit)
    if case.M <= 8192:
        r64 = C.reference(case, d, np.float64)
        for key in ("out", "dw", "dy", "s1", "s2", "dbias"):
            if key in r:
                assert np.array_equal(np.asarray(r[key], np.float64), r64[key]), (case.id, key)
    # the data exercise what the case is about: both sides of every mask threshold, non-zero weights in every column block
    z = d["x"] if d["s"] is None else d["s"] * d["x"] + d["t"]
    if case.act:
        assert (z <= 0).any() and (z > 0).any() and (case.act != 2 or ((z >= 6).any() and (z == 6).any())) and (z == 0).any(), case.id
    assert all((d["w"][:, j:j + 32] != 0).any() for j in range(0, case.N, 32)), case.id
    assert all((d["w"][k:k + 8] != 0).any() for k in range(0, case.K, 8)), case.id


def test_every_instantiation_is_named_by_a_case(probe):
    """launch_stream, launch_lds, launch_ws, launch_ksplit, launch_wgrad and the fused launcher switch over the instantiations
    C.universe() lists; each is the declared plan of a case, except the combinations C.EXEMPT names — which the planner must
    then never produce, for a case or for a shape of the recorded plan table"""
    uni, cov = C.universe(), C.covered()
    assert cov <= uni, sorted(cov - uni)
    assert set(C.EXEMPT) <= uni and not (set(C.EXEMPT) & cov)
    assert uni - cov == set(C.EXEMPT), sorted(uni - cov - set(C.EXEMPT))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "pwconv_plan_table.json")))
    fake = C.BY_ID["stream-cfg0-fwd"]
    seen = set()
    for spec, entry, kw in (("f:%d:%d:%d:16:0:%d:%d:1", "fwd", {}), ("b:%d:%d:%d:18:0:%d:%d:%d:1", "bwd_data", {}),
                            ("w:%d:%d:%d:513:0", "bwd_weight", dict(two=True)), ("w:%d:%d:%d:512:0", "bwd_weight", {})):
        shapes = [tuple(r[:3]) for r in gold["rows"]]
        args = [spec % ((M, K, N) + {"fwd": (K, N), "bwd_data": (N, K, K), "bwd_weight": ()}[entry]) for M, K, N in shapes]
        for (M, K, N), p in zip(shapes, probe(args)):
            c = fake._replace(entry=entry, M=M, K=K, N=N, dy_out=False, **kw)
            for inst in C.instantiation(c, C.describe(c, p)):
                w = inst.split()
                seen.add(" ".join(w[:4]) if w[0] == "wgrad" else ("wgrad_narrow" if w[0] == "wgrad_narrow" else inst))
    assert seen <= uni, sorted(seen - uni)
    assert not (seen & set(C.EXEMPT)), sorted(seen & set(C.EXEMPT))


def test_universe_restates_the_launchers():
    """the switch statements of the launchers, as text: a launcher that gains or loses an instantiation fails here"""
    import re
    src = {n: re.sub(r"\s+", " ", open(os.path.join(PKG, "csrc", n)).read())
           for n in ("pwstream.hip", "pwlds.hip", "pwws.hip", "pwsmall.hip", "pwwgrad.hip", "pwfused.hip")}
    assert len(re.findall(r"case \d+: DL3_F32\(|default: DL3_F32\(", src["pwstream.hip"])) == 7
    assert len(re.findall(r"case \d+: DL3_SPLIT\(|default: DL3_SPLIT\(", src["pwstream.hip"])) == 5
    assert src["pwstream.hip"].count("pw_gemm_stream_kernel<1, 3, ") == 4                       # the four prefetching forms
    assert len(re.findall(r"case \d+: DL3_LDS\(|default: DL3_LDS\(", src["pwlds.hip"])) == 5
    assert [int(m) for m in re.findall(r"pw_gemm_kernel<TM_, TN_, WM_, WN_, (\d)>", src["pwlds.hip"])] == [1, 2, 0]
    assert re.findall(r"pw_ksplit32_kernel<(\d), (\w+)>\)", src["pwsmall.hip"]) == [
        ("2", "false"), ("2", "true"), ("3", "false"), ("3", "true"), ("5", "false"), ("5", "true")]
    assert [(int(a), int(b)) for a, b in re.findall(r"DL3_GO\(\(pw_fwd_ws_kernel<(\d+), (\d+), \d>\)", src["pwws.hip"])] == [
        (2, 3), (3, 5), (4, 1), (4, 6), (12, 1), (18, 1), (24, 1)]
    assert re.findall(r"DL3_GO\(\(pw_ws2_kernel<([^>]*)>\)", src["pwws.hip"]) == [
        "32, 1, NW, false, false, false, true", "48, 2, NW, true, true, true", "48, 2, NW, true, true, false", "20, 5, NW, true",
        "12, 3, NW, true", "8, 4, NW, true", "20, 5, NW", "12, 3, NW", "8, 4, NW"]
    assert src["pwws.hip"].count("DL3_GO((pw_narrowk_kernel<8, NW>)") == 1
    assert len(re.findall(r"case \d: DL3_WG\(|default: DL3_WG\(", src["pwwgrad.hip"])) == 10
    assert re.findall(r"DL3_GO\(\(pw_wgrad_kernel<TA_, TB_, WA_, WB_, ([^>]*)>\)", src["pwwgrad.hip"]) == ["1, true", "1", "2", "0"]
    assert re.findall(r"DL3_GO\(\(pw_wgrad_row_kernel<(\d), 1, 1, 4, (\w+)>\)", src["pwwgrad.hip"]) == [
        ("5", "true"), ("5", "false"), ("3", "true"), ("3", "false")]
    assert src["pwwgrad.hip"].count("hipLaunchKernelGGL((pw_wgrad_narrow_kernel<") == 1
    for version, pat in ((1, r"DL3_FUSED\((\d), (\d), (\w+)\);"), (2, r"DL3_FUSED\((\d), (\d), (\w+), \d\);")):
        got = sorted((int(a), int(b), f == "true") for a, b, f in re.findall(pat, src["pwfused.hip"]))
        assert got == C.fused_shapes(version), version
