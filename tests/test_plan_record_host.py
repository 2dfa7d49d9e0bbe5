"""The engine's lowering against its record (tools/plan_record.py): every recorded plan — training, inference, evaluation
and CRF-unary plans of every head form, the benchmarked 512x512 plans, each lowering knob — lowers on the CPU to the launch
lists, arguments, buffer aliases, offsets and sizes whose hash tests/golden/engine_plans.json holds.  No GPU needed."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("plan_record", os.path.join(ROOT, "tools", "plan_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_plan_equals_the_recorded_one():
    T = _tool()
    gold = json.load(open(T.GOLDEN))
    names = [p[0] for p in T.plans()]
    assert sorted(names) == sorted(gold) and len(names) == 40, "the plan list and the golden file name different plans"
    got = T.run()
    bad = [T.compare(k, gold[k], v[0]) for k, v in got.items() if gold[k] != v[0]]
    print("\n".join(bad))
    assert not bad, "%d of %d plans differ from the recorded ones:\n%s" % (len(bad), len(got), "\n".join(bad))


def test_a_pointer_outside_the_engines_tensors_is_an_error():
    """the record's own net: a launch argument that points into no tensor the engine holds is refused, NULL and None are
    one value, and a pointer is recorded as (allocation in order of first use, byte offset, allocation bytes)"""
    import pytest
    import torch
    T = _tool()
    a, b = torch.zeros(16), torch.zeros(8)
    A = T._Allocations([b, a, a[4:]])
    assert A.norm(None, "x") is None and A.norm(0, "x") is None
    assert A.norm(a.data_ptr() + 20, "x") == [0, 20, 64] and A.norm(b.data_ptr(), "x") == [1, 0, 32]
    assert A.norm(a[4:].data_ptr(), "x") == [0, 16, 64]
    with pytest.raises(RuntimeError):
        A.norm(a.data_ptr() + 64 if a.data_ptr() + 64 != b.data_ptr() else b.data_ptr() + 32, "x")
