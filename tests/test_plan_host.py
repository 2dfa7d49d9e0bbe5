"""Host tests of the host layer's shared decisions: engine.Plan (run eagerly once, capture on the second call, replay from
then on, fall back to eager launches engine-wide when the capture raises) against counting fakes of torch's graph API, and
the input coercion helpers on CPU tensors and arrays.  No GPU."""
import types

import numpy as np
import pytest
import torch

import dl3_amd  # noqa: F401
from dl3_amd import graph as G
from dl3_amd.engine import Plan, flat_f32, pixels_to_device


class _Fakes:
    """counting stand-ins for torch.cuda.synchronize / CUDAGraph / graph; events: what happened, in order"""

    def __init__(self, monkeypatch, fail=False):
        self.events, self.graphs, self.capturing = [], [], False
        fakes = self

        class FakeGraph:
            def __init__(self):
                fakes.graphs.append(self)
                self.replays = 0

            def replay(self):
                assert not fakes.capturing
                self.replays += 1
                fakes.events.append("replay")

        class FakeCapture:
            def __init__(self, g):
                assert isinstance(g, FakeGraph)

            def __enter__(self):
                if fail:
                    raise RuntimeError("no capture today")
                fakes.capturing = True
                fakes.events.append("capture")

            def __exit__(self, *exc):
                fakes.capturing = False
                return False

        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: self.events.append("sync"))
        monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
        monkeypatch.setattr(torch.cuda, "graph", FakeCapture)

    def body(self, tag="body"):
        def run():
            self.events.append(tag + ("@capture" if self.capturing else ""))
        return run


def test_plan_runs_eagerly_once_then_captures_and_replays(monkeypatch):
    f = _Fakes(monkeypatch)
    plan = Plan(types.SimpleNamespace(use_graph=True), f.body())
    plan.run()
    assert plan.graph is None and f.events == ["body"]
    plan.run()
    assert plan.graph is f.graphs[0] and f.events == ["body", "sync", "capture", "body@capture", "replay"]
    plan.run()
    assert f.events[5:] == ["replay"] and len(f.graphs) == 1 and plan.graph.replays == 2
    assert f.events.count("sync") == 1 and sum(e.startswith("body") for e in f.events) == 2


def test_plan_without_graphs_only_calls_the_body(monkeypatch):
    f = _Fakes(monkeypatch)
    plan = Plan(types.SimpleNamespace(use_graph=False), f.body())
    for _ in range(3):
        plan.run()
    assert f.events == ["body"] * 3 and f.graphs == [] and plan.graph is None and plan.calls == 0


def test_plan_capture_failure_falls_back_to_eager(monkeypatch, capsys):
    f = _Fakes(monkeypatch, fail=True)
    eng = types.SimpleNamespace(use_graph=True)
    plan = Plan(eng, f.body())
    plan.run()
    assert f.events == ["body"] and eng.use_graph
    plan.run()   # the capture context raises on entry: the body of this call runs exactly once, eagerly
    out = capsys.readouterr().out
    assert "dl3: hipGraph capture failed (no capture today); running eagerly" in out
    assert eng.use_graph is False and plan.graph is None
    assert f.events == ["body", "sync", "sync", "body"]
    plan.run()
    plan.run()
    assert f.events[4:] == ["body", "body"] and plan.graph is None and len(f.graphs) == 1
    assert capsys.readouterr().out == ""


def test_two_plans_share_only_the_engines_switch(monkeypatch):
    f = _Fakes(monkeypatch)
    eng = types.SimpleNamespace(use_graph=True)
    a, b = Plan(eng, f.body("a")), Plan(eng, f.body("b"))
    a.run()
    a.run()
    assert a.graph is not None and (a.calls, b.calls) == (2, 0) and b.graph is None
    b.run()
    assert f.events[-1] == "b" and b.graph is None and b.calls == 1   # b's own first call: eager
    b.run()
    assert b.graph is not None and b.graph is not a.graph and (a.graph.replays, b.graph.replays) == (1, 1)
    # a capture failure in one plan makes the other one eager from then on, captured graph or not
    f2 = _Fakes(monkeypatch, fail=True)
    c = Plan(eng, f2.body("c"))
    c.run()
    c.run()
    assert eng.use_graph is False and c.graph is None and f2.events == ["c", "sync", "sync", "c"]
    a.run()
    b.run()
    assert f.events[-2:] == ["a", "b"] and (a.graph.replays, b.graph.replays) == (1, 1)


def test_raw_pixels_and_pixels_to_device():
    u8 = np.arange(2 * 4 * 4 * 3, dtype=np.uint8).reshape(2, 4, 4, 3)
    assert G.raw_pixels(u8) is u8
    t = pixels_to_device(u8, "cpu")
    assert t.dtype == torch.uint8 and t.is_contiguous() and np.array_equal(t.numpy(), u8)
    for other in (u8.astype(np.float64), u8.tolist(), u8.astype(np.int32)):
        r = G.raw_pixels(other)
        assert isinstance(r, np.ndarray) and r.dtype == np.float32 and np.array_equal(r, u8)
        t = pixels_to_device(other, "cpu")
        assert t.dtype == torch.float32 and t.is_contiguous() and np.array_equal(t.numpy(), u8)
    # non-contiguous inputs come out contiguous, values in place
    for strided in (u8[:, ::2], u8.astype(np.float32).transpose(0, 2, 1, 3), torch.from_numpy(u8)[:, :, ::2]):
        assert not (strided.flags.c_contiguous if isinstance(strided, np.ndarray) else strided.is_contiguous())
        t = pixels_to_device(strided, "cpu")
        assert t.is_contiguous() and tuple(t.shape) == tuple(strided.shape) and np.array_equal(t.numpy(), np.asarray(strided))
    # a tensor is not copied: raw_pixels hands it back, pixels_to_device keeps its storage (uint8 and float32 alike)
    for ten in (torch.from_numpy(u8), torch.from_numpy(u8.astype(np.float32))):
        assert G.raw_pixels(ten) is ten
        assert pixels_to_device(ten, "cpu").data_ptr() == ten.data_ptr()
    t = pixels_to_device(torch.from_numpy(u8.astype(np.float64)), "cpu")
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), u8)


def test_flat_f32_of_labels_and_weights():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 4, (2, 16, 1))
    sw = rng.random((2, 16))
    for a in (y, y.astype(np.float32), y.tolist(), torch.from_numpy(y), sw, sw.astype(np.float32), torch.from_numpy(sw),
              torch.from_numpy(sw).t()):
        t = flat_f32(a, "cpu")
        want = (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float32).reshape(-1)
        assert t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous() and np.array_equal(t.numpy(), want)
    f = torch.from_numpy(sw.astype(np.float32))
    assert flat_f32(f, "cpu").data_ptr() == f.data_ptr()   # already flat-able float32: a view, no copy


@pytest.mark.parametrize("n,bs,want", [(5, 2, [(0, 2), (2, 4), (4, 6)]), (3, 8, [(0, 3)]), (4, 2, [(0, 2), (2, 4)])])
def test_batches_cut_as_predict_does(n, bs, want):
    assert [(s.start, s.stop) for s in G.batches(n, bs)] == want
    assert [len(range(n)[s]) for s in G.batches(n, bs)] == [min(b, n) - a for a, b in want]
