"""Hard-example mining, host side (no GPU): the numpy oracle's selection and schedule against hand-computed values, the
argument checks of utils.sparse_crossentropy_top_k, and the training-engine key."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import graph as G
from dl3_amd import utils as U
from tests import mine_oracle as M

V = np.array([0, .5, .5, 2, 0, 1], np.float32)


@pytest.mark.parametrize("k,tau,mask,n", [
    (2, 1.0, [0, 0, 0, 1, 0, 1], 2),
    (3, 0.5, [0, 1, 1, 1, 0, 1], 4),      # both ties at tau are kept: 4 pixels for k = 3
    (6, 0.0, [0, 1, 1, 1, 0, 1], 4),      # tau = 0: the zeros pass v >= tau but not v > 0
    (0, np.inf, [0, 0, 0, 0, 0, 0], 0),
])
def test_selection_by_hand(k, tau, mask, n):
    t, m, cnt = M.select(V, k)
    assert t == np.float32(tau) and cnt == n
    assert m.tolist() == [bool(b) for b in mask]


def test_mined_weights_by_hand():
    w = np.array([3, 3, 0, 2, 5, 7], np.float32)
    v = V * (w != 0)                      # the zero weight takes pixel 2 out: v = [0, .5, 0, 2, 0, 1]
    k, tau, w2, n = M.mine(v, w, 0.5, 0, 0)
    assert (k, float(tau), n) == (3, 0.5, 3)
    assert w2.tolist() == [0, 3, 0, 2, 0, 7]
    # no weights: w = 1
    assert M.mine(V, None, 0.5, 0, 0)[2].tolist() == [0, 1, 1, 1, 0, 1]


def _k(p, S, s, N):
    """the schedule by the oracle and by the package's host restatement (sparse_crossentropy_top_k.pixels_kept): one value"""
    k = M.schedule_k(p, S, s, N)
    assert U.sparse_crossentropy_top_k(p, S).pixels_kept(s, N) == k
    return k


def test_schedule_by_hand():
    p, S = 0.25, 100
    assert M.schedule_pct(p, S, 0) == np.float32(1.0) and _k(p, S, 0, 4096) == 4096     # s = 0: k = N
    assert M.schedule_pct(p, S, 50) == np.float32(0.625)                                          # .5 * .25 + .5
    for s in (100, 107, 10 ** 6):
        assert M.schedule_pct(p, S, s) == np.float32(0.25) and _k(p, S, s, 4096) == 1024
    assert _k(p, 0, 0, 4096) == 1024 and _k(p, 0, 12345, 4096) == 1024        # S = 0: pct = p at once
    # truncation: 0.625 * 10 = 6.25 -> 6; 0.25 * 7 = 1.75 -> 1; 0.25 * 3 = 0.75 -> 0
    assert _k(p, S, 50, 10) == 6 and _k(p, S, 100, 7) == 1 and _k(p, S, 100, 3) == 0
    # k never exceeds N
    assert _k(1.0, 0, 0, 5) == 5


def test_schedule_float32_roundings_matter():
    """p = 0.1, S = 3, s = 2: ratio = fl(2/3) = 0.6666667, fl(ratio * p) = 0.06666667, fl(1 - ratio) = 0.3333333 and their
    float32 sum is 0.39999998, so 1000 pixels give k = 399 — in exact (or float64) arithmetic pct = 0.4 and k = 400"""
    assert M.schedule_pct(0.1, 3, 2) == np.float32(0.39999998)
    assert M.schedule_pct(0.1, 3, 2) < np.float32(0.4)
    assert _k(0.1, 3, 2, 1000) == 399
    r = 2.0 / 3.0
    assert int((r * 0.1 + (1 - r)) * 1000) == 400


def test_loss_object_arguments():
    l = U.sparse_crossentropy_top_k(0.25, 100)
    assert l.mining == (0.25, 100) and (l.top_k_percent_pixels, l.hard_example_mining_step) == (0.25, 100)
    assert U.sparse_crossentropy_top_k(0.5).mining == (0.5, 0)
    assert U.sparse_crossentropy_top_k(1.0, 10).mining is None        # p == 1 switches mining off
    assert U.sparse_crossentropy_top_k(1, 0).mining is None
    assert U.sparse_crossentropy_top_k(np.float32(0.5), np.int64(3)).mining == (0.5, 3)
    for bad in [(0.0, 0), (-0.1, 0), (1.0001, 0), (float("nan"), 0), ("0.5", 0), (None, 0), (True, 0)]:
        with pytest.raises(ValueError):
            U.sparse_crossentropy_top_k(*bad)
    for bad in [(0.5, -1), (0.5, 1.5), (0.5, 2.0), (0.5, "3"), (0.5, None), (0.5, True)]:
        with pytest.raises(ValueError):
            U.sparse_crossentropy_top_k(*bad)


def test_loss_object_on_host_arrays_returns_the_pixel_losses():
    rng = np.random.default_rng(0)
    p = rng.uniform(0.1, 1.0, (2, 7, 3))
    y = rng.integers(0, 4, (2, 7, 1)).astype(np.float32)
    a = U.sparse_crossentropy_top_k(0.25, 3)(y, p)
    assert np.array_equal(a, U.sparse_crossentropy_ignoring_last_label(y, p))
    assert a.shape == (2, 7) and (a[y[..., 0] == 3] == 0).all()


def _model():
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone="mobilenetv2", OS=16)


def test_engine_key_carries_the_mining_settings():
    model = _model()
    keys = {}
    for name, loss in [("plain", U.sparse_crossentropy_ignoring_last_label), ("none", None),
                       ("one", U.sparse_crossentropy_top_k(1.0, 50)), ("a", U.sparse_crossentropy_top_k(0.25, 4)),
                       ("b", U.sparse_crossentropy_top_k(0.25, 5)), ("c", U.sparse_crossentropy_top_k(0.5, 4))]:
        model.compile(optimizer=None, loss=loss)
        model._compile_gen = 1            # the compile counter is part of every key: hold it still
        keys[name] = model._engine_key(2, True, {"dropout": False})
    # p == 1.0 (and any other loss) lowers today's engine: same key, same constructor keywords
    assert keys["one"] == keys["plain"] == keys["none"]
    assert "mining" not in keys["plain"][1]
    assert keys["a"][1]["mining"] == (0.25, 4)
    assert len({keys[n][0] for n in ("plain", "a", "b", "c")}) == 4
    # inference engines never carry it
    model.compile(optimizer=None, loss=U.sparse_crossentropy_top_k(0.25, 4))
    key, kw = model._engine_key(2, False, {})
    assert "mining" not in kw and key == (2, False, ())
