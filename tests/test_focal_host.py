"""The focal loss on the host: the oracle's closed-form gradient against autograd of the definition, its
reduction to the cross-entropy, hand-computed pixels on both sides of the clip, the loss object, the argument checks, the
engine key, and what the header and the head's table declare."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import graph as G
from dl3_amd import utils as U
from oracle import dl3_oracle as O
from tests import focal_oracle as F


def _case(seed=3, B=3, HW=37, C=5):
    """void labels, a fifth of the weights zero, a random alpha"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, HW, C)) * 3
    t = rng.integers(0, C + 1, (B, HW)).astype(np.float64)
    w = rng.uniform(0.5, 2.0, (B, HW)) * (rng.random((B, HW)) > 0.2)
    alpha = rng.uniform(0.5, 2.0, C)
    assert (t == C).any() and (w == 0).any()
    return z, t, w, alpha


def _torch_loss(z, t, w, gamma, alpha):
    """the definition, written down independently: per-pixel function, then sample weight, then count(w != 0)"""
    import torch
    C = z.shape[-1]
    p = torch.softmax(z, -1)
    valid = t < C
    tc = torch.where(valid, t, torch.zeros_like(t))
    q = torch.clamp((p / p.sum(-1, keepdim=True)).gather(-1, tc[..., None])[..., 0], float(F.CLIP_LO), float(F.CLIP_HI))
    ell = alpha[tc] * (1 - q) ** gamma * -torch.log(q)
    return (torch.where(valid, ell, torch.zeros_like(ell)) * w).sum() / (w != 0).sum()


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
def test_closed_form_equals_autograd_of_the_definition(gamma):
    """B = 3, HW = 37, C = 5 in float64: loss and gradient against torch-CPU autograd, 1e-15 absolute"""
    import torch
    z, t, w, alpha = _case()
    r = F.evaluate("plain", z[:, None], None, t, w, gamma, alpha, np.float64)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    L = _torch_loss(zt, torch.tensor(t).long(), torch.tensor(w), gamma, torch.tensor(alpha))
    L.backward()
    d, L = float(np.abs(r["dlogits"] - zt.grad.numpy()).max()), float(L.detach())
    print("gamma %.1f: loss %.17g against %.17g, gradient distance %.3e" % (gamma, r["loss"], L, d))
    assert abs(r["loss"] - L) <= 1e-15 * max(1.0, abs(L)) and d <= 1e-15
    assert (r["dlogits"][(t == 5) | (w == 0)] == 0).all() and np.abs(r["dlogits"]).max() > 1e-4


def test_gamma_zero_without_alpha_is_the_cross_entropy_exactly():
    z, t, w, _ = _case(seed=5)
    r = F.evaluate("plain", z[:, None], None, t, w, 0.0, None, np.float64)
    ce = U.sparse_crossentropy_ignoring_last_label(t[..., None], O.softmax(z))
    assert np.array_equal(r["ell"], ce)
    loss, dl = O.loss_sparse_xent_ignoring_last_label(z, t, w)[:2]
    assert abs(r["loss"] - loss) <= 1e-15 * loss and np.abs(r["dlogits"] - dl).max() <= 1e-17
    ones = F.evaluate("plain", z[:, None], None, t, w, 0.0, np.ones(5), np.float64)
    assert np.array_equal(ones["ell"], r["ell"]) and np.array_equal(ones["dlogits"], r["dlogits"])


def test_two_classes_by_hand_on_both_sides_of_the_clip():
    """C = 2, label 0, w = 1, nnz = 4, gamma = 2, alpha = (3, 1).  Pixel 0: z = (0, 0), q = 1/2: l = 3/4 log 2, mu = 1/4 +
    2 * 1/2 * 1/2 * log 2.  Pixel 1: z = (0, 20), p_0 = 1 / (1 + e^20) = 2.06e-9 < 1e-7: q is the lower bound, the loss is
    the constant 3 (1 - lo)^2 (-log lo) and the gradient is zero.  Pixel 2: z = (20, 0), p_0 > 1 - 1e-7: q is the upper
    bound, constant loss, zero gradient.  Pixel 3: void."""
    z = np.array([[[0.0, 0.0], [0.0, 20.0], [20.0, 0.0], [1.0, -1.0]]])
    t = np.array([[0.0, 0.0, 0.0, 2.0]])
    r = F.evaluate("plain", z[:, None], None, t, None, 2.0, (3.0, 1.0), np.float64)
    lo, hi = float(F.CLIP_LO), float(F.CLIP_HI)
    ell = [3 * 0.25 * np.log(2.0), 3 * (1 - lo) ** 2 * -np.log(lo), 3 * (1 - hi) ** 2 * -np.log(hi), 0.0]
    assert np.allclose(r["ell"][0], ell, rtol=1e-14, atol=0)
    assert abs(r["loss"] - sum(ell) / 4) <= 1e-15
    mu = 0.25 + 2 * 0.5 * 0.5 * np.log(2.0)
    assert np.allclose(r["dlogits"][0, 0], [3 * mu * (0.5 - 1) / 4, 3 * mu * 0.5 / 4], rtol=1e-14, atol=0)
    assert (r["dlogits"][0, 1:] == 0).all()
    # nudging a clipped pixel's logits leaves its loss where it is
    z2 = z.copy()
    z2[0, 1] += [0.25, -0.25]
    z2[0, 2] += [0.25, -0.25]
    r2 = F.evaluate("plain", z2[:, None], None, t, None, 2.0, (3.0, 1.0), np.float64)
    assert np.array_equal(r2["ell"][0, 1:3], r["ell"][0, 1:3])


def test_float32_yardstick_is_close_and_not_equal():
    z, t, w, alpha = _case()
    a = F.evaluate("plain", z[:, None].astype(np.float32), None, t, w.astype(np.float32), 2.0, alpha.astype(np.float32), np.float64)
    b = F.evaluate("plain", z[:, None].astype(np.float32), None, t, w.astype(np.float32), 2.0, alpha.astype(np.float32), np.float32)
    assert b["dlogits"].dtype == np.float32 and b["ell"].dtype == np.float32
    d = np.abs(a["dlogits"] - b["dlogits"]).max()
    assert 0 < d < 1e-7 and 0 < abs(a["loss"] - b["loss"]) < 1e-6 * a["loss"]


def test_shuffle_form_reads_through_the_subpixel_index_map():
    rng = np.random.default_rng(2)
    u = rng.standard_normal((2, 3, 5, 3 * 4))
    full = O.phase_shift(u, 2)
    assert np.array_equal(F.unshuffle(full, u.shape, 2), u)
    t = rng.integers(0, 4, (2, 6 * 10)).astype(np.float64)
    a = F.evaluate("shuffle", u, 2, t, None, 2.0, None)
    b = F.evaluate("plain", full, None, t, None, 2.0, None)
    assert np.array_equal(a["dlogits"], b["dlogits"]) and a["loss"] == b["loss"]


def test_loss_object_on_host_arrays_returns_the_per_pixel_focal_loss():
    z, t, w, alpha = _case(seed=9)
    for gamma, al in ((2.0, tuple(alpha)), (0.5, None), (2.0, 0.25), (0.0, tuple(alpha))):
        obj = U.sparse_focal_crossentropy(gamma, al)
        got = obj(t[..., None], O.softmax(z))
        want = F.evaluate("plain", z[:, None], None, t, None, gamma, al, np.float64)["ell"]
        assert got.dtype == np.float64 and got.shape == t.shape
        assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), (gamma, al)
    with pytest.raises(ValueError, match="class weights"):
        U.sparse_focal_crossentropy(2.0, (1.0, 2.0))(t[..., None], O.softmax(z))


def test_loss_object():
    l = U.sparse_focal_crossentropy()
    assert l.gamma == 2.0 and l.alpha is None and l.focal == (2.0, None)
    assert l.__name__ == "sparse_focal_crossentropy" and repr(l) == "sparse_focal_crossentropy(2.0, None)"
    l = U.sparse_focal_crossentropy(np.float32(0.5), np.array([0.5, 1, 2], np.float32))
    assert l.focal == (0.5, (0.5, 1.0, 2.0)) and repr(l) == "sparse_focal_crossentropy(0.5, (0.5, 1.0, 2.0))"
    assert U.sparse_focal_crossentropy(1, 0.25).focal == (1.0, (0.25,))
    # off: gamma == 0 with alpha None or all ones
    for al in (None, 1, 1.0, (1, 1, 1), np.ones(3)):
        assert U.sparse_focal_crossentropy(0.0, al).focal is None
    assert U.sparse_focal_crossentropy(0.0, (1, 2, 1)).focal == (0.0, (1.0, 2.0, 1.0))
    assert U.sparse_focal_crossentropy(2.0, (1, 1, 1)).focal == (2.0, None)
    assert G.check_focal(None) is None


@pytest.mark.parametrize("bad", [(-1.0, None), (float("nan"), None), (float("inf"), None), (-0.5, (1, 1)), (True, None),
                                 ("2", None), (2.0, (1.0, -1.0)), (2.0, (1.0, float("nan"))), (2.0, (float("inf"),)),
                                 (2.0, -0.25), (2.0, ()), (2.0, (1.0, "x")), (2.0, (True, 1.0)), (1e39, None)])
def test_check_focal_refuses(bad):
    with pytest.raises(ValueError):
        G.check_focal(bad)
    with pytest.raises(ValueError):
        U.sparse_focal_crossentropy(*bad)


def _model():
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone="mobilenetv2", OS=16)


def test_engine_key_carries_gamma_and_alpha():
    model = _model()
    keys = {}
    for name, loss in [("plain", U.sparse_crossentropy_ignoring_last_label), ("none", None),
                       ("off", U.sparse_focal_crossentropy(0.0)), ("ones", U.sparse_focal_crossentropy(0.0, (1, 1, 1))),
                       ("g2", U.sparse_focal_crossentropy(2.0)), ("g1", U.sparse_focal_crossentropy(1.0)),
                       ("g2a", U.sparse_focal_crossentropy(2.0, (0.5, 1.0, 2.0))),
                       ("g2b", U.sparse_focal_crossentropy(2.0, (0.5, 1.0, 3.0))),
                       ("mined", U.sparse_crossentropy_top_k(0.25, 4)), ("jaccard", U.sparse_crossentropy_jaccard(0.5))]:
        model.compile(optimizer=None, loss=loss)
        model._compile_gen = 1   # (compile() counts: the keys are compared across compiles)
        assert model._focal() == getattr(loss, "focal", None)
        keys[name] = model._engine_key(2, True, {"dropout": False})
    # the loss off lowers today's engine: same key, same constructor keywords
    assert keys["off"] == keys["ones"] == keys["plain"] == keys["none"]
    assert all("focal" not in keys[k][1] for k in ("plain", "off", "ones", "mined", "jaccard"))
    assert keys["g2"][1]["focal"] == (2.0, None) and keys["g2a"][1]["focal"] == (2.0, (0.5, 1.0, 2.0))
    assert len({keys[k][0] for k in ("plain", "g2", "g1", "g2a", "g2b", "mined", "jaccard")}) == 7
    # inference engines never carry it; a keyword is normalised, and one that is off disappears
    model.compile(optimizer=None, loss=U.sparse_focal_crossentropy(2.0))
    model._compile_gen = 1
    key, kw = model._engine_key(2, False, {})
    assert "focal" not in kw and key == (2, False, ())
    model.compile(optimizer=None, loss=None)
    model._compile_gen = 1
    assert model._engine_key(2, True, {"dropout": False, "focal": (2, [0.5, 1, 2])}) == keys["g2a"]
    assert model._engine_key(2, True, {"dropout": False, "focal": (0, None)}) == keys["plain"]


def test_focal_with_mining_or_jaccard_is_refused_on_the_host():
    model = _model()
    model.compile(optimizer=None, loss=U.sparse_focal_crossentropy(2.0))
    with pytest.raises(ValueError, match="separate losses"):
        model._engine_key(2, True, {"mining": (0.25, 0)})
    with pytest.raises(ValueError, match="separate losses"):
        model._engine_key(2, True, {"jaccard": 0.5})
    model.compile(optimizer=None, loss=U.sparse_crossentropy_top_k(0.25))
    with pytest.raises(ValueError, match="separate losses"):
        model._engine_key(2, True, {"focal": (2.0, None)})
    # the loss rides a data-parallel engine: distribute() accepts it, in either order
    model.compile(optimizer=None, loss=U.sparse_focal_crossentropy(2.0))
    model._refuse_jaccard_dp(model._compiled["loss"], True)
    assert model._engine_key(2, True, {"external_nnz": True})[1]["focal"] == (2.0, None)


def test_header_and_table_declare_the_four_forms():
    from dl3_amd import capi, head
    from dl3_amd.engine import Engine
    protos = capi.parse_header()
    entries = {"plain": "dl3_focal_xent", "bilinear": "dl3_upsample_focal_xent",
               "bilinear_fold": "dl3_upsample_focal_xent_fold", "shuffle": "dl3_shuffle_focal_xent"}
    assert sorted(head.KERNELS["focal_loss"]) == sorted(entries) == sorted(head.KERNELS["loss"])
    assert sorted(Engine.FOCAL_OPS) == sorted(entries.values())
    n_dims = {"rows": 2, "dims": {"bilinear": 6, "bilinear_fold": 6, "shuffle": 5}}
    for form, (name, slots) in head.KERNELS["focal_loss"].items():
        assert name == entries[form] and name in protos and protos[name][0] == "int"
        args = protos[name][1]
        assert args[-1] == ("void *", "stream")
        assert ("const float *", "alpha") in args and ("float", "gamma") in args
        assert [a for _, a in args[:4]] == [a for _, a in protos[head.KERNELS["loss"][form][0]][1][:4]]
        # the `loss` family's arguments plus alpha and gamma (no probs output)
        assert [s for s in slots if s not in ("alpha", "gamma")] == [s for s in head.KERNELS["loss"][form][1] if s is not None]
        n = sum((n_dims["rows"] if s == "rows" else n_dims["dims"][form] if s == "dims" else 1) for s in slots)
        assert n + 1 == len(args), (form, n, len(args))
    src = open(capi.HEADER).read()
    assert "DESIGN.md §18" in src
