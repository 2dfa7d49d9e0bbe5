"""The soft-Jaccard loss on the host: the oracle's closed-form gradient against torch-CPU autograd of the
definition, the identity with utils.Jaccard that motivates the definition, cases by hand, the loss object, the engine key,
the distribute() refusal and the header."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import graph as G
from dl3_amd import utils as U
from tests import jaccard_oracle as J


def _case(seed=3, B=3, HW=37, C=5):
    """void labels, zero weights, class 1 absent from image 0, class 3 absent everywhere"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, HW, C)) * 2
    t = rng.integers(0, C + 1, (B, HW))
    t[t == 3] = 0
    t[0][t[0] == 1] = 2
    w = rng.uniform(0.5, 2.0, (B, HW)) * (rng.random((B, HW)) > 0.2)
    return z, t, w


def _torch_lj(z, t, w):
    """the definition, term by term, in torch float64"""
    import torch
    C = z.shape[-1]
    p = torch.softmax(z, -1)
    u = ((t < C) & (w != 0)).to(z.dtype)
    y = torch.nn.functional.one_hot(torch.clamp(t, max=C), C + 1)[..., :C].to(z.dtype)
    I = (u[..., None] * p * y).sum(1)
    S = (u[..., None] * p).sum(1)
    Y = (u[..., None] * y).sum(1)
    present = Y > 0
    n_c = present.sum(0)
    legal = n_c > 0
    if not bool(legal.any()):
        return (p * 0).sum()
    Jbc = torch.where(present, I / torch.where(present, S + Y - I, torch.ones_like(S)), torch.zeros_like(S))
    return 1 - (Jbc.sum(0)[legal] / n_c[legal]).mean()


def test_gradient_equals_autograd_of_the_definition():
    """B = 3, HW = 37, C = 5 in float64: the closed form against torch autograd, 1e-12 absolute (measured: below 1e-18)"""
    import torch
    z, t, w = _case()
    s, p, u, ti = J.sums(z, t, w)
    assert (s[:, 3, 2] == 0).all() and s[0, 1, 2] == 0 and (s[1:, 1, 2] > 0).all()      # the case is what it says
    assert (~u).any() and (t == 5).any() and (w == 0).any()
    coef, lj, n_c, n_legal = J.coefficients(s)
    assert n_legal == 4 and n_c.tolist() == [3, 2, 3, 0, 3]
    g = J.gradient(p, u, ti, coef)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    l = _torch_lj(zt, torch.tensor(t), torch.tensor(w))
    l.backward()
    d, lt = float(np.abs(zt.grad.numpy() - g).max()), float(l.detach())
    print("closed form against autograd: %.3e; L_J %.17g against %.17g" % (d, lj, lt))
    assert d <= 1e-12 and abs(lt - lj) <= 1e-12
    assert float(np.abs(g).max()) > 1e-4                                              # not a comparison of zeros
    # the loss object's host evaluation is the same number
    assert abs(U.sparse_crossentropy_jaccard().jaccard_term(t[..., None], p, w) - lj) <= 1e-15


def test_one_hot_prediction_gives_the_hard_jaccard():
    """a one-hot p, no void label, no zero weight: L_J = 1 - utils.Jaccard, exactly"""
    rng = np.random.default_rng(5)
    B, HW, C = 4, 50, 6
    t = rng.integers(0, C - 1, (B, HW))            # class 5 occurs nowhere (dropped by both)
    t[0][t[0] == 2] = 1                            # class 2 is absent from image 0
    pred = np.where(rng.random((B, HW)) < 0.6, t, rng.integers(0, C, (B, HW)))
    p = np.eye(C)[pred]
    hard = U.Jaccard(t[..., None], p)
    assert 0.2 < hard < 0.95
    loss = U.sparse_crossentropy_jaccard()
    assert loss.jaccard_term(t[..., None], p) == 1.0 - hard
    assert loss.jaccard_term(t[..., None], p, np.ones((B, HW))) == 1.0 - hard
    # the oracle from logits that saturate the softmax
    s, _, _, _ = J.sums(np.where(p > 0, 0.0, -1e4), t)
    assert J.coefficients(s)[1] == 1.0 - hard


def test_two_by_two_by_hand():
    """one 2 x 2 image, two classes, all logits equal (p = 1/2 everywhere)"""
    z = np.zeros((1, 4, 2))
    # labels 0 0 1 1: per class I = 1, S = 2, Y = 2, U = 3, J = 1/3 -> L_J = 2/3
    s, p, u, t = J.sums(z, np.array([[0, 0, 1, 1]]))
    assert s.tolist() == [[[1.0, 2.0, 2.0], [1.0, 2.0, 2.0]]]
    coef, lj, n_c, n_legal = J.coefficients(s)
    assert lj == 1.0 - 1.0 / 3.0 and n_legal == 2 and n_c.tolist() == [1, 1]
    # kappa = 1/2: A = -1/6, Bc = (1/2) * 1 / 9
    assert np.allclose(coef, [[[-1 / 6, 1 / 18], [-1 / 6, 1 / 18]]], rtol=1e-15, atol=0)
    # pixel 0 (label 0): G = (A, Bc), sum p G = (A + Bc) / 2 -> g_0 = (A - Bc) / 4 = -1/18, g_1 = +1/18
    g = J.gradient(p, u, t, coef)
    assert np.allclose(g[0, 0], [-1 / 18, 1 / 18], rtol=1e-14, atol=0) and np.allclose(g.sum(-1), 0, atol=1e-17)
    # labels 0 1 void 0 with the last weight zero: u = 1 1 0 0; per class I = 1/2, S = 1, Y = 1, U = 3/2, J = 1/3
    s, p, u, t = J.sums(z, np.array([[0, 1, 2, 0]]), np.array([[1.0, 3.0, 1.0, 0.0]]))
    assert s.tolist() == [[[0.5, 1.0, 1.0], [0.5, 1.0, 1.0]]] and u.tolist() == [[True, True, False, False]]
    coef, lj, _, _ = J.coefficients(s)
    assert lj == 1.0 - 1.0 / 3.0
    g = J.gradient(p, u, t, coef)
    assert (g[0, 2:] == 0).all() and (g[0, :2] != 0).all()
    # a perfect one-hot prediction: J = 1, L_J = 0, and the gradient vanishes with p (1 - p)
    zs = np.where(np.eye(2)[[0, 0, 1, 1]] > 0, 0.0, -1e4)[None]
    s, p, u, t = J.sums(zs, np.array([[0, 0, 1, 1]]))
    coef, lj, _, _ = J.coefficients(s)
    assert lj == 0.0 and (J.gradient(p, u, t, coef) == 0).all()


def test_absent_classes_and_the_all_void_batch():
    z, t, w = _case()
    s, p, u, ti = J.sums(z, t, w)
    coef, lj, n_c, n_legal = J.coefficients(s)
    # a class absent from one image has no coefficients there, a class absent everywhere has none at all
    assert (coef[0, 1] == 0).all() and (coef[:, 3] == 0).all() and (coef[1:, 1] != 0).all()
    assert (coef[..., 0] <= 0).all() and (coef[..., 1] >= 0).all() and 0 < lj < 1
    # the gradient of every pixel sums to zero over the classes (softmax) and is zero where u = 0
    g = J.gradient(p, u, ti, coef)
    assert np.abs(g.sum(-1)).max() < 1e-17 and (g[~u] == 0).all() and (g[u] != 0).any()
    for tv, wv in ((np.full(t.shape, 5), w), (t, np.zeros_like(w))):
        s, p, u, ti = J.sums(z, tv, wv)
        coef, lj, n_c, n_legal = J.coefficients(s)
        assert (s == 0).all() and lj == 0.0 and n_legal == 0 and (coef == 0).all()
        assert (J.gradient(p, u, ti, coef) == 0).all()
        r = J.evaluate("plain", z[:, None], None, tv, wv, lam=2.0)
        assert r["lj"] == 0.0 and r["loss"] == r["ce"] and (r["dj"] == 0).all()
        assert U.sparse_crossentropy_jaccard().jaccard_term(tv[..., None], p, wv) == 0.0


def test_float32_yardstick_follows_the_contract():
    """per-pixel float32, sums in float64, coefficients rounded once: close to the reference, not equal to it"""
    z, t, w = _case()
    a = J.evaluate("plain", z[:, None].astype(np.float32), None, t, w.astype(np.float32), 0.5, np.float64)
    b = J.evaluate("plain", z[:, None].astype(np.float32), None, t, w.astype(np.float32), 0.5, np.float32)
    assert b["sums"].dtype == np.float64 and b["coef"].dtype == np.float32 and b["dlogits"].dtype == np.float32
    assert np.array_equal(a["sums"][..., 2], b["sums"][..., 2])
    assert 0 < np.abs(a["sums"] - b["sums"]).max() < 1e-5
    assert np.array_equal(b["coef"], J.coefficients(b["sums"])[0].astype(np.float32))
    assert 0 < np.abs(a["dlogits"] - b["dlogits"]).max() < 1e-6
    assert a["loss"] == a["ce"] + 0.5 * a["lj"]


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf"), "1", None, True, 1e39, [1.0]])
def test_loss_object_refuses(bad):
    if bad is None:
        assert G.check_jaccard(None) is None
        with pytest.raises((ValueError, TypeError)):
            U.sparse_crossentropy_jaccard(None)
        return
    with pytest.raises(ValueError):
        U.sparse_crossentropy_jaccard(bad)


def test_loss_object():
    l = U.sparse_crossentropy_jaccard()
    assert l.jaccard == 1.0 and l.jaccard_weight == 1.0
    assert U.sparse_crossentropy_jaccard(0.25).jaccard == 0.25 and U.sparse_crossentropy_jaccard(np.float32(2)).jaccard == 2.0
    assert U.sparse_crossentropy_jaccard(0).jaccard is None and U.sparse_crossentropy_jaccard(0.0).jaccard_weight == 0.0
    assert l.__name__ == "sparse_crossentropy_jaccard" and repr(U.sparse_crossentropy_jaccard(0.25)) == \
        "sparse_crossentropy_jaccard(0.25)"
    rng = np.random.default_rng(0)
    p = rng.uniform(0.1, 1.0, (2, 7, 3))
    y = rng.integers(0, 4, (2, 7, 1)).astype(np.float32)
    assert np.array_equal(l(y, p), U.sparse_crossentropy_ignoring_last_label(y, p))


def _model():
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    return Deeplabv3(weights=None, input_shape=(64, 64, 3), classes=3, backbone="mobilenetv2", OS=16)


def test_engine_key_carries_the_jaccard_weight():
    model = _model()
    keys = {}
    for name, loss in [("plain", U.sparse_crossentropy_ignoring_last_label), ("none", None),
                       ("zero", U.sparse_crossentropy_jaccard(0.0)), ("a", U.sparse_crossentropy_jaccard(1.0)),
                       ("b", U.sparse_crossentropy_jaccard(0.5)), ("mined", U.sparse_crossentropy_top_k(0.25, 4))]:
        model.compile(optimizer=None, loss=loss)
        model._compile_gen = 1            # the compile counter is part of every key: hold it still
        keys[name] = model._engine_key(2, True, {"dropout": False})
    # jaccard_weight == 0 (and any other loss) lowers today's engine: same key, same constructor keywords
    assert keys["zero"] == keys["plain"] == keys["none"]
    assert "jaccard" not in keys["plain"][1] and "jaccard" not in keys["mined"][1]
    assert keys["a"][1]["jaccard"] == 1.0 and keys["b"][1]["jaccard"] == 0.5 and "mining" not in keys["a"][1]
    assert len({keys[n][0] for n in ("plain", "a", "b", "mined")}) == 4
    # inference engines never carry it
    model.compile(optimizer=None, loss=U.sparse_crossentropy_jaccard(1.0))
    key, kw = model._engine_key(2, False, {})
    assert "jaccard" not in kw and key == (2, False, ())


class _NoComm:
    """stands where a parallel.DataParallel would: the refusal must come before anything touches it"""

    def __getattr__(self, name):
        raise AssertionError("the communicator was used: %s" % name)


def test_distribute_refuses_the_loss_in_either_order():
    model = _model()
    model.compile(optimizer=None, loss=U.sparse_crossentropy_jaccard(1.0))
    with pytest.raises(ValueError, match="distribute"):
        model.distribute(_NoComm())
    with pytest.raises(ValueError, match="distribute"):
        model.distribute()                # refused before a process group is looked for
    assert model._dp is None
    # the other order
    model = _model()
    model.compile(optimizer=None, loss=U.sparse_crossentropy_ignoring_last_label)
    dp = _NoComm()
    model.distribute(dp)
    with pytest.raises(ValueError, match="distribute"):
        model.compile(optimizer=None, loss=U.sparse_crossentropy_jaccard(0.5))
    assert model._compiled["loss"] is U.sparse_crossentropy_ignoring_last_label      # the refused compile changed nothing
    # the term switched off is the plain loss: nothing to refuse
    model.compile(optimizer=None, loss=U.sparse_crossentropy_jaccard(0.0))
    assert model._dp is dp


def test_header_exports():
    from dl3_amd import capi
    from dl3_amd import head
    protos = capi.parse_header()
    names = ["dl3_jaccard_partials", "dl3_jaccard_loss_partials", "dl3_jaccard_sums_plain", "dl3_jaccard_sums_bilinear",
             "dl3_jaccard_coef", "dl3_softmax_xent_jaccard", "dl3_upsample_softmax_xent_jaccard"]
    for n in names:
        assert n in protos, n
        assert all(t in capi._CTYPES for t, _ in protos[n][1]), n
    assert [t for t, _ in protos["dl3_jaccard_coef"][1]][:5] == ["const double *", "int", "int", "int", "float"]
    # the head's table names them, with as many slots as the prototype has arguments (the stream comes last)
    for family in ("jaccard_sums", "jaccard_loss"):
        assert sorted(head.KERNELS[family]) == ["bilinear", "plain"]
        for form, (name, slots) in head.KERNELS[family].items():
            n_dims = {"images": 3, "dims": 6}
            n = sum(n_dims.get(s, 1) for s in slots)
            assert n + 1 == len(protos[name][1]), (family, form)
