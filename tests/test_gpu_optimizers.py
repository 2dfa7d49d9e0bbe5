"""-m gpu: the optimizer step beyond plain Adam — dl3_grad_sumsq and dl3_opt_step through the C ABI against the float64
restatement in tests/optim_oracle.py (bounds: tests/ops_oracle.py), Engine.opt_step on given gradients, and SGD / RMSprop
/ clipping / LearningRateScheduler through Model.compile, train_on_batch and fit_generator.

Roundings are counted as in tests/test_gpu_ops_edges.py (Adam there: p 12, m 4, v 6 for a gradient that carries one
rounding).  Here the effective gradient g' carries r_g roundings relative to itself:
  g * sc                                  1
  sc = gs / max(denom, 1e-20)            +1  (the quotient is rounded before it multiplies)
  clipping engaged: * (clipnorm / norm)  +4  (the product; norm = sc * float(sqrt(sumsq)): 2; the quotient: 1)
  the clamp is exact and 1-Lipschitz      0
and per rule, on the magnitudes optim_oracle returns:
  SGD      v = c0*m - lr*g': (r_g + 1) + 1 = r_g + 2;  p: nesterov c0*v (r_g + 3), lr*g', two adds: r_g + 5
  RMSprop  a: g'^2 (2 r_g + 1), 1 - rho, product, rho*a || add: 2 r_g + 4
           p: numerator r_g + 1; denominator a halved by the root (r_g + 2), sqrtf, + eps: r_g + 4; /, p - u: 2 r_g + 7
  Adam     m: r_g + 3;  v: 2 r_g + 4;  p: (r_g + 3) + (r_g + 2 + 2) + 3 = 2 r_g + 10      (r_g = 1: 4, 6, 12)"""
import math

import numpy as np
import pytest
import torch

from oracle import dl3_oracle as O
from tests import ops_oracle as OO
from tests import optim_oracle as PO
from tests.gpu_util import call, dev, host, ptr, release

pytestmark = pytest.mark.gpu

NS = [1, 5, 1027, 1048576 + 777]   # the last: beyond one pass of a 4096 x 256 grid (test_adam_step_grid_stride_loop's n)


@pytest.fixture(scope="module")
def L():
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    return capi.lib()


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for fam in sorted(OO.RATIOS):
        print("\nworst error / bound, %-22s %.3f" % (fam, OO.RATIOS[fam]), end="")
    print()


# ================================================================================================== dl3_grad_sumsq
def _f64(value=0.0, n=1):
    return torch.full((n,), value, dtype=torch.float64, device="cuda")


def _sumsq(L, g_dev, off, n, ws=None):
    from dl3_amd import capi
    need = int(L.dl3_grad_sumsq_workspace_bytes(n))
    ws = _f64(float("nan"), (need + 7) // 8 + 3) if ws is None else ws
    out = _f64(float("nan"), 3)   # [guard, result, guard]
    capi.call("dl3_grad_sumsq", ptr(g_dev, off), n, out.data_ptr() + 8, ws.data_ptr(), need,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2])                       # one double is written
    assert np.isnan(ws.cpu().numpy()[(need + 7) // 8:]).all()      # nothing behind the promised workspace
    return o[1:2].copy()


@pytest.fixture(scope="module")
def sumsq_values():
    rng = np.random.default_rng(2201)
    n = NS[-1] + 1
    return (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_grad_sumsq_matches_float64_and_repeats_bit_for_bit(L, sumsq_values, n, off):
    """values over 1e-6 .. 1e3; off = 1: the pointer is one float past a 16-byte boundary, so the 16-byte loads must give way
    to the scalar loop; n % 4 != 0 takes the scalar tail.  Accumulated in double: 1e-12 of the exact sum (math.fsum).  Two
    launches give the same 64 bits."""
    g = sumsq_values
    gd = dev(g)
    assert gd.data_ptr() % 16 == 0
    a = _sumsq(L, gd, off, n)
    b = _sumsq(L, gd, off, n)
    want = math.fsum(float(v) * float(v) for v in g[off:off + n].astype(np.float64))
    rel = abs(float(a[0]) - want) / want
    print("grad_sumsq n=%d off=%d rel err %.3e" % (n, off, rel))
    assert rel <= 1e-12
    assert a.view(np.uint64)[0] == b.view(np.uint64)[0]


def test_grad_sumsq_short_workspace_is_the_workspace_error(L, sumsq_values):
    from dl3_amd import capi
    n = NS[-1]
    gd, out = dev(sumsq_values), _f64(-1.0, 1)
    need = int(L.dl3_grad_sumsq_workspace_bytes(n))
    ws = _f64(0.0, need // 8)
    for short_ptr, short_bytes in ((ws.data_ptr(), need - 8), (ws.data_ptr(), 0), (None, need)):
        rc = L.dl3_grad_sumsq(ptr(gd), n, out.data_ptr(), short_ptr, short_bytes, None)
        assert rc == -3, rc                                        # DL3_EWORKSPACE
        assert b"workspace" in L.dl3_last_error()
    with pytest.raises(capi.DL3Error, match="rc=-3"):
        capi.call("dl3_grad_sumsq", ptr(gd), n, out.data_ptr(), ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == -1.0                             # nothing was launched


# ==================================================================================================== dl3_opt_step
HYP = dict(lr_t=1e-3, c0=0.9, c1=0.999)
RULES = {   # name -> (rule id, nesterov, eps)
    "sgd": (0, 0, 0.0), "sgd_nesterov": (0, 1, 0.0), "rmsprop": (1, 0, 1e-7), "adam": (2, 0, 1e-8)}
CLIPS = ["none", "clipnorm_above", "clipnorm_below", "clipvalue", "both"]
SCALES = {"plain": (0.5, None), "denom": (0.5, 1234.0), "denom_zero": (0.5, 0.0)}


@pytest.fixture(scope="module")
def step_inputs():
    rng = np.random.default_rng(2202)
    n = NS[-1]
    return dict(p=rng.normal(0, 1, n).astype(np.float32), g=rng.normal(0, 1, n).astype(np.float32),
                s0=rng.normal(0, 0.1, n).astype(np.float32), s1=rng.uniform(0, 0.1, n).astype(np.float32))


def _slots(inputs, rule, n):
    """p, slot 0, slot 1 of a step in flight: RMSprop's accumulator is a mean of squares, never negative"""
    s0 = inputs["s0"][:n]
    return inputs["p"][:n], (np.abs(s0) if rule == "rmsprop" else s0), inputs["s1"][:n]


def _clip_settings(clip, g, gs, denom):
    """(clipnorm, clipvalue, does the norm clip) placed a factor 4 off the norm of the SCALED gradient: the decision cannot
    flip on a rounding"""
    sc = gs if denom is None else gs / max(denom, 1e-20)
    norm = sc * math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    if norm == 0.0:   # zero gradients under the floored denominator
        return {"none": (0.0, 0.0, False), "clipnorm_above": (1.0, 0.0, False), "clipnorm_below": (1e-3, 0.0, False),
                "clipvalue": (0.0, 1.0, False), "both": (1e-3, 1.0, False)}[clip]
    rms = norm / math.sqrt(g.size)
    return {"none": (0.0, 0.0, False), "clipnorm_above": (4.0 * norm, 0.0, False), "clipnorm_below": (0.25 * norm, 0.0, True),
            "clipvalue": (0.0, 0.5 * rms, False), "both": (0.25 * norm, 0.1 * rms, True)}[clip]


def _opt_call(L, rule, n, p, g, s0, s1, gs, denom, clipnorm, clipvalue, lead=0):
    """dl3_grad_sumsq (when clipnorm is on) + dl3_opt_step as the engine issues them; p / s0 / s1 live in sentinel-guarded
    buffers; lead = 1 puts every array one float past a 16-byte boundary (the scalar kernel)"""
    import ctypes
    from dl3_amd import capi
    rid, nesterov, eps = RULES[rule]
    bufs = []
    for a in (p, s0, s1):
        b = OO.guard_buffer(n, 1, lead=lead)
        b[lead:lead + n] = a
        bufs.append(dev(b))
    gd = dev(np.concatenate([np.zeros(lead, np.float32), g]))
    sumsq = None
    if clipnorm > 0:
        sumsq = _f64(float("nan"), 1)
        need = int(L.dl3_grad_sumsq_workspace_bytes(n))
        ws = _f64(0.0, (need + 7) // 8)
        call("dl3_grad_sumsq", ptr(gd, lead), n, sumsq.data_ptr(), ws.data_ptr(), need)
    h = capi.OptHyper(HYP["lr_t"], HYP["c0"], HYP["c1"], eps, gs, clipnorm, clipvalue, nesterov)
    call("dl3_opt_step", ptr(bufs[0], lead), ptr(gd, lead), ptr(bufs[1], lead), ptr(bufs[2], lead) if rid == 2 else None, n,
         rid, ctypes.byref(h), None if denom is None else ptr(dev(np.array([denom], np.float32))),
         None if sumsq is None else sumsq.data_ptr())
    outs = []
    for b in bufs:
        hb = host(b)
        OO.assert_guard(hb, lead + np.arange(n))
        outs.append(hb[lead:lead + n])
    release()
    return outs


def _oracle(rule, p, g, s0, s1, gs, denom, clipnorm, clipvalue, clips):
    """-> [(device output index, expected, magnitude, roundings)]"""
    rid, nesterov, eps = RULES[rule]
    ge = PO.effective_gradient(g, gs, denom, clipnorm, clipvalue)
    rg = 1 + (denom is not None) + 4 * bool(clips)
    if rid == 0:
        (rp, rv), (mp, mv) = PO.sgd(p, ge, s0, HYP["lr_t"], HYP["c0"], bool(nesterov))
        return [(0, rp, mp, rg + 5), (1, rv, mv, rg + 2)]
    if rid == 1:
        (rp, ra), (mp, ma) = PO.rmsprop(p, ge, s0, HYP["lr_t"], HYP["c0"], eps)
        return [(0, rp, mp, 2 * rg + 7), (1, ra, ma, 2 * rg + 4)]
    (rp, rm, rv), (mp, mm, mv) = PO.adam(p, ge, s0, s1, HYP["lr_t"], HYP["c0"], HYP["c1"], eps)
    return [(0, rp, mp, 2 * rg + 10), (1, rm, mm, rg + 3), (2, rv, mv, 2 * rg + 4)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("rule", list(RULES))
def test_opt_step_follows_the_oracle(L, step_inputs, rule, clip, scale, n):
    """every rule x clip setting x scale form at n = 1 (one live lane), 5 (one 16-byte trip + a scalar tail), 1027 and
    1 049 353 (grid-stride); denom = 0 takes the 1e-20 floor with zero gradients, as in
    test_adam_step_norm_denominator_and_floor.  The unused slot of a one-slot rule is not touched (its guard buffer holds
    the input)."""
    gs, denom = SCALES[scale]
    p, s0, s1 = _slots(step_inputs, rule, n)
    g = np.zeros(n, np.float32) if scale == "denom_zero" else step_inputs["g"][:n]
    clipnorm, clipvalue, clips = _clip_settings(clip, g, gs, denom)
    got = _opt_call(L, rule, n, p, g, s0, s1, gs, denom, clipnorm, clipvalue)
    for i, ref, mag, rd in _oracle(rule, p, g, s0, s1, gs, denom, clipnorm, clipvalue, clips):
        OO.assert_elementwise(got[i], ref, mag, rd, "opt_step " + rule.split("_")[0])
    if RULES[rule][0] != 2:
        assert np.array_equal(got[2], s1)
    if clip == "clipnorm_below" and scale == "plain" and rule == "sgd" and n >= 1027:
        # the clipped gradient has norm clipnorm: v = c0*m - lr*g' gives it back.  (Only where g' is of the size of m / lr:
        # under the denom forms g' is 1e-4 and the difference c0*m - v cancels down to the rounding of v.)
        ge = (HYP["c0"] * s0.astype(np.float64) - got[1].astype(np.float64)) / HYP["lr_t"]
        assert abs(np.linalg.norm(ge) - clipnorm) <= 1e-4 * clipnorm


@pytest.mark.parametrize("rule", list(RULES))
def test_opt_step_unaligned_pointers_take_the_scalar_kernel(L, step_inputs, rule):
    """every array one float past a 16-byte boundary (n = 1027, clipping and clamp on): the same values as the aligned launch
    to the oracle's bound, nothing outside [0, n) written"""
    n, gs = 1027, 0.5
    (p, s0, s1), g = _slots(step_inputs, rule, n), step_inputs["g"][:n]
    clipnorm, clipvalue, clips = _clip_settings("both", g, gs, None)
    got = _opt_call(L, rule, n, p, g, s0, s1, gs, None, clipnorm, clipvalue, lead=1)
    for i, ref, mag, rd in _oracle(rule, p, g, s0, s1, gs, None, clipnorm, clipvalue, clips):
        OO.assert_elementwise(got[i], ref, mag, rd, "opt_step " + rule.split("_")[0])


@pytest.mark.parametrize("n", NS)
def test_opt_step_adam_with_a_far_clipnorm_is_adam_step(L, step_inputs, n):
    """Adam through dl3_opt_step with clipnorm far above the norm (nothing clips) against dl3_adam_step on the same inputs:
    fp32 rounding apart (both evaluate the same expression; the bound is the oracle's for either)"""
    p, g, s0, s1 = (step_inputs[k][:n] for k in ("p", "g", "s0", "s1"))
    got = _opt_call(L, "adam", n, p, g, s0, s1, 0.5, None, 1e30, 0.0)
    bufs = [dev(a.copy()) for a in (p, s0, s1)]
    call("dl3_adam_step", ptr(bufs[0]), ptr(dev(g)), ptr(bufs[1]), ptr(bufs[2]), n, HYP["lr_t"], HYP["c0"], HYP["c1"],
         RULES["adam"][2], 0.5)
    for (i, ref, mag, rd), b in zip(_oracle("adam", p, g, s0, s1, 0.5, None, 0.0, 0.0, False), bufs):
        OO.assert_elementwise(got[i], host(b).astype(np.float64), mag, rd, "opt_step adam")
        OO.assert_elementwise(got[i], ref, mag, rd, "opt_step adam")


def test_opt_step_refuses_bad_arguments(L):
    import ctypes
    from dl3_amd import capi
    t = dev(np.zeros(8, np.float32))
    h = capi.OptHyper(1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, 0.0, 0)
    assert L.dl3_opt_step(ptr(t), ptr(t), ptr(t), None, 8, 2, ctypes.byref(h), None, None, None) == -1     # Adam, one slot
    assert L.dl3_opt_step(ptr(t), ptr(t), ptr(t), ptr(t), 8, 7, ctypes.byref(h), None, None, None) == -1   # unknown rule
    h.clipnorm = 1.0
    assert L.dl3_opt_step(ptr(t), ptr(t), ptr(t), None, 8, 0, ctypes.byref(h), None, None, None) == -1     # clipnorm, no norm
    torch.cuda.synchronize()
    assert not host(t).any()


# ========================================================================================================== engine
def _build(backbone="mobilenetv2", input_shape=(64, 64, 3), classes=3):
    import dl3_amd  # noqa: F401
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    G.clear_session()
    model = Deeplabv3(weights=None, input_shape=input_shape, classes=classes, backbone=backbone, OS=16)
    params = O.init_params(O.param_shapes(backbone, classes, head="deeplab"), seed=1)
    for l in model.layers:
        if l.weights:
            l.set_weights([params[n] for n in l.weights])
    return model


def _batch(B, seed, classes=3, side=64):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (B, side, side, 3)).astype(np.float32)
    y = rng.integers(0, classes, (B, side * side, 1)).astype(np.float32)
    return x, y


def _np64(t, n):
    return t[:n].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("backbone", ["mobilenetv2", "xception"])
def test_arena_padding_has_exactly_zero_gradients(backbone):
    """the global norm runs over the whole gradient arena [0, n_param): the channels _dshape pads (Xception's 728-channel
    tensors are stored 736 wide; MobileNetV2 pads none) and the gaps that round a slot to 4 floats must hold exact zeros after
    a backward pass, or clipnorm would see them"""
    model = _build(backbone)
    eng = model._engine(2, True, dropout=False, use_graph=False)
    x, y = _batch(2, 40)
    eng.set_input(x)
    eng.set_targets(y[:, :, 0], np.ones(y.shape[:2], np.float32))
    eng.fwd_bwd()
    torch.cuda.synchronize()
    g = eng.grads.cpu().numpy()
    pad = np.ones(eng.n_param, bool)
    n_padded = 0
    for name, (kind, off, size, dshape, _) in eng.slots.items():
        if kind != "p":
            continue
        m = np.ones(dshape, bool)
        m[tuple(slice(0, k) for k in eng.hshape[name])] = False
        n_padded += int(m.sum())
        pad[off:off + size] = m.reshape(-1)
    print("arena: %d floats, %d of them padding (%d padded channels' worth)" % (eng.n_param, int(pad.sum()), n_padded))
    assert pad.any() and (n_padded > 0 or backbone != "xception") and np.abs(g[:eng.n_param][~pad]).max() > 0
    assert not g[:eng.n_param][pad].any(), "%d padding elements carry a gradient" % np.count_nonzero(g[:eng.n_param][pad])


ENGINE_CASES = {
    "sgd_nesterov": dict(rule="sgd", hyper=dict(lr=0.01, momentum=0.9, decay=0.5, nesterov=True)),
    "sgd_clipped": dict(rule="sgd", hyper=dict(lr=0.01, momentum=0.9, decay=0.5), clipnorm="half", clipvalue=1.0),
    "rmsprop": dict(rule="rmsprop", hyper=dict(lr=1e-3, rho=0.9, epsilon=1e-7, decay=0.5)),
    "rmsprop_clipped": dict(rule="rmsprop", hyper=dict(lr=1e-3, rho=0.95, epsilon=1e-4, decay=0.5), clipnorm="half"),
    "adam_clipped": dict(rule="adam", hyper=dict(lr=1e-3, decay=0.5, epsilon=1e-4, beta_1=0.8, beta_2=0.99),
                         clipnorm="half", clipvalue=1.0),
}


@pytest.fixture(scope="module")
def engine_model():
    return _build()


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_opt_step_follows_the_oracle_on_given_gradients(engine_model, case):
    """Engine.opt_step — the host half (decay on the iteration count BEFORE the increment, Adam's bias correction) +
    dl3_grad_sumsq + dl3_opt_step — over FOUR steps on gradients handed in (magnitudes 1e-9 .. 1e+1), against
    optim_oracle.keras_step in float64 on the same numbers.  What separates the two is fp32: the hyper-parameters as floats
    (lr_t 6e-8; 1 - 0.9f is 2.4e-7 off 0.1; 1 - 0.99f 1e-6 off) and at most 17 roundings per step — under 4e-6 of the terms
    of one step, summed over four steps; the bars are 1e-5 of the summed step sizes for SGD / RMSprop and, as in
    test_engine_adam_follows_the_oracle_on_given_gradients, 1e-4 for Adam, plus the fp32 representation of the weight: every
    add onto the weight rounds once at 2**-24 (6e-8) of the weight — one add per step, two with nesterov (p + c0*v, - lr*g')."""
    desc = dict(ENGINE_CASES[case])
    rule, hyper = desc["rule"], desc["hyper"]
    eng = engine_model._engine(2, True, dropout=False, use_graph=False)
    n = eng.n_param
    rng = np.random.default_rng(31)
    scale = 10.0 ** rng.uniform(-9, 1, n)
    gs = [(rng.normal(0, 1, n) * scale).astype(np.float32) for _ in range(4)]
    if desc.get("clipnorm") == "half":   # half the smallest of the four norms: every step clips, none is near the edge
        desc["clipnorm"] = 0.5 * min(float(np.linalg.norm(g.astype(np.float64))) for g in gs)
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.iteration = 0
    p0 = _np64(eng.params, n)
    p, s0, s1, steps = p0.copy(), np.zeros(n), np.zeros(n), np.zeros(n)
    for it, g in enumerate(gs):
        eng.grads[:n].copy_(torch.from_numpy(g).cuda())
        eng.opt_step(desc, 1.0)
        q, s0, s1 = PO.keras_step(rule, p, g, s0, s1, it, clipnorm=desc.get("clipnorm", 0.0),
                                  clipvalue=desc.get("clipvalue", 0.0), **hyper)
        ge = PO.effective_gradient(g, clipnorm=desc.get("clipnorm", 0.0), clipvalue=desc.get("clipvalue", 0.0))
        steps += np.abs(q - p) if rule != "sgd" else np.abs(s0) + hyper["lr"] * np.abs(ge)   # SGD: the terms of v
        p = q
    torch.cuda.synchronize()
    assert eng.iteration == 4
    bar = 1e-4 if rule == "adam" else 1e-5
    adds = 4 * (2 if hyper.get("nesterov") else 1)
    gp, g0, g1 = _np64(eng.params, n), _np64(eng.adam_m, n), _np64(eng.adam_v, n)
    assert np.all(np.abs(gp - p) <= adds * 6e-8 * np.maximum(np.abs(p), np.abs(p0)) + bar * steps)
    if rule == "sgd":
        assert np.all(np.abs(g0 - s0) <= bar * steps)
    elif rule == "rmsprop":
        assert np.all(np.abs(g0 - s0) <= bar * s0 + 1e-37)
    else:
        assert np.abs(g0 - s0).max() <= 1e-6 * np.abs(s0).max()
    if rule == "adam":
        assert np.all(np.abs(g1 - s1) <= bar * s1 + 1e-37)
    else:
        assert not g1.any()                                       # slot 1 is not touched by the one-slot rules
    # the schedule is visible: replaying with `it` taken AFTER the increment moves the weights by more than the bar
    q = p0.copy()
    z0, z1 = np.zeros(n), np.zeros(n)
    for it, g in enumerate(gs):
        q, z0, z1 = PO.keras_step(rule, q, g, z0, z1, it + 1, clipnorm=desc.get("clipnorm", 0.0),
                                  clipvalue=desc.get("clipvalue", 0.0), **hyper)
    assert np.any(np.abs(q - p) > 100 * (adds * 6e-8 * np.maximum(np.abs(p), np.abs(p0)) + bar * steps))
    eng.params[:n].copy_(torch.from_numpy(p0.astype(np.float32)).cuda())
    eng.dirty = True


@pytest.mark.parametrize("rule", ["sgd", "rmsprop", "adam"])
def test_data_parallel_form_clips_the_normalised_gradient(engine_model, rule):
    """an external_nnz engine (the data-parallel step on one GPU), its gradient arena and the count in the arena's tail
    filled by hand: sc = c0 / count on the device, and the norm clipnorm sees is that of g * sc.  Against the plain engine
    handed g * sc (the same fp32 product) with scale 1: the two differ by the roundings of the norm only (1e-6 of the
    step).  clipnorm is half the NORMALISED norm; a norm taken from the raw arena (10 000 x larger) would shrink the step
    10 000-fold, which the float64 replay of SGD's buffer below would show."""
    hyper = dict(sgd=dict(lr=0.01, momentum=0.9, decay=0.1), rmsprop=dict(lr=1e-3, decay=0.1),
                 adam=dict(lr=1e-3, decay=0.1, epsilon=1e-8))[rule]
    model = engine_model
    ext = model._engine(2, True, dropout=False, use_graph=False, external_nnz=True)
    n = ext.n_param
    rng = np.random.default_rng(77)
    g = rng.normal(0, 1, n).astype(np.float32)
    count = 1.0e4 * ext.nnz_host                      # sc = 1e-4: the raw norm is 10 000 x the normalised one
    sc32 = np.float32(ext.nnz_host) / np.float32(count)
    norm = float(sc32) * float(np.linalg.norm(g.astype(np.float64)))
    desc = dict(rule=rule, hyper=hyper, clipnorm=0.5 * norm)
    p0 = ext.params.clone()
    with pytest.raises(ValueError):
        ext.opt_step(desc, 1.0, norm=False)           # the refusal holds for every rule
    results = []
    for eng, grad, kw in ((ext, g, {}), (None, g * sc32, dict(grad_scale=1.0))):
        if eng is None:
            eng = model._engine(2, True, dropout=False, use_graph=False)
        eng.params.copy_(p0)
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.iteration = 0
        for _ in range(2):
            eng.grads.zero_()
            eng.grads[:n].copy_(torch.from_numpy(grad).cuda())
            if eng.external_nnz:
                eng.grads[eng.tail] = count
            eng.opt_step(desc, **kw)
        torch.cuda.synchronize()
        results.append((_np64(eng.params, n), _np64(eng.adam_m, n)))
        eng.params.copy_(p0)
        eng.dirty = True
    (pe, me), (pp, mp) = results
    step = np.abs(pp - _np64(p0, n))
    assert step.max() > 0
    assert np.all(np.abs(pe - pp) <= 2 * 6e-8 * np.abs(pp) + 1e-5 * step.max())
    assert np.all(np.abs(me - mp) <= 1e-5 * np.abs(mp).max())
    # and it is the clipped, normalised gradient: SGD's first-step buffer has norm lr * clipnorm ... checked on two steps
    if rule == "sgd":
        want = PO.keras_step("sgd", np.zeros(n), g, np.zeros(n), None, 0, clipnorm=desc["clipnorm"], gs=float(sc32), **hyper)[1]
        want = PO.keras_step("sgd", np.zeros(n), g, want, None, 1, clipnorm=desc["clipnorm"], gs=float(sc32), **hyper)[1]
        assert np.all(np.abs(me - want) <= 1e-5 * np.abs(want).max())


# =========================================================================================================== model
def test_train_on_batch_sgd_without_momentum_is_w_minus_lr_g():
    from dl3_amd.optimizers import SGD
    model = _build()
    x, y = _batch(2, 41)
    lr = 0.05
    model.compile(optimizer=SGD(lr=lr, momentum=0.0))
    eng = model._engine(2, True, dropout=False)
    n = eng.n_param
    before = _np64(eng.params, n)
    model.train_on_batch(x, y, dropout=False)
    assert model._active is eng and eng.iteration == 1
    after, g = _np64(eng.params, n), _np64(eng.grads, n)
    assert np.abs(g).max() > 0
    # v = 0*m - lr*g (lr as a float: 6e-8; the product: 1 rounding), p + v (1 rounding): 2 x the oracle's factor 2
    lr32 = float(np.float32(lr))
    assert np.all(np.abs(after - (before - lr32 * g)) <= 4 * OO.U * (np.abs(before) + lr32 * np.abs(g)))
    assert np.all(np.abs(_np64(eng.adam_m, n) + lr32 * g) <= 2 * OO.U * lr32 * np.abs(g))   # the buffer: v = -lr g


def test_three_train_on_batch_steps_with_nesterov_momentum_replay_in_float64():
    """three steps on three batches with SGD(momentum=0.9, nesterov=True, decay): replayed in float64 from the gradients the
    engine holds after each step.  Per step at most 6 roundings and the fp32 hyper-parameters (6e-8 each) on terms the size
    of |v| + lr |g|: 1e-6 of their sum over the steps, plus the fp32 representation of the weight — with nesterov two adds
    onto the weight per step (p + c0*v, - lr*g), each rounding once at 2**-24 (6e-8) of the weight: 6 over the three steps"""
    from dl3_amd.optimizers import SGD
    model = _build()
    hyper = dict(lr=0.02, momentum=0.9, decay=0.25, nesterov=True)
    model.compile(optimizer=SGD(**hyper))
    eng = model._engine(2, True, dropout=False)
    n = eng.n_param
    p0 = _np64(eng.params, n)
    p, m, terms = p0.copy(), np.zeros(n), np.zeros(n)
    for it in range(3):
        x, y = _batch(2, 50 + it)
        model.train_on_batch(x, y, dropout=False)
        g = _np64(eng.grads, n)
        p, m, _ = PO.keras_step("sgd", p, g, m, None, it, **hyper)
        terms += np.abs(m) + hyper["lr"] * np.abs(g)
    assert eng.iteration == 3
    gp, gm = _np64(eng.params, n), _np64(eng.adam_m, n)
    err = np.abs(gp - p)
    bound = 6 * 6e-8 * np.maximum(np.abs(p), np.abs(p0)) + 1e-6 * terms
    print("nesterov replay: worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert np.all(np.abs(gm - m) <= 1e-6 * terms)
    assert np.any(np.abs(p - p0) > 1e3 * bound)   # the steps are far above the bar


def test_train_on_batch_clipnorm_limits_the_applied_update():
    """SGD(lr, clipnorm=c) with c below the measured norm: the update that reaches the weights has global norm lr * c"""
    from dl3_amd.optimizers import SGD
    model = _build()
    x, y = _batch(2, 42)
    model.compile(optimizer=SGD(lr=0.0))              # a step that moves nothing: measures the gradient norm
    model.train_on_batch(x, y, dropout=False)
    e0 = model._active
    norm = float(np.linalg.norm(_np64(e0.grads, e0.n_param)))
    assert norm > 0
    lr, c = 0.1, 0.5 * norm
    model.compile(optimizer=SGD(lr=lr, clipnorm=c))
    eng = model._engine(2, True, dropout=False)
    n = eng.n_param
    before = _np64(eng.params, n)
    model.train_on_batch(x, y, dropout=False)
    assert model._active is eng and eng is not e0
    upd = np.linalg.norm(_np64(eng.params, n) - before)
    print("clipnorm: gradient norm %.6g, c %.6g, update norm / (lr c) - 1 = %.3e" % (norm, c, upd / (lr * c) - 1))
    assert abs(upd - lr * c) <= 1e-5 * lr * c
    assert abs(float(np.linalg.norm(_np64(eng.grads, n))) - norm) <= 1e-3 * norm    # the same gradient was clipped


# =========================================================================================================== state
def test_sgd_momentum_survives_a_batch_size_change():
    """as test_optimizer_state_survives_a_batch_size_change for Adam: the last, smaller batch continues the momentum"""
    from dl3_amd.optimizers import SGD
    model = _build()
    x, y = _batch(4, 8)
    lr = 0.01
    model.compile(optimizer=SGD(lr=lr, momentum=0.9))
    model.train_on_batch(x, y, dropout=False)
    model.train_on_batch(x, y, dropout=False)
    e4 = model._active
    m4 = e4.adam_m.clone()
    assert float(m4.abs().max()) > 0
    model.train_on_batch(x[:2], y[:2], dropout=False)
    e2 = model._active
    assert e2 is not e4 and e2.iteration == 3 and e4.iteration == 2
    g = e2.grads[:e2.n_param]
    assert torch.allclose(e2.adam_m[:e2.n_param], 0.9 * m4[:e2.n_param] - lr * g, rtol=1e-4,
                          atol=1e-6 * lr * float(g.abs().max()))


def test_recompile_with_the_same_sgd_object_keeps_iterations_and_zeroes_the_slot():
    from dl3_amd.optimizers import SGD
    model = _build()
    x, y = _batch(2, 14)
    lr, decay = 0.01, 0.5
    opt = SGD(lr=lr, momentum=0.9, decay=decay)
    model.compile(optimizer=opt)
    for _ in range(3):
        model.train_on_batch(x, y, dropout=False)
    e1 = model._active
    assert e1.iteration == 3 and float(e1.adam_m.abs().max()) > 0
    model.compile(optimizer=opt)                      # same object: the clock goes on, the momentum starts over
    model.train_on_batch(x, y, dropout=False)
    e2 = model._active
    assert e2 is not e1 and e2.iteration == 4
    g = e2.grads[:e2.n_param]
    # step it = 3 from a zero buffer: v = -lr / (1 + 3 decay) g exactly (one rounding of lr_t, one of the product)
    assert torch.allclose(e2.adam_m[:e2.n_param], -(lr / (1 + 3 * decay)) * g, rtol=1e-6, atol=0)
    model.compile(optimizer=SGD(lr=lr, momentum=0.9, decay=decay))   # a NEW object starts at 0
    model.train_on_batch(x, y, dropout=False)
    e3 = model._active
    assert e3.iteration == 1
    assert torch.allclose(e3.adam_m[:e3.n_param], -lr * e3.grads[:e3.n_param], rtol=1e-6, atol=0)


# =================================================================================================== fit_generator
class _OneBatch:
    def __init__(self, seeds):
        self.batches = [_batch(2, s) + (np.ones((2, 64 * 64), np.float32),) for s in seeds]
        self.batch_size = 2

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.batches[i]


def test_fit_generator_follows_a_poly_learning_rate_schedule():
    """LearningRateScheduler(poly_decay) over three one-step epochs: History records the schedule, and the step uses it — with
    SGD momentum 0 the epoch's update is -lr_epoch * gradient"""
    from dl3_amd.callbacks import LambdaCallback, LearningRateScheduler, poly_decay
    from dl3_amd.optimizers import SGD
    model = _build()
    model.compile(optimizer=SGD(lr=123.0, momentum=0.0))   # the schedule replaces it before the first step
    sched = poly_decay(0.05, 3, power=0.9)
    eng = model._engine(2, True)
    n = eng.n_param
    snaps, ratios = {}, []

    def begin(epoch, logs):
        snaps["p"] = _np64(eng.params, n)

    def end(epoch, logs):
        assert model._active is eng
        upd, g = _np64(eng.params, n) - snaps["p"], _np64(eng.grads, n)
        lr = float(np.float32(sched(epoch)))
        assert np.all(np.abs(upd + lr * g) <= 4 * OO.U * (np.abs(snaps["p"]) + lr * np.abs(g)))
        ratios.append(float(-(upd * g).sum() / (g * g).sum()))   # the rate the step applied (least squares over the arena)
    hist = model.fit_generator(_OneBatch([60]), steps_per_epoch=1, epochs=3,
                               callbacks=[LearningRateScheduler(sched), LambdaCallback(on_epoch_begin=begin, on_epoch_end=end)])
    want = [0.05, 0.05 * (2.0 / 3) ** 0.9, 0.05 * (1.0 / 3) ** 0.9]
    assert hist.history["lr"] == pytest.approx(want, rel=1e-12) and len(hist.history["loss"]) == 3
    assert ratios == pytest.approx(want, rel=1e-5)         # the update size scales with the schedule
    assert eng.iteration == 3 and model._get_lr() == pytest.approx(want[-1], rel=1e-12)
