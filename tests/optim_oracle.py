"""float64 restatement of the optimizer step of include/dl3.h (dl3_grad_sumsq, dl3_opt_step) and of the host half in
engine.Engine.opt_step — numpy only, written from the formulas, no device code and nothing of the package.

[TF-semantics: Keras 2.2.4 keras/optimizers.py — Optimizer.get_gradients, SGD / RMSprop / Adam.get_updates — restated
from memory; the package is not installed.]

The kernel-level functions follow tests/ops_oracle.py: they take the launch's own arguments (lr_t already scheduled)
and return (expected, magnitude), magnitude being per element the sum of the absolute values of the terms that make the
element up.  `dt` is the arithmetic type (float64: the expected values)."""
import numpy as np


def effective_gradient(g, gs=1.0, denom=None, clipnorm=0.0, clipvalue=0.0, dt=np.float64):
    """Optimizer.get_gradients on the scaled gradient: sc = gs, or gs / max(denom, 1e-20) (the data-parallel form);
    clipnorm > 0: the GLOBAL norm sc * sqrt(sum g^2) — g' = g * sc * (clipnorm / norm) when norm >= clipnorm;
    clipvalue > 0: clamp to [-clipvalue, clipvalue] afterwards."""
    g = np.asarray(g, dt)
    sc = dt(np.float32(gs)) if denom is None else dt(np.float32(gs)) / np.maximum(dt(np.float32(denom)), dt(1e-20))
    ge = g * sc
    if clipnorm and clipnorm > 0:
        c = dt(np.float32(clipnorm))
        norm = sc * np.sqrt((g.astype(np.float64) ** 2).sum()).astype(dt)
        if norm >= c:
            ge = ge * (c / norm)
    if clipvalue and clipvalue > 0:
        cv = dt(np.float32(clipvalue))
        ge = np.clip(ge, -cv, cv)
    return ge


def sgd(p, ge, m, lr_t, momentum, nesterov=False, dt=np.float64):
    """v = momentum*m - lr_t*g'; m <- v; p += v, or with nesterov p += momentum*v - lr_t*g'.  -> (p', m'), magnitudes"""
    p, ge, m = [np.asarray(a, dt) for a in (p, ge, m)]
    lr_t, mom = dt(np.float32(lr_t)), dt(np.float32(momentum))
    v = mom * m - lr_t * ge
    vm = np.abs(mom * m) + np.abs(lr_t * ge)
    if nesterov:
        p2 = p + mom * v - lr_t * ge
        pm = np.abs(p) + mom * vm + np.abs(lr_t * ge)
    else:
        p2 = p + v
        pm = np.abs(p) + vm
    return (p2, v), (pm.astype(np.float64), vm.astype(np.float64))


def rmsprop(p, ge, a, lr_t, rho, eps, dt=np.float64):
    """a <- rho*a + (1-rho)*g'^2; p -= lr_t*g' / (sqrt(a) + eps).  -> (p', a'), magnitudes"""
    p, ge, a = [np.asarray(x, dt) for x in (p, ge, a)]
    lr_t, rho, eps = dt(np.float32(lr_t)), dt(np.float32(rho)), dt(np.float32(eps))
    a2 = rho * a + (dt(1) - rho) * (ge * ge)
    den = np.sqrt(a2) + eps
    p2 = p - lr_t * ge / den
    pm = np.abs(p) + np.abs(lr_t * ge / den)
    return (p2, a2), (pm.astype(np.float64), np.abs(a2).astype(np.float64))


def adam(p, ge, m, v, lr_t, b1, b2, eps, dt=np.float64):
    """m <- b1 m + (1-b1) g'; v <- b2 v + (1-b2) g'^2; p -= lr_t m / (sqrt(v) + eps) (the bias correction is in lr_t).
    -> (p', m', v'), magnitudes"""
    p, ge, m, v = [np.asarray(x, dt) for x in (p, ge, m, v)]
    lr_t, b1, b2, eps = dt(np.float32(lr_t)), dt(np.float32(b1)), dt(np.float32(b2)), dt(np.float32(eps))
    m2 = b1 * m + (dt(1) - b1) * ge
    v2 = b2 * v + (dt(1) - b2) * ge * ge
    den = np.sqrt(v2) + eps
    p2 = p - lr_t * m2 / den
    mm = np.abs(b1 * m) + np.abs((dt(1) - b1) * ge)
    pm = np.abs(p) + lr_t * mm / den
    return (p2, m2, v2), (pm.astype(np.float64), mm.astype(np.float64), np.abs(v2).astype(np.float64))


# ------------------------------------------------------------------------------------------- one whole Keras step
DEFAULTS = {
    "sgd": dict(lr=0.01, momentum=0.0, decay=0.0, nesterov=False),
    "rmsprop": dict(lr=0.001, rho=0.9, epsilon=1e-7, decay=0.0),
    "adam": dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0),
}


def keras_step(rule, p, g, s0, s1, it, clipnorm=0.0, clipvalue=0.0, gs=1.0, denom=None, **hyper):
    """get_updates of `rule` at iteration count `it` (the count BEFORE the increment: lr = lr / (1 + decay * it); Adam:
    t = it + 1 in the bias correction), float64 throughout and WITHOUT the fp32 rounding of the hyper-parameters.
    -> (p', s0', s1'); s1 passes through untouched for the one-slot rules"""
    o = dict(DEFAULTS[rule])
    o.update(hyper)
    p, g, s0 = np.asarray(p, np.float64), np.asarray(g, np.float64), np.asarray(s0, np.float64)
    sc = float(gs) if denom is None else float(gs) / max(float(denom), 1e-20)
    ge = g * sc
    if clipnorm and clipnorm > 0:
        norm = sc * np.sqrt((g ** 2).sum())
        if norm >= clipnorm:
            ge = ge * (clipnorm / norm)
    if clipvalue and clipvalue > 0:
        ge = np.clip(ge, -clipvalue, clipvalue)
    lr = o["lr"] / (1.0 + o["decay"] * it)
    if rule == "sgd":
        v = o["momentum"] * s0 - lr * ge
        p2 = p + o["momentum"] * v - lr * ge if o["nesterov"] else p + v
        return p2, v, s1
    if rule == "rmsprop":
        a = o["rho"] * s0 + (1.0 - o["rho"]) * ge * ge
        return p - lr * ge / (np.sqrt(a) + o["epsilon"]), a, s1
    t = it + 1
    lr_t = lr * np.sqrt(1.0 - o["beta_2"] ** t) / (1.0 - o["beta_1"] ** t)
    m = o["beta_1"] * s0 + (1.0 - o["beta_1"]) * ge
    v = o["beta_2"] * np.asarray(s1, np.float64) + (1.0 - o["beta_2"]) * ge * ge
    return p - lr_t * m / (np.sqrt(v) + o["epsilon"]), m, v
