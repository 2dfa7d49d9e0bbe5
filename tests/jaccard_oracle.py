"""numpy statement of the soft-Jaccard loss (include/dl3.h dl3_jaccard_* / dl3_*softmax_xent_jaccard):
per-image sums, the coefficient table, L_J and the gradient on the logits, for the plain and the bilinear form.  `dtype`
selects the arithmetic: float64 is the reference; float32 is the yardstick a float32 device evaluation is measured
against, and follows the contract — per-pixel arithmetic in float32, the three sums accumulated in float64, the
coefficients evaluated in float64 and rounded to float32 once.  (Summing in float32 would loosen the yardstick enough to
hide a wrong kernel.)"""
import numpy as np

from oracle import dl3_oracle as O
from tests import eval_oracle as E


def mask(labels, weights, C):
    """u [B,HW]: the sample weight is non-zero (None: w = 1) and the label is below C"""
    t = np.asarray(labels).astype(np.int64)
    t = t.reshape(t.shape[0], -1)
    u = (t >= 0) & (t < C)
    if weights is not None:
        u = u & (np.asarray(weights).reshape(t.shape) != 0)
    return u, t


def sums(z, labels, weights=None, dtype=np.float64):
    """logits z [B,HW,C] -> (sums [B,C,3] float64 = (I, S, Y), p [B,HW,C] in dtype, u, t)"""
    z = np.asarray(z, dtype)
    C = z.shape[-1]
    z = z.reshape(z.shape[0], -1, C)
    u, t = mask(labels, weights, C)
    p = O.softmax(z)
    y = (t[..., None] == np.arange(C)) & u[..., None]
    pu = p.astype(np.float64) * u[..., None]
    return np.stack([(pu * y).sum(1), pu.sum(1), y.sum(1).astype(np.float64)], -1), p, u, t


def coefficients(s, dtype=np.float64):
    """sums [B,C,3] -> (coef [B,C,2] = (A, Bc) in dtype, L_J, n_c [C], n_legal); float64 throughout, one rounding"""
    s = np.asarray(s, np.float64)
    I, S, Y = s[..., 0], s[..., 1], s[..., 2]
    present = Y > 0
    n_c = present.sum(0)
    n_legal = int((n_c > 0).sum())
    coef = np.zeros(s.shape[:2] + (2,), np.float64)
    if n_legal == 0:
        return coef.astype(dtype), 0.0, n_c, 0
    U = np.where(present, S + Y - I, 1.0)
    kappa = present / (np.maximum(n_c, 1)[None, :] * float(n_legal))
    coef[..., 0] = -kappa / U
    coef[..., 1] = kappa * I / (U * U)
    J = np.where(present, I / U, 0.0)
    legal = n_c > 0
    lj = 1.0 - float((J.sum(0)[legal] / n_c[legal]).sum() / n_legal)
    return coef.astype(dtype), lj, n_c, n_legal


def gradient(p, u, t, coef, dtype=np.float64):
    """dL_J/dz [B,HW,C] = u p_k (G_k - sum_c p_c G_c), G_c = A[b,c] where c is the pixel's label, else Bc[b,c]"""
    p = np.asarray(p, dtype)
    coef = np.asarray(coef, dtype)
    C = p.shape[-1]
    onehot = t[..., None] == np.arange(C)
    G = np.where(onehot, coef[:, None, :, 0], coef[:, None, :, 1]).astype(dtype)
    dot = (p * G).sum(-1, keepdims=True, dtype=dtype)
    return (u[..., None].astype(dtype) * (p * (G - dot))).astype(dtype)


def evaluate(form, x, shape, labels, weights=None, lam=1.0, dtype=np.float64):
    """the whole step loss of one form (eval_oracle.full_logits: 'plain' x [B,H,W,C]; 'bilinear' x [B,Hi,Wi,C], shape
    (Ho, Wo)) -> dict(sums, coef, lj, ce, loss, dlogits [B,HW,C], dce, dj): CE and its gradient by the oracle's
    loss_sparse_xent_ignoring_last_label (Keras' renormalise and clip, count(w != 0)), the Jaccard half on top"""
    z = E.full_logits(form, x, shape, dtype)
    B, C = z.shape[0], z.shape[-1]
    z = z.reshape(B, -1, C)
    t = np.asarray(labels).reshape(B, -1)
    w = np.ones(t.shape, dtype) if weights is None else np.asarray(weights, dtype).reshape(t.shape)
    ce, dce, _ = O.loss_sparse_xent_ignoring_last_label(z, t, w)
    s, p, u, ti = sums(z, t, weights, dtype)
    coef, lj, _, _ = coefficients(s, dtype)
    dj = gradient(p, u, ti, coef, dtype)
    return dict(sums=s, coef=coef, lj=lj, ce=ce, loss=ce + float(lam) * lj, dce=dce, dj=dj,
                dlogits=(dce + dtype(lam) * dj).astype(dtype), logits=z)
