"""numpy statement of the focal loss (include/dl3.h dl3_focal_xent and its three siblings): per pixel, with
p = softmax(z), q = clip(p_t / sum p, 1e-7f, 1 - 1e-7f) and inside = (the unclipped quotient lies in that interval),
  l = alpha[t] (1 - q)^gamma (-log q),  L = sum_m w l / count(w != 0),
  dL/dz[m,k] = (w / nnz) inside alpha[t] mu (p_k - [k = t]),  mu = (1 - q)^gamma + gamma q (1 - q)^(gamma - 1) (-log q)
for the plain, the bilinear and the shuffle form (eval_oracle.full_logits).  `dtype` selects the arithmetic: float64 is the
reference; float32 is the yardstick a float32 device evaluation is measured against — per-pixel arithmetic in float32,
1 - q the plain subtraction, the loss terms l * w / nnz added in float32 in index order."""
import numpy as np

from oracle import dl3_oracle as O
from tests import eval_oracle as E

CLIP_LO = np.float32(1e-7)                    # the contract's fp32 constants 1e-7f and 1.f - 1e-7f
CLIP_HI = np.float32(1) - np.float32(1e-7)


def class_weights(alpha, C, dtype=np.float64):
    """alpha [C] in dtype: None -> ones, a scalar (or one entry) broadcast"""
    if alpha is None:
        return np.ones(C, dtype)
    return np.broadcast_to(np.asarray(alpha, dtype).reshape(-1), (C,)).copy()


def pixel(z, t, gamma, alpha=None, dtype=np.float64):
    """logits z [..., C], labels t [...] -> dict(ell, mu, inside, p, valid, at): the per-pixel loss and gradient factors"""
    z = np.asarray(z, dtype)
    C = z.shape[-1]
    g, one = dtype(gamma), dtype(1)
    t = np.asarray(t).astype(np.int64).reshape(z.shape[:-1])
    valid = (t >= 0) & (t < C)
    tc = np.where(valid, t, 0)
    p = O.softmax(z)
    qt = np.take_along_axis(p / p.sum(-1, keepdims=True), tc[..., None], -1)[..., 0]
    lo, hi = dtype(CLIP_LO), dtype(CLIP_HI)
    inside = (qt >= lo) & (qt <= hi)
    q = np.clip(qt, lo, hi)
    omq = one - q
    nl = -np.log(q)
    pw = np.power(omq, g) if gamma else np.ones_like(q)
    mu = pw + g * q * np.power(omq, g - one) * nl if gamma else np.ones_like(q)
    at = class_weights(alpha, C, dtype)[tc]
    ell = np.where(valid, at * pw * nl, dtype(0)).astype(dtype)
    return dict(ell=ell, mu=mu.astype(dtype), inside=inside, p=p, valid=valid, at=at, t=tc)


def evaluate(form, x, shape, t, w=None, gamma=2.0, alpha=None, dtype=np.float64):
    """the step loss of one form ('plain' x [B,H,W,C]; 'bilinear' x [B,Hi,Wi,C], shape (Ho, Wo); 'shuffle' x
    [B,H,W,C*r*r], shape r) -> dict(ell [B,HW], loss, dlogits [B,HW,C] on the full-resolution logits, logits, nnz)"""
    z = E.full_logits(form, x, shape, dtype)
    B, C = z.shape[0], z.shape[-1]
    z = z.reshape(B, -1, C)
    t = np.asarray(t).reshape(B, -1)
    w = np.ones(t.shape, dtype) if w is None else np.asarray(w, dtype).reshape(t.shape)
    r = pixel(z, t, gamma, alpha, dtype)
    nnz = max(int((w != 0).sum()), 1)
    wv = np.where(r["valid"], w, dtype(0))
    if dtype == np.float64:
        loss = float((r["ell"] * wv).sum() / nnz)
        inv = 1.0 / nnz
    else:
        inv = dtype(1) / dtype(nnz)
        loss = float(np.cumsum((r["ell"] * wv * inv).reshape(-1), dtype=dtype)[-1])
    onehot = (r["t"][..., None] == np.arange(C)) & r["valid"][..., None]
    gs = (wv * inv * r["inside"] * r["at"] * r["mu"]).astype(dtype)
    dlogits = ((r["p"] - onehot.astype(dtype)) * gs[..., None]).astype(dtype)
    return dict(ell=r["ell"], loss=loss, dlogits=dlogits, logits=z, nnz=nnz)


def unshuffle(d, ushape, r):
    """a full-resolution tensor d [B,H*r,W*r,C] (or [B,HW,C]) in the layout of the unshuffled Subpixel output u
    [B,H,W,C*r*r], through the Subpixel index map (the oracle's phase_shift of u's own flat indices)"""
    idx = O.phase_shift(np.arange(int(np.prod(ushape)), dtype=np.int64).reshape(ushape), r)
    out = np.empty(int(np.prod(ushape)), np.asarray(d).dtype)
    out[idx.reshape(-1)] = np.asarray(d).reshape(-1)
    return out.reshape(ushape)
