"""numpy statement of hard-example mining (include/dl3.h dl3_pixel_xent_* / dl3_topk_threshold / dl3_mine_weights,
DESIGN.md §15): the per-pixel losses v of the three training forms (float64 is the reference, float32 the yardstick a
float32 device evaluation is measured against), the schedule in float32 — every operation one rounded float32 operation,
so k is the device's bit for bit — and tau, the mask and n' by np.partition."""
import numpy as np

from tests import eval_oracle as E

f32 = np.float32


def pixel_v(form, x, shape, labels, weights=None, dtype=np.float64):
    """v [N*Ho*Wo] = w * -log clip(p_label, 1e-7, 1 - 1e-7), 0 for a void label.  form / x / shape as
    eval_oracle.full_logits: 'plain' x [N,H,W,C]; 'bilinear' x [N,Hi,Wi,C], shape (Ho, Wo); 'shuffle' x [N,H,W,C*r*r],
    shape r.  The product w * l is formed in float32 from the rounded l, as the contract states (fp32 v)."""
    z = E.full_logits(form, x, shape, dtype)
    ell = E.pixel_loss(z, np.asarray(labels).reshape(z.shape[:-1]), dtype).reshape(-1)
    w = np.ones(ell.shape, dtype) if weights is None else np.asarray(weights, dtype).reshape(-1)
    v = ell * w
    return np.where(v > 0, v, dtype(0)).astype(dtype)


def schedule_pct(p, S, s):
    """pct in float32: p if S == 0 else fl(fl(ratio * p) + fl(1 - ratio)), ratio = min(1, fl32(s) / fl32(S))"""
    p = f32(p)
    if int(S) == 0:
        return p
    ratio = min(f32(1), f32(f32(int(s)) / f32(int(S))))
    return f32(f32(ratio * p) + f32(f32(1) - ratio))


def schedule_k(p, S, s, N):
    """k = min(N, trunc(fl(pct * fl32(N))))"""
    x = f32(schedule_pct(p, S, s) * f32(int(N)))
    return min(int(N), int(np.trunc(np.float64(x))))


def select(v, k):
    """-> (tau, mask, n'): tau the k-th largest of v (+inf for k == 0), mask = (v >= tau) & (v > 0) with every tie at
    tau kept, n' = count(mask)"""
    v = np.asarray(v, f32).reshape(-1)
    N = v.size
    k = int(k)
    assert 0 <= k <= N
    if k == 0:
        return f32(np.inf), np.zeros(N, bool), 0
    tau = np.partition(v, N - k)[N - k]
    m = (v >= tau) & (v > 0)
    return f32(tau), m, int(m.sum())


def mine(v, w, p, S, s):
    """the three outputs the loss kernel sees, from v: (k, tau, w', n')"""
    v = np.asarray(v, f32).reshape(-1)
    k = schedule_k(p, S, s, v.size)
    tau, m, n = select(v, k)
    w = np.ones(v.size, f32) if w is None else np.asarray(w, f32).reshape(-1)
    return k, tau, np.where(m, w, f32(0)).astype(f32), n
