"""numpy statement of the evaluation tail (include/dl3.h dl3_eval_tail_*): from the low-resolution logits and the labels
to per-image loss sums, count(w != 0), dl3_seg_counts' counts, the confusion matrix and the mask.  Built from the
oracle's own operators (resize_bilinear_tf1, phase_shift, softmax, seg_counts) and Keras' clip rule; `dtype` selects the
arithmetic — float64 is the reference, float32 the yardstick a float32 device evaluation is measured against."""
import numpy as np

from oracle import dl3_oracle as O


def full_logits(form, x, shape, dtype=np.float64):
    """form 'bilinear': x [N,Hi,Wi,C], shape (Ho, Wo); 'shuffle': x [N,H,W,C*r*r], shape r; 'plain': x [N,H,W,C]"""
    x = np.asarray(x, dtype)
    if form == "bilinear":
        return O.resize_bilinear_tf1(x, shape[0], shape[1])
    if form == "shuffle":
        return O.phase_shift(x, shape)
    if form == "plain":
        return x
    raise ValueError(form)


def pixel_loss(logits, labels, dtype=np.float64):
    """l[m] of dl3_softmax_xent: softmax, renormalise, clip to [1e-7, 1 - 1e-7], -log; void (label == C) -> 0"""
    logits = np.asarray(logits, dtype)
    C = logits.shape[-1]
    p = O.softmax(logits)
    p = p / p.sum(-1, keepdims=True)
    t = np.asarray(labels).astype(np.int64).reshape(p.shape[:-1])
    valid = (t >= 0) & (t < C)
    pt = np.take_along_axis(p, np.where(valid, t, 0)[..., None], -1)[..., 0]
    q = np.clip(pt, dtype(1e-7), dtype(1) - dtype(1e-7))
    return np.where(valid, -np.log(q), dtype(0)).astype(dtype)


def eval_tail(form, x, shape, labels, weights=None, dtype=np.float64):
    """-> dict(loss_sum [N], nnz [N], counts [N,3,C], confusion [C,C], mask [N,Ho,Wo], margin [N,Ho,Wo]);
    margin = top-two gap of the interpolated logits (what decides whether a mask pixel is well defined)"""
    z = full_logits(form, x, shape, dtype)
    N, Ho, Wo, C = z.shape
    t = np.asarray(labels).reshape(N, Ho, Wo)
    w = np.ones((N, Ho, Wo), dtype) if weights is None else np.asarray(weights, dtype).reshape(N, Ho, Wo)
    ell = pixel_loss(z, t, dtype)
    loss_sum = (ell * w).reshape(N, -1).sum(1, dtype=dtype)
    mask = z.argmax(-1).astype(np.int32)
    top2 = np.sort(z, -1)[..., -2:] if C > 1 else np.concatenate([z - 1, z], -1)
    return dict(loss_sum=loss_sum, nnz=(w != 0).reshape(N, -1).sum(1).astype(np.int32),
                counts=O.seg_counts(mask, t, C), confusion=confusion(mask, t, C), mask=mask,
                margin=top2[..., 1] - top2[..., 0], logits=z)


def confusion(mask, labels, C):
    """int64 [C,C]: row = label, column = prediction, void labels skipped"""
    t = np.asarray(labels).astype(np.int64).reshape(-1)
    p = np.asarray(mask).astype(np.int64).reshape(-1)
    ok = (t >= 0) & (t < C)
    return np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C).astype(np.int64)


def batch_metrics(loss_sum, nnz, counts):
    """Keras' per-batch numbers from the tail's outputs of ONE batch: loss = sum(l*w) / count(w != 0) (0 when no weight
    is non-zero: every term is zero), Jaccard / accuracy from the batch's per-image counts"""
    from dl3_amd import utils as U
    n = int(np.sum(nnz))
    loss = float(np.sum(np.asarray(loss_sum, np.float64)) / n) if n else 0.0
    return [loss, U.Jaccard_from_counts(counts), U.accuracy_from_counts(counts)]


def weighted_average(per_batch, sizes):
    """Keras 2.2.4 test_loop: the pass returns the average of the per-batch values weighted by batch size"""
    a = np.asarray(per_batch, np.float64)
    s = np.asarray(sizes, np.float64)
    return list((a * s[:, None]).sum(0) / s.sum())
