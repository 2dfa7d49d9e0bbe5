"""numpy restatement of the trimap definitions, written to be obviously right rather than fast: seeds by
array shifts, rings by brute force over the list of seeds with an integer ceiling root, bands by searchsorted and bincount.
tests/test_trimap_host.py holds it against scipy's chessboard and Euclidean distance transforms and against maps worked
out by hand; the device tests hold the kernels against it."""
import numpy as np

CHEBYSHEV, EUCLIDEAN = "chebyshev", "euclidean"
SEED_VOID, SEED_EDGES = 1, 2


def canon(labels, C):
    """label values as the seed rule compares them: 0..C-1, everything else void = C"""
    lab = np.asarray(labels)
    t = np.trunc(np.nan_to_num(lab.astype(np.float64), nan=0.0)).astype(np.int64)
    return np.where((t >= 0) & (t < C), t, C)


def seeds_of(labels, C, seeds=SEED_VOID | SEED_EDGES):
    """bool [B,H,W]: void pixels (bit 1) and / or pixels with a 4-neighbour of another value inside the image (bit 2)"""
    v = canon(labels, C)
    out = np.zeros(v.shape, bool)
    if seeds & SEED_VOID:
        out |= v == C
    if seeds & SEED_EDGES:
        dy = v[:, 1:, :] != v[:, :-1, :]
        dx = v[:, :, 1:] != v[:, :, :-1]
        out[:, 1:, :] |= dy
        out[:, :-1, :] |= dy
        out[:, :, 1:] |= dx
        out[:, :, :-1] |= dx
    return out


def ceil_root(d2):
    """the smallest integer r >= 0 with r * r >= d2, in integers"""
    d2 = np.asarray(d2, np.int64)
    r = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > d2, r - 1, r)          # floor root, whatever the float root did
    r = np.where((r + 1) * (r + 1) <= d2, r + 1, r)
    return np.where(r * r < d2, r + 1, r)


def rings_from_seeds(seed, wmax, metric):
    """uint8 [B,H,W]: per image, the smallest integer w with a seed within distance w, clamped to wmax + 1"""
    seed = np.asarray(seed, bool)
    B, H, W = seed.shape
    out = np.full((B, H, W), wmax + 1, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        ys, xs = np.nonzero(seed[b])
        best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
        for i in range(0, len(ys), 256):          # the seed list in slabs, to bound the memory of the brute force
            dy = np.abs(yy[None] - ys[i:i + 256, None, None])
            dx = np.abs(xx[None] - xs[i:i + 256, None, None])
            d = np.maximum(dy, dx) if metric == CHEBYSHEV else dy * dy + dx * dx
            best = np.minimum(best, d.min(0))
        if len(ys):
            r = best if metric == CHEBYSHEV else ceil_root(best)
            out[b] = np.minimum(r, wmax + 1)
    return out.astype(np.uint8)


def rings(labels, C, wmax, metric=CHEBYSHEV, seeds=SEED_VOID | SEED_EDGES):
    return rings_from_seeds(seeds_of(labels, C, seeds), wmax, metric)


def bins_of(ring, widths):
    """the first k with ring <= widths[k], else K"""
    return np.searchsorted(np.asarray(widths, np.int64), np.asarray(ring, np.int64), side="left")


def band_confusion(pred, labels, ring, C, widths):
    """int64 [K+1,C,C], disjoint: pixels with a legal label t and a prediction p in 0..C-1 counted at [bin][t][p]"""
    K = len(widths)
    t = canon(labels, C).reshape(-1)
    p = np.asarray(pred, np.int64).reshape(-1)
    k = bins_of(ring, widths).reshape(-1)
    keep = (t < C) & (p >= 0) & (p < C)
    flat = (k[keep] * C + t[keep]) * C + p[keep]
    return np.bincount(flat, minlength=(K + 1) * C * C).reshape(K + 1, C, C).astype(np.int64)


def confusion(pred, labels, C):
    """the whole-image matrix: numpy's bincount over label * C + prediction"""
    t = canon(labels, C).reshape(-1)
    p = np.asarray(pred, np.int64).reshape(-1)
    keep = (t < C) & (p >= 0) & (p < C)
    return np.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C).astype(np.int64)


# --------------------------------------------------------------------------------------------------------- test inputs
def blobby(rng, B, H, W, C, void=0.01):
    """arg-max of box-smoothed noise, with a fraction of void pixels: float32 [B,H,W], void = C"""
    z = rng.standard_normal((B, H, W, C))
    for _ in range(3):
        p = np.pad(z, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
        z = sum(p[:, i:i + H, j:j + W] for i in range(3) for j in range(3))
    lab = z.argmax(-1).astype(np.float32)
    lab[rng.random((B, H, W)) < void] = C
    return lab


def corner(H, W):
    """background with a 3x3 block (clipped to the image) of class 1 in the top-left corner: the far corner sees every ring
    value the image has room for"""
    lab = np.zeros((H, W), np.float32)
    lab[:3, :3] = 1.0
    return lab
