"""numpy restatement of the dense-CRF contract [pydensecrf-semantics]: the exact mean-field inference of
the model the reference's do_crf configures (utils.py:74-91), by brute force — the N x N kernels are built explicitly in
row blocks, no separability trick, no code shared with the package's crf.py.  Every function takes a `dtype`: float64 is
the reference the device is compared with, the SAME code in float32 is the yardstick for what fp32 can resolve."""
import numpy as np

PARAMS = dict(gt_prob=0.7, gaussian_sxy=(3, 3), gaussian_compat=3, bilateral_sxy=80, bilateral_srgb=13,
              bilateral_compat=10, iterations=5)


def unary_from_labels(labels, L, gt_prob, zero_unsure, dtype=np.float64):
    labels = np.asarray(labels).reshape(-1)
    n_e = -np.log((1.0 - gt_prob) / (L - 1))
    p_e = -np.log(gt_prob)
    U = np.full((L, labels.size), n_e, dtype)
    for i, lab in enumerate(labels):
        U[(lab - 1) if zero_unsure else lab, i] = p_e  # Python's negative index: label 0 writes row L - 1
    if zero_unsure:
        U[:, labels == 0] = -np.log(1.0 / L)
    return U


def gauss_features(H, W, sxy, dtype=np.float64):
    y, x = np.mgrid[:H, :W]
    return np.stack([x.reshape(-1).astype(dtype) / dtype(sxy[0]), y.reshape(-1).astype(dtype) / dtype(sxy[1])], 1)


def bilateral_features(im, sxy, srgb, dtype=np.float64):
    H, W = im.shape[:2]
    y, x = np.mgrid[:H, :W]
    c = im.astype("uint8").reshape(H * W, 3).astype(dtype) / dtype(srgb)
    p = np.stack([x.reshape(-1).astype(dtype), y.reshape(-1).astype(dtype)], 1) / dtype(sxy)
    return np.concatenate([p, c], 1)


def kernel_rows(feat, rows, dtype=np.float64):
    """K[r, j] = exp(-|f_rows[r] - f_j|^2 / 2) for all j, the j = i term included"""
    f = np.asarray(feat, dtype)
    s = np.zeros((len(rows), f.shape[0]), dtype)
    for d in range(f.shape[1]):
        diff = f[rows, d][:, None] - f[None, :, d]
        s += diff * diff
    return np.exp(dtype(-0.5) * s)


def message_rows(feat, Q, rows, dtype=np.float64, block=64):
    """out[r] = sum_j K[rows[r], j] Q[j] for Q [N, L]"""
    Q = np.asarray(Q, dtype)
    rows = np.asarray(rows)
    out = np.empty((len(rows), Q.shape[1]), dtype)
    for i0 in range(0, len(rows), block):
        out[i0:i0 + block] = kernel_rows(feat, rows[i0:i0 + block], dtype) @ Q
    return out


def message(feat, Q, dtype=np.float64, block=64):
    return message_rows(feat, Q, np.arange(np.asarray(feat).shape[0]), dtype, block)


def full_kernel(feat, dtype=np.float64, block=256):
    N = feat.shape[0]
    K = np.empty((N, N), dtype)
    for i0 in range(0, N, block):
        K[i0:i0 + block] = kernel_rows(feat, np.arange(i0, min(i0 + block, N)), dtype)
    return K


def normalised(K, dtype=np.float64):
    """pydensecrf's default NORMALIZE_SYMMETRIC: n_i K_ij n_j with n = 1 / sqrt(row sum + 1e-20)"""
    n = dtype(1) / np.sqrt(K.sum(1, dtype=dtype) + dtype(1e-20))
    return n[:, None] * K * n[None, :]


def softmax0(E):
    E = E - E.max(0, keepdims=True)
    P = np.exp(E)
    return P / P.sum(0, keepdims=True)


def inference(im, U, params=PARAMS, dtype=np.float64, iters=None):
    """(Q [L,N], energy [L,N] of the last update, MAP [N]) for image im [H,W,3] and unary U [L,N]"""
    H, W = im.shape[:2]
    U = np.asarray(U, dtype)
    Kg = normalised(full_kernel(gauss_features(H, W, params["gaussian_sxy"], dtype), dtype), dtype)
    Kb = normalised(full_kernel(bilateral_features(im, params["bilateral_sxy"], params["bilateral_srgb"], dtype), dtype),
                    dtype)
    wg, wb = dtype(params["gaussian_compat"]), dtype(params["bilateral_compat"])
    E = -U
    Q = softmax0(E)
    for _ in range(params["iterations"] if iters is None else iters):
        E = -U + wg * (Q @ Kg.T) + wb * (Q @ Kb.T)
        Q = softmax0(E)
    return Q, E, np.argmax(Q, 0)


def restore(MAP, colors):
    """utils.py:86-89, the in-place loop with its quirk"""
    MAP = MAP.copy()
    for u in np.unique(MAP):
        np.putmask(MAP, MAP == u, colors[u])
    return MAP


def do_crf(im, mask, zero_unsure=True, dtype=np.float64, params=PARAMS):
    """the whole of the reference's do_crf; returns (restored mask [H,W], Q, energy, MAP, colors)"""
    colors, labels = np.unique(mask, return_inverse=True)
    labels = labels.reshape(-1)
    L = len(colors)
    if L == 1:
        return np.asarray(mask), None, None, None, colors
    U = unary_from_labels(labels, L, params["gt_prob"], zero_unsure, dtype)
    Q, E, MAP = inference(im, U, params, dtype)
    return restore(MAP.reshape(mask.shape[:2]), colors), Q, E, MAP, colors


def structured_case(H, W, L, seed, noise=0.25):
    """an image of L flat-coloured regions (vertical / horizontal bands crossed by a diagonal) with mild pixel noise, and
    its region map with `noise` of the pixels relabelled at random: the appearance kernel has something to find"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    region = ((x * L) // W + ((y * 2) // H) * ((L + 1) // 2) + (x + y > (H + W) // 2)) % L
    palette = rng.permutation(np.linspace(20, 235, L * 3).astype(np.int64)).reshape(L, 3)
    im = palette[region] + rng.integers(-6, 7, (H, W, 3))
    im = np.clip(im, 0, 255).astype(np.uint8)
    mask = region.copy()
    flip = rng.random((H, W)) < noise
    mask[flip] = rng.integers(0, L, int(flip.sum()))
    return im, mask.astype(np.int32), region.astype(np.int32)
