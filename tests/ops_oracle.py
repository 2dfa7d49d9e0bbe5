"""float64 restatements of the element-wise, resize, gather and loss operators of include/dl3.h, the two derived
comparison bounds and the guard-band helper (numpy only; no device code).

Every oracle takes flat buffers with explicit leading dimensions and column offsets — the way the engine calls the
kernels (padded rows, column slices of wider buffers) — and returns (expected, magnitude).  `magnitude` is, per
element, the sum of the absolute values of the terms that make the element up: an fp32 evaluation with r roundings on
its longest path differs from the exact value by at most r * 2**-24 * magnitude (first order), whatever cancels.

`dt` (where a function has it) is the arithmetic type of the evaluation: float64 for the expected values, float32 for
a host emulation of the kernel that the bounds must ACCEPT (tests/test_ops_oracle_host.py).  Keyword `bug=` selects a
deliberately wrong variant that the bounds must REJECT (same file)."""
import numpy as np

from oracle import dl3_oracle as O

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
SENTINEL = np.float32(-1.2345679e30)
GUARD_TAIL = 67


# ------------------------------------------------------------------------------------------------ comparison helpers
def worst_ratio(err, bound):
    """largest error / bound over the elements (0/0 counts as 0: an exact element of zero magnitude)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


RATIOS = {}   # family -> worst error / bound seen (the GPU file prints it; shows the slack the derived bounds leave)


def _note(family, ratio):
    if family is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


def assert_elementwise(dev, ref64, mag, roundings, family=None):
    """every element: |dev - ref64| <= 2 * roundings * 2**-24 * mag (the 2: an FMA contraction either way)"""
    dev, ref64, mag = np.asarray(dev, np.float64), np.asarray(ref64, np.float64), np.asarray(mag, np.float64)
    assert dev.shape == ref64.shape == mag.shape, (dev.shape, ref64.shape, mag.shape)
    assert np.isfinite(dev).all(), "non-finite device output"
    err, bound = np.abs(dev - ref64), 2.0 * roundings * U * mag
    ratio = worst_ratio(err, bound)
    _note(family, ratio)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0))), err.shape)
        raise AssertionError("%d of %d elements outside the element-wise bound; worst at %s: dev %r ref %r err %.3e "
                             "bound %.3e (ratio %.2f)" % (bad.sum(), bad.size, i, dev[i], ref64[i], err[i], bound[i],
                                                          ratio))
    return ratio


def assert_reduction(dev, ref64, abs_sum, chain, family=None):
    """every output of a sum: |dev - ref64| <= chain * 2**-24 * abs_sum (chain: longest fp32 add chain incl. the
    roundings of one term and the partial fold; abs_sum: the sum of the absolute values of the terms)"""
    dev, ref64, abs_sum = np.asarray(dev, np.float64), np.asarray(ref64, np.float64), np.asarray(abs_sum, np.float64)
    assert dev.shape == ref64.shape == abs_sum.shape, (dev.shape, ref64.shape, abs_sum.shape)
    assert np.isfinite(dev).all(), "non-finite device output"
    err, bound = np.abs(dev - ref64), chain * U * abs_sum
    ratio = worst_ratio(err, bound)
    _note(family, ratio)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0))), err.shape)
        raise AssertionError("%d of %d sums outside the reduction bound; worst at %s: dev %r ref %r err %.3e bound "
                             "%.3e (ratio %.2f)" % (bad.sum(), bad.size, i, dev[i], ref64[i], err[i], bound[i], ratio))
    return ratio


# ------------------------------------------------------------------------------------------------------- guard band
def guard_buffer(rows, ld, lead=0, tail=GUARD_TAIL):
    """flat float32 buffer of lead + rows*ld + tail sentinels: the region [rows][ld] starts `lead` elements in"""
    return np.full(lead + rows * ld + tail, SENTINEL, np.float32)


def region_index(rows, ld, c0, C, lead=0):
    """flat indices [rows][C] of columns c0..c0+C-1 of a [rows][ld] region that starts `lead` elements in"""
    return lead + np.arange(rows, dtype=np.int64)[:, None] * ld + c0 + np.arange(C, dtype=np.int64)[None, :]


def view(buf, rows, ld, c0, C, lead=0):
    return np.asarray(buf).ravel()[region_index(rows, ld, c0, C, lead)]


def put(buf, vals, rows, ld, c0, C, lead=0):
    buf.ravel()[region_index(rows, ld, c0, C, lead)] = np.asarray(vals).reshape(rows, C)
    return buf


def assert_guard(buf, written_index):
    """every element outside `written_index` (flat indices the contract writes) still holds the sentinel, bit for bit"""
    flat = np.ascontiguousarray(np.asarray(buf, np.float32)).ravel()
    untouched = np.ones(flat.size, bool)
    untouched[np.asarray(written_index).ravel()] = False
    got = flat.view(np.uint32)[untouched]
    want = np.array([SENTINEL], np.float32).view(np.uint32)[0]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d elements outside the contract were written (first flat index %d)" % (
        bad.size, int(np.nonzero(untouched)[0][bad[0]]))


# ------------------------------------------------------------------------------------------------------- primitives
def act(x, a):
    if a == 1:
        return np.maximum(x, 0)
    if a == 2:
        return np.minimum(np.maximum(x, 0), 6)
    return x


def act_mask(z, a):
    if a == 1:
        return (z > 0).astype(z.dtype)
    if a == 2:
        return ((z > 0) & (z < 6)).astype(z.dtype)
    return np.ones_like(z)


def transform(x, scale, shift, a, dt=np.float64):
    """T(x) = act(scale*x + shift) per channel (last axis); returns (T(x), |scale*x| + |shift|)"""
    x = np.asarray(x, dt)
    if scale is None:
        return act(x, a), np.abs(x).astype(np.float64)
    s, t = np.asarray(scale, dt), np.asarray(shift, dt)
    return act(s * x + t, a), (np.abs(s * x) + np.abs(t)).astype(np.float64)


def unambiguous_mask_input(x, scale, shift, a, margin=1e-4):
    """nudge the elements of x whose pre-activation lies within `margin` of a kink of the activation's derivative
    (0, and 6 for relu6): there an fp32 kernel and a float64 oracle may legitimately pick different masks"""
    x = np.array(x, np.float32)
    for _ in range(8):
        z = np.asarray(scale, np.float64) * x + np.asarray(shift, np.float64)
        near = np.abs(z) < margin
        if a == 2:
            near |= np.abs(z - 6) < margin
        if not near.any():
            return x
        x[near] += np.float32(0.03125)
    raise AssertionError("could not move the pre-activations off the kinks")


def keep_mask(seed, n, rate, step=0):
    """dl3_uniform / dl3_step_seed (csrc/common.h): splitmix64 of (seed + step * odd constant, element index)"""
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        seed = np.uint64(seed) + np.uint64(step) * np.uint64(0xD1B54A32D192ED03)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(rate)


def _keep(seed, M, C, rate, step, ld=None):
    """keep set [M][C] of element index m*C + c (bug: ld given -> indexed with m*ld + c)"""
    if ld is None:
        return keep_mask(seed, M * C, rate, step).reshape(M, C)
    return keep_mask(seed, M * ld, rate, step).reshape(M, ld)[:, :C]


# ------------------------------------------------------------------------------------------- affine_add, grad_finish
def affine_add(a, lda, ca, sa, ta, act_a, b, ldb, cb, sb, tb, act_b, M, C, rate=0.0, seed=0, step=0, dt=np.float64,
               bug=None, ldo=None):
    """out[m][c] = act_a(sa*a+ta) + act_b(sb*b+tb), then Dropout: * keep(m*C + c) / (1 - rate)"""
    v, mag = transform(view(a, M, lda, ca, C), sa, ta, act_a, dt)
    if b is not None:
        u, mu = transform(view(b, M, ldb, cb, C), sb, tb, act_b, dt)
        v, mag = v + u, mag + mu
    if rate > 0:
        ks = dt(1) / (dt(1) - dt(rate))
        k = _keep(seed, M, C, rate, step, ldo if bug == "mask_ld" else None)
        v, mag = np.where(k, v * ks, dt(0)), np.where(k, mag * float(ks), 0.0)
    return v, mag


def grad_finish(gin, ldgin, cg, gin_div, gin_scale, add, ldadd, cad, x, ldx, cx, scale, shift, a, mean, invstd, M, C,
                rate=0.0, seed=0, step=0, dt=np.float64, bug=None):
    """gout = mask_act(scale*x+shift) * gin_scale * gin[m // gin_div] * keep/(1-rate) + add;
    sums (per channel, over the rows): s1 = sum gout, s2 = sum gout * (x - mean) * invstd.
    Returns gout, magnitude, and (s1, |s1| terms, s2, |s2| terms) when mean is given."""
    g = view(gin, (M - 1) // gin_div + 1, ldgin, cg, C).astype(dt)
    if gin_div > 1:
        g = np.repeat(g, gin_div, axis=0)[:M]
    v = dt(gin_scale) * g
    if rate > 0:
        v = np.where(_keep(seed, M, C, rate, step, ldgin if bug == "mask_ld" else None), v * (dt(1) / (dt(1) - dt(rate))),
                     dt(0))
    xv = None
    if x is not None:
        xv = view(x, M, ldx, cx, C).astype(dt)
        z = xv if scale is None else np.asarray(scale, dt) * xv + np.asarray(shift, dt)
        v = v * act_mask(z, a)
    mag = np.abs(v).astype(np.float64)
    if add is not None:
        ad = view(add, M, ldadd, cad, C).astype(dt)
        v, mag = v + ad, mag + np.abs(ad)
    if mean is None:
        return v, mag
    rows = slice(0, M - 1) if bug == "drop_last_row" else slice(0, M)
    v64, x64 = v.astype(np.float64), xv.astype(np.float64)
    mu, isd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    s1, a1 = v64[rows].sum(0), mag[rows].sum(0)
    s2 = (v64 * ((x64 - mu) * isd))[rows].sum(0)
    a2 = (mag * ((np.abs(x64) + np.abs(mu)) * np.abs(isd)))[rows].sum(0)
    return v, mag, (s1, a1, s2, a2)


# ------------------------------------------------------------------------------------------ pooling, subsample, taps
def gap(x, ldx, cx, scale, shift, a, N, HW, C, out_scale):
    """out[n][c] = out_scale * sum_hw T(x)[n, hw, c]; magnitude: out_scale * sum of the term magnitudes"""
    t, m = transform(view(x, N * HW, ldx, cx, C), scale, shift, a)
    return t.reshape(N, HW, C).sum(1) * float(np.float32(out_scale)), m.reshape(N, HW, C).sum(1) * abs(out_scale)


def subsample_fwd(x, ldx, cx, scale, shift, a, N, H, W, C, stride, Ho, Wo):
    t, m = transform(view(x, N * H * W, ldx, cx, C), scale, shift, a)
    sl = (slice(None), slice(0, (Ho - 1) * stride + 1, stride), slice(0, (Wo - 1) * stride + 1, stride))
    return t.reshape(N, H, W, C)[sl], m.reshape(N, H, W, C)[sl]


def subsample_bwd(g, N, H, W, C, stride, Ho, Wo):
    dx = np.zeros((N, H, W, C), np.float32)
    dx[:, 0:(Ho - 1) * stride + 1:stride, 0:(Wo - 1) * stride + 1:stride] = np.asarray(g, np.float32).reshape(N, Ho, Wo, C)
    return dx


def conv_taps_fwd(x, ldx, cx, scale, shift, a, N, H, W, C, k, pad_t, pad_l, Ho, Wo, bug=None):
    """cols[(n,oy,ox)][(i*k+j)*C + c] = T(x)[n, oy-pad_t+i, ox-pad_l+j, c], exactly 0 outside the image"""
    t, m = transform(view(x, N * H * W, ldx, cx, C), scale, shift, a)
    t, m = t.reshape(N, H, W, C), m.reshape(N, H, W, C)
    cols, mag = np.zeros((N, Ho, Wo, k * k, C)), np.zeros((N, Ho, Wo, k * k, C))
    if bug == "pad_transformed":   # the transform applied to the zero padding: act(shift) instead of 0
        cols[:] = transform(np.zeros(C), scale, shift, a)[0]
    for i in range(k):
        for j in range(k):
            for oy in range(Ho):
                iy = oy - pad_t + i
                if not 0 <= iy < H:
                    continue
                ox0, ox1 = max(0, pad_l - j), min(Wo, W + pad_l - j)
                if ox1 > ox0:
                    cols[:, oy, ox0:ox1, i * k + j] = t[:, iy, ox0 - pad_l + j:ox1 - pad_l + j]
                    mag[:, oy, ox0:ox1, i * k + j] = m[:, iy, ox0 - pad_l + j:ox1 - pad_l + j]
    return cols.reshape(N * Ho * Wo, k * k * C), mag.reshape(N * Ho * Wo, k * k * C)


def conv_taps_bwd(dcols, N, H, W, C, k, pad_t, pad_l, Ho, Wo):
    """the adjoint of the gather: dx[n,iy,ix,c] = sum over the taps that read (iy,ix) of dcols; (dx, sum of |terms|)"""
    d = np.asarray(dcols, np.float64).reshape(N, Ho, Wo, k * k, C)
    dx, ab = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for i in range(k):
        for j in range(k):
            for oy in range(Ho):
                iy = oy - pad_t + i
                if not 0 <= iy < H:
                    continue
                ox0, ox1 = max(0, pad_l - j), min(Wo, W + pad_l - j)
                if ox1 > ox0:
                    dx[:, iy, ox0 - pad_l + j:ox1 - pad_l + j] += d[:, oy, ox0:ox1, i * k + j]
                    ab[:, iy, ox0 - pad_l + j:ox1 - pad_l + j] += np.abs(d[:, oy, ox0:ox1, i * k + j])
    return dx, ab


# ------------------------------------------------------------------------------------------------- bilinear resize
def lerp_matrix(out_size, in_size, bug=None):
    """A [out][in] of the TF1 legacy bilinear resize along one axis, from oracle.dl3_oracle._tf1_lerp: the source
    coordinate and its floor are taken from the FP32 product fl(o * fl(in/out)) as TF and the kernels do; the entries
    (1 - w, w) are the exact float64 values of the fp32 weight w.  bug="hi_unclamped": upper = lower + 1 without the
    clamp to in-1 (the out-of-range neighbour reads as 0)."""
    lo, hi, w = O._tf1_lerp(out_size, in_size)
    A = np.zeros((out_size, in_size + 1))
    if bug == "hi_unclamped":
        hi = lo + 1
    o = np.arange(out_size)
    np.add.at(A, (o, lo), 1.0 - w.astype(np.float64))
    np.add.at(A, (o, hi), w.astype(np.float64))
    return A[:, :in_size]


def lerp_slack(out_size, in_size):
    """S [out][in]: the source coordinate f(o) = fl(o * fl(in/out)) at the (at most two) inputs output o reads.  The
    weight w = f - floor(f) is exact GIVEN f, but f is a rounded product of magnitude f: a kernel that contracts
    o*scale - floor into one FMA keeps the unrounded product and its weight differs by up to 2**-24 * f — an absolute
    error of the weight, far above 2**-24 * w for a long row.  It enters the magnitudes as f * (|lower| + |upper|)."""
    lo, hi, _ = O._tf1_lerp(out_size, in_size)
    f = (np.arange(out_size, dtype=np.float32) * (np.float32(in_size) / np.float32(out_size))).astype(np.float64)
    S = np.zeros((out_size, in_size))
    o = np.arange(out_size)
    S[o, lo] = f
    S[o, hi] = f
    return S


def fp32_index_differs(out_size, in_size):
    """output indices whose fp32 source coordinate floors to another integer than the exact rational o*in/out"""
    lo, _, _ = O._tf1_lerp(out_size, in_size)
    exact = np.minimum((np.arange(out_size, dtype=np.int64) * in_size) // out_size, in_size - 1)
    return np.nonzero(lo != exact)[0]


def resize_fwd(x, ldx, cx, scale, shift, a, N, Hi, Wi, Ho, Wo, C, dt=np.float64, bug=None):
    """y = resize_bilinear_tf1(T(x)); magnitude: the same interpolation of the term magnitudes"""
    t, m = transform(view(x, N * Hi * Wi, ldx, cx, C), scale, shift, a, dt)
    t, m = t.reshape(N, Hi, Wi, C), m.reshape(N, Hi, Wi, C)
    Ay, Ax = lerp_matrix(Ho, Hi), lerp_matrix(Wo, Wi)
    # |top| <= |tl| + (|tr| + |tl|) * w and the same again for the rows: at most 3x the plain interpolation of |T(x)|
    mag = 3.0 * np.einsum("oh,nhwc,pw->nopc", Ay, m, Ax)
    mag += np.einsum("oh,nhwc,pw->nopc", Ay, m, lerp_slack(Wo, Wi)) + np.einsum("oh,nhwc,pw->nopc", lerp_slack(Ho, Hi), m, Ax)
    if bug == "hi_unclamped":
        return np.einsum("oh,nhwc,pw->nopc", lerp_matrix(Ho, Hi, bug), t.astype(np.float64), lerp_matrix(Wo, Wi, bug)), mag
    return O.resize_bilinear_tf1(t, Ho, Wo), mag


def resize_bwd(dy, lddy, cy, N, Hi, Wi, Ho, Wo, C):
    """dx = resize^T(dy) [N,Hi,Wi,C]; (dx, sum of |terms|, each term with the slack of its two weights: lerp_slack)"""
    d = view(dy, N * Ho * Wo, lddy, cy, C).astype(np.float64).reshape(N, Ho, Wo, C)
    Ay, Ax = lerp_matrix(Ho, Hi), lerp_matrix(Wo, Wi)
    ab = np.einsum("oh,nopc,pw->nhwc", Ay, np.abs(d), Ax)
    ab += np.einsum("oh,nopc,pw->nhwc", Ay, np.abs(d), lerp_slack(Wo, Wi))
    ab += np.einsum("oh,nopc,pw->nhwc", lerp_slack(Ho, Hi), np.abs(d), Ax)
    return np.einsum("oh,nopc,pw->nhwc", Ay, d, Ax), ab


def resize_bwd_cols(d, Wi, Wo):
    """the x half: [N,Ho,Wo,C] -> [N,Ho,Wi,C]; (fold, sum of |terms|)"""
    Ax = lerp_matrix(Wo, Wi)
    d = np.asarray(d, np.float64)
    return np.einsum("nopc,pw->nowc", d, Ax), np.einsum("nopc,pw->nowc", np.abs(d), Ax + lerp_slack(Wo, Wi))


def resize_bwd_rows(xfold, Hi, Ho):
    """the y half: [N,Ho,Wi,C] -> [N,Hi,Wi,C]; (dx, sum of |terms|)"""
    Ay = lerp_matrix(Ho, Hi)
    d = np.asarray(xfold, np.float64)
    return np.einsum("oh,nowc->nhwc", Ay, d), np.einsum("oh,nowc->nhwc", Ay + lerp_slack(Ho, Hi), np.abs(d))


def taps_per_input(out_size, in_size):
    """the largest number of output indices that one input index collects from (length of the gather's add chain)"""
    return int((lerp_matrix(out_size, in_size) != 0).sum(0).max())


# ----------------------------------------------------------------------------------------------------- loss tail
CLIP_LO = float(np.float32(1e-7))                    # the kernels' fp32 constants 1e-7f and 1.f - 1e-7f
CLIP_HI = float(np.float32(1) - np.float32(1e-7))


def argmax_first(x, bug=None):
    x = np.asarray(x)
    if bug == "last_max":
        return x.shape[-1] - 1 - np.argmax(x[..., ::-1], axis=-1)
    return np.argmax(x, axis=-1)


def softmax_rows(x, zmag=None, dt=np.float64):
    """softmax over the last axis and its magnitude p * A.  The fp32 argument x - max carries an absolute error of
    2**-24 * (|x - max| + what the logits themselves carry: zmag, for interpolated logits), which the exponential turns
    into a RELATIVE error of the same size: A = 1 + max_c |x_c - max| (+ 2 * max_c zmag)."""
    x = np.asarray(x, dt)
    p = O.softmax(x)
    x64 = x.astype(np.float64)
    A = 1.0 + (x64.max(-1, keepdims=True) - x64.min(-1, keepdims=True))
    if zmag is not None:
        A = A + 2.0 * np.asarray(zmag, np.float64).max(-1, keepdims=True)
    return p, p.astype(np.float64) * A, A[..., 0]


def softmax_xent(x, labels, weights, nnz, zmag=None, dt=np.float64, bug=None):
    """sparse_crossentropy_ignoring_last_label with temporal sample weights on logits x [M][C] (include/dl3.h):
    row loss l = -log clip(q_t, 1e-7f, 1 - 1e-7f) * w / max(nnz, 1e-20), q = p / sum p;
    dlogits = (p - onehot) * w / nnz where q_t lies inside the clip interval, 0 outside; void rows (label outside
    0..C-1): no loss, no gradient whatever their weight.  Reuses oracle.dl3_oracle.softmax.
    Returns dict(p, pmag, dl, dlmag, l (row losses), lmag)."""
    x = np.asarray(x, dt)
    M, C = x.shape
    p, pmag, A = softmax_rows(x, zmag, dt)
    t = np.asarray(labels).astype(np.int64)
    valid = (t >= 0) & (t < C)
    w = np.ones(M, dt) if weights is None else np.asarray(weights, dt)
    if bug != "void_gradient":
        w = np.where(valid, w, dt(0))
    inv = dt(1) / np.maximum(dt(nnz), dt(1e-20))
    onehot = np.zeros((M, C), dt)
    onehot[np.nonzero(valid)[0], t[valid]] = 1
    q = (p * onehot).sum(-1) / p.sum(-1)
    inside = np.where(valid, (q >= dt(CLIP_LO)) & (q <= dt(CLIP_HI)), True)
    with np.errstate(divide="ignore"):
        lq = np.where(valid, -np.log(np.clip(q, dt(CLIP_LO), dt(CLIP_HI))), dt(0))
    wv = np.where(valid, w, dt(0))
    l = lq * wv * inv
    # log q: relative error of q (the probability's, twice: numerator and sum) taken absolutely, plus its own rounding
    lmag = (np.abs(lq).astype(np.float64) + A) * np.abs(wv).astype(np.float64) * float(inv)
    gs = w * inv * inside
    dl = (p - onehot) * gs[:, None]
    dlmag = (pmag + onehot.astype(np.float64)) * np.abs(gs).astype(np.float64)[:, None]
    return dict(p=p, pmag=pmag, dl=dl, dlmag=dlmag, l=l, lmag=lmag)


def clip_ambiguous_rows(x, labels):
    """rows whose true-class q lies so close to a clip bound that fp32 and float64 may decide `inside` differently"""
    x = np.asarray(x, np.float64)
    M, C = x.shape
    p = O.softmax(x)
    t = np.asarray(labels).astype(np.int64)
    valid = (t >= 0) & (t < C)
    q = np.where(valid, p[np.arange(M), np.clip(t, 0, C - 1)], 0.5)
    return valid & (((1 - q > 2e-8) & (1 - q < 5e-7)) | (np.abs(q - 1e-7) < 1e-9))


def xent_inputs(rng, M, C, void_w):
    """logits, labels (void == C), weights of a loss case: the clip-interval rows of tests/test_gpu_ops.py (true-class
    probability pushed outside [1e-7, 1 - 1e-7] on either side) in rows 0..19, and no row on the edge of the interval"""
    x = rng.normal(0, 3, (M, C)).astype(np.float32)
    labels = rng.integers(0, C + 1, M).astype(np.float32)
    for i in range(min(20, M)):
        labels[i] = i % C
        x[i, i % C] = x[i].max() + 40.0 if (i >= 10 or C == 1) else x[i].min() - 40.0
    amb = clip_ambiguous_rows(x, labels)
    x[amb] *= np.float32(0.5)
    assert not clip_ambiguous_rows(x, labels).any()
    w = rng.uniform(0.5, 2, M)
    w = (w if void_w else (labels < C) * w).astype(np.float32)
    return x, labels, w


# ------------------------------------------------------------------------------------------------------ optimizer
def adam(p, g, m, v, lr_t, b1, b2, eps, gs, denom=None, dt=np.float64):
    """Keras Adam (include/dl3.h): g' = g * scale, scale = gs (adam_step) or gs / max(denom, 1e-20) (adam_step_norm);
    m' = b1 m + (1-b1) g'; v' = b2 v + (1-b2) g'^2; p' = p - lr_t m' / (sqrt(v') + eps).
    Returns (p', m', v') and their magnitudes."""
    p, g, m, v = [np.asarray(a, dt) for a in (p, g, m, v)]
    b1, b2, lr_t, eps = dt(np.float32(b1)), dt(np.float32(b2)), dt(np.float32(lr_t)), dt(np.float32(eps))
    sc = dt(np.float32(gs)) if denom is None else dt(np.float32(gs)) / np.maximum(dt(np.float32(denom)), dt(1e-20))
    gi = g * sc
    m2 = b1 * m + (dt(1) - b1) * gi
    v2 = b2 * v + (dt(1) - b2) * gi * gi
    den = np.sqrt(v2) + eps
    p2 = p - lr_t * m2 / den
    mm = (np.abs(b1 * m) + np.abs((dt(1) - b1) * gi)).astype(np.float64)
    vm = np.abs(v2).astype(np.float64)
    pm = np.abs(p).astype(np.float64) + float(lr_t) * mm / den.astype(np.float64)
    return (p2, m2, v2), (pm, mm, vm)


# ------------------------------------------------------------------------------------------------------ BatchNorm
def bn_finalize(part, P, ldc, c0, C, count, gamma, beta, eps, momentum, unbias, mmean, mvar, bug=None):
    """fold partials [P][ldc][2] (channels c0..c0+C-1) into scale, shift, mean, invstd and the moving statistics;
    the biased variance is clamped at 0"""
    pt = np.asarray(part, np.float64).reshape(P, ldc, 2)[:, c0:c0 + C]
    s1, s2 = pt[:, :, 0].sum(0), pt[:, :, 1].sum(0)
    mean = s1 / count
    var = s2 / count - mean * mean
    if bug != "var_unclamped":
        var = np.maximum(var, 0)
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    with np.errstate(invalid="ignore"):
        invstd = 1 / np.sqrt(var + eps)
    scale = np.asarray(gamma, np.float64) * invstd
    out = dict(scale=scale, shift=np.asarray(beta, np.float64) - mean * scale, mean=mean, invstd=invstd)
    if mmean is not None:
        out["mmean"] = mom * np.asarray(mmean, np.float64) + (1 - mom) * mean
        out["mvar"] = mom * np.asarray(mvar, np.float64) + (1 - mom) * var * unbias
    return out


def bn_bwd_finalize(dpart, P, ldc, c0, C, count, gamma, mean, invstd, batch_mode):
    pt = np.asarray(dpart, np.float64).reshape(P, ldc, 2)[:, c0:c0 + C]
    s1, s2 = pt[:, :, 0].sum(0), pt[:, :, 1].sum(0)
    ga, mu, isd = [np.asarray(a, np.float64) for a in (gamma, mean, invstd)]
    a = ga * isd
    b = -a * isd * s2 / count if batch_mode else np.zeros(C)
    c = -a * s1 / count - b * mu if batch_mode else np.zeros(C)
    return dict(cA=a, cB=b, cC=c, dgamma=s2, dbeta=s1)


def negative_variance_sums(n=4096):
    """(s1, s2) fp32 sums of a constant tensor of n values whose float64 s2/n - (s1/n)^2 is NEGATIVE: the squares are
    rounded to fp32 before they are summed, and for some constants they round down"""
    for i in range(1, 200):
        c = np.float32(1.0 + i / 128.0 + 1.0 / 3.0)
        y = np.full(n, c, np.float32)
        s1, s2 = np.float32(y.sum(dtype=np.float32)), np.float32((y * y).sum(dtype=np.float32))
        if float(s2) / n - (float(s1) / n) ** 2 < 0:
            return float(s1), float(s2), n
    raise AssertionError("no constant with a negative fp32 variance found")
