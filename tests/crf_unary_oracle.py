"""numpy restatement of the softmax-unary contract (include/dl3.h dl3_crf_unary_*): the three gathers that
turn what the head leaves behind into full-resolution logits, the softmax, and pydensecrf's unary_from_softmax
[pydensecrf-semantics].  No code shared with the package's crf.py; the mean-field part is tests/crf_oracle.py.

Every function takes a `dtype` and works in it throughout: float64 is the reference the device is compared with, the
SAME code in float32 is the yardstick for what float32 can resolve.

The bilinear gather is the legacy tf.image.resize_bilinear rule as oracle/dl3_oracle.py states it (align_corners=False,
no half-pixel centres): src = dst * (in / out), lower = floor(src), upper = min(lower + 1, in - 1), weight = src - lower.
TF evaluates the coordinates in float32, and so does the float32 run here (tests/test_crf_unary_host.py checks that its
coordinates ARE oracle/'s).  The float64 run evaluates the same rule in float64: it is the reference, and a reference
that carried float32's coordinate rounding would count that rounding as "truth" — the float32 run's distance from it
would then leave out the part of float32's error that comes from the coordinates, which both a float32 oracle and a
float32 device pay (each in its own way: TF rounds the product, dl3_resize_bilinear_fwd fuses it into the weight)."""
import numpy as np


def lerp_coords(out_size, in_size, dtype=np.float64):
    scale = dtype(in_size) / dtype(out_size)
    src = np.arange(out_size).astype(dtype) * scale
    lo = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    hi = np.minimum(lo + 1, in_size - 1)
    return lo, hi, (src - lo.astype(dtype)).astype(dtype)


def gather_bilinear(x, Ho, Wo, dtype=np.float64):
    """x [B,Hi,Wi,C] -> [B,Ho,Wo,C]: top / bottom rows interpolated along x, then along y"""
    x = np.asarray(x, dtype)
    B, Hi, Wi, C = x.shape
    ylo, yhi, wy = lerp_coords(Ho, Hi, dtype)
    xlo, xhi, wx = lerp_coords(Wo, Wi, dtype)
    out = np.empty((B, Ho, Wo, C), dtype)
    for oy in range(Ho):
        r0, r1 = x[:, ylo[oy]], x[:, yhi[oy]]                      # [B,Wi,C]
        top = r0[:, xlo] + (r0[:, xhi] - r0[:, xlo]) * wx[None, :, None]
        bot = r1[:, xlo] + (r1[:, xhi] - r1[:, xlo]) * wx[None, :, None]
        out[:, oy] = top + (bot - top) * wy[oy]
    return out


def gather_shuffle(u, r, dtype=np.float64):
    """Subpixel._phase_shift by its index formula, one element at a time over (q, p):
    out[n, ia*r + q, ib*r + p, ch] = u[n, ia, ib, ch*r*r + p*r + q]"""
    u = np.asarray(u, dtype)
    B, H, W, P = u.shape
    C = P // (r * r)
    assert C * r * r == P
    out = np.empty((B, H * r, W * r, C), dtype)
    ch = np.arange(C) * r * r
    for q in range(r):
        for p in range(r):
            out[:, q::r, p::r, :] = u[:, :, :, ch + p * r + q]
    return out


def gather_plain(x, dtype=np.float64):
    return np.asarray(x, dtype)


def softmax(z, dtype=np.float64):
    z = np.asarray(z, dtype)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)


def unary_from_softmax(sm, scale=None, clip=1e-5, dtype=np.float64):
    """sm [C, ...] probabilities -> [C, N] energies in `dtype`: mix with the uniform distribution (scale), clip to
    [clip, 1], -log.  An unclipped zero probability costs +inf."""
    sm = np.asarray(sm, dtype)
    C = sm.shape[0]
    if scale is not None:
        sm = dtype(scale) * sm + dtype((1.0 - scale) / C)
    if clip is not None:
        sm = np.minimum(np.maximum(sm, dtype(clip)), dtype(1))
    with np.errstate(divide="ignore"):
        return (-np.log(sm)).reshape(C, -1).astype(dtype)


def unary(form, x, shape, is_prob=False, scale=None, clip=1e-5, dtype=np.float64):
    """the whole of one dl3_crf_unary_* call: x as the form takes it (bilinear: shape (Ho, Wo); shuffle: shape r; plain:
    x [B,N,C], logits or with is_prob probabilities) -> U [B,C,N]"""
    if form == "bilinear":
        z = gather_bilinear(x, shape[0], shape[1], dtype)
    elif form == "shuffle":
        z = gather_shuffle(x, shape, dtype)
    elif form == "plain":
        z = gather_plain(x, dtype)
    else:
        raise ValueError(form)
    B, C = z.shape[0], z.shape[-1]
    p = z.reshape(B, -1, C) if is_prob else softmax(z.reshape(B, -1, C), dtype)
    return np.stack([unary_from_softmax(p[b].T, scale, clip, dtype) for b in range(B)])


# ------------------------------------------------------------------------------------------- end-to-end cases
def softmax_case(H, W, C, seed):
    """an image (smooth gradient + noise, as tests/test_gpu_crf.py's smooth features) and logits [H,W,C]: the blurred
    one-hot of a blocky label map, scaled, plus N(0,1)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    im = 128 + 90 * np.stack([np.sin(x / 80.0 * (3 + seed % 3)), np.cos(y / 80.0 * 2.5), np.sin((x + y) / 80.0 * 2)], -1)
    im = np.clip(np.rint(im + rng.integers(-2, 3, (H, W, 3))), 0, 255).astype(np.uint8)
    blocks = rng.integers(0, C, ((H + 7) // 8, (W + 7) // 8))
    lab = np.kron(blocks, np.ones((8, 8), np.int64))[:H, :W]
    onehot = np.eye(C)[lab]                                          # [H,W,C]
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    pad = np.pad(onehot, ((2, 2), (2, 2), (0, 0)), mode="edge")
    blur = sum(k[a] * pad[a:a + H] for a in range(5))
    blur = sum(k[a] * blur[:, a:a + W] for a in range(5))
    logits = (4.0 * blur + rng.standard_normal((H, W, C))).astype(np.float32)
    return im, logits


def excusable(Q64, Q32):
    """the pixels the oracle itself cannot resolve: float64 top-two gap of Q below tau = max(1e-5, 10 x the distance of
    the oracle's float32 Q from its float64 Q).  -> (mask [N], tau, distance)"""
    dist = float(np.abs(np.asarray(Q32, np.float64) - Q64).max())
    tau = max(1e-5, 10.0 * dist)
    srt = np.sort(Q64, 0)
    return (srt[-1] - srt[-2]) < tau, tau, dist
