// tailmath.h — the per-pixel arithmetic the output head's consumers share (device helpers only): misc.hip (resize),
// losstail.hip (the training loss tails, cross-entropy and focal), evaltail.hip (evaluation tail), crfunary.hip (CRF unary),
// mine.hip and jaccard.hip (the fronts of the mined and the soft-Jaccard loss) decode the same class scores.
#pragma once
#include "common.h"

// tf.image.resize_bilinear(align_corners=False) of TF 1.x: src = dst * (in/out), no half-pixel offset; lower =
// floor(src), upper = min(lower + 1, in - 1), lerp = src - lower.  Both weights are pinned.  HIP's __fmul_rn / __fsub_rn are
// plain operators, which the compiler may still contract: what pins w is the explicit __fmaf_rn, and what pins wl is the
// block with contraction off around its one subtraction (before, wl was merged with the product into w in one kernel and
// not in the next: the 16-byte variant of eval_bilinear_kernel did).
//   f   the source coordinate, a ROUNDED product (it feeds floor, and the subtraction of wl keeps it rounded)
//   w   ONE fused multiply-subtract scale * o - lo: the weight of dl3_resize_bilinear_fwd / _bwd / _bwd_rows and of
//       dl3_upsample_softmax_xent_fold (both variants: its gradient goes back through _bwd_rows).  Whatever has to
//       reproduce the resize kernel bit for bit takes it: the mask of dl3_eval_tail_bilinear, dl3_crf_unary_bilinear.
//   wl  f - lo with f rounded, the weight as TF 1.x (and the oracle) state it; it differs from w by up to an ulp of src
//       (2e-6 at 33 -> 513).  dl3_upsample_softmax_xent and the LOSS of dl3_eval_tail_bilinear take it (same source
//       pixels, same lerps).
// The multiplicand orders below are the ones the resize and loss kernels were compiled to: an IEEE product does not
// depend on them, the instruction schedule does.
struct Lerp {
  int lo, hi;
  float w, wl;
};
__device__ __forceinline__ Lerp tf1_lerp(int o, float scale, int in_size) {
  const float f = __fmul_rn((float)o, scale);
  Lerp r;
  r.lo = (int)floorf(f);
  if (r.lo > in_size - 1) r.lo = in_size - 1;
  r.hi = min(r.lo + 1, in_size - 1);
  r.w = __fmaf_rn(scale, (float)o, -(float)r.lo);
  {
#pragma clang fp contract(off)
    r.wl = f - (float)r.lo;
  }
  return r;
}
// a + (b - a) * w: the difference rounded, then ONE fused multiply-add
__device__ __forceinline__ float lerp1(float a, float b, float w) { return __fmaf_rn(w, __fsub_rn(b, a), a); }
__device__ __forceinline__ float bilerp(float tl, float tr, float bl, float br, float wx, float wy) {
  return lerp1(lerp1(tl, tr, wx), lerp1(bl, br, wx), wy);
}
// logit c of one output pixel from the rows of its four source pixels; classes past C - 1 repeat the last one, so that a
// loop unrolled to MAXC >= C needs no branch.  The loop stays with the caller (#pragma unroll) and the loads keep this
// order, top pair then bottom pair: the schedule of the loss kernels follows both.
__device__ __forceinline__ float bilerp_logit(const float *tl, const float *tr, const float *bl, const float *br, int c,
                                              int C, float wx, float wy) {
  const int cc = min(c, C - 1);
  const float top = lerp1(tl[cc], tr[cc], wx);
  const float bot = lerp1(bl[cc], br[cc], wx);
  return lerp1(top, bot, wy);
}
// The four source pixels of output pixel (oy, ox) and its two lerps.  The call site names the weights it takes:
// t.load<MAXC>(z, C, t.lx.w, t.ly.w) or (.., t.lx.wl, t.ly.wl).
struct BilinearTaps {
  const float *tl, *tr, *bl, *br;
  Lerp ly, lx;
  // from the image's low-resolution logits b [Hi][Wi][C]
  __device__ __forceinline__ BilinearTaps(const float *b, int oy, int ox, float sy, float sx, int Hi, int Wi, int C)
      : ly(tf1_lerp(oy, sy, Hi)), lx(tf1_lerp(ox, sx, Wi)) {
    tl = b + ((size_t)ly.lo * Wi + lx.lo) * C, tr = b + ((size_t)ly.lo * Wi + lx.hi) * C;
    bl = b + ((size_t)ly.hi * Wi + lx.lo) * C, br = b + ((size_t)ly.hi * Wi + lx.hi) * C;
  }
  // from the two source rows of an output row staged in LDS, src [2][Wi][C] (rows ly.lo, ly.hi)
  __device__ __forceinline__ BilinearTaps(const float *src, const Lerp &ly_, int ox, float sx, int Wi, int C)
      : ly(ly_), lx(tf1_lerp(ox, sx, Wi)) {
    tl = src + lx.lo * C, tr = src + lx.hi * C;
    bl = src + (Wi + lx.lo) * C, br = src + (Wi + lx.hi) * C;
  }
  template <int MAXC>
  __device__ __forceinline__ void load(float (&z)[MAXC], int C, float wx, float wy) const {
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = bilerp_logit(tl, tr, bl, br, c, C, wx, wy);
  }
};
// flat output pixel m of [N][Ho][Wo] -> (n, oy, ox)
struct PixelPos {
  int n, oy, ox;
};
__device__ __forceinline__ PixelPos split_pixel(long m, int Ho, int Wo) {
  PixelPos p;
  p.ox = (int)(m % Wo);
  const long q = m / Wo;
  p.oy = (int)(q % Ho), p.n = (int)(q / Ho);
  return p;
}

// The logits of a pixel live in registers, float z[MAXC] with MAXC in {8, 24, 32} >= C (DL3_DISPATCH_MAXC); classes past
// C - 1 repeat z[0] for the maximum and give 0 for the exponential, so that the unrolled loops need no branch.
constexpr int kHeadMaxC = 32;
// the maximum of the pixel's logits
template <int MAXC>
__device__ __forceinline__ float logit_max(const float (&z)[MAXC], int C) {
  const float z0 = z[0];
  float mx = z0;
#pragma unroll
  for (int c = 1; c < MAXC; c++) {
    const float zc = z[c];   // a value, not `(c < C) ? z[c] : z[0]`: that selects the ADDRESS, a dynamic index into z
    mx = fmaxf(mx, (c < C) ? zc : z0);
  }
  return mx;
}
// z[c] <- exp(z[c] - mx) in place (expf, or __expf where FAST); returns their sum, added in ascending class order in Sum
template <int MAXC, typename Sum, bool FAST = false>
__device__ __forceinline__ Sum exp_sum(float (&z)[MAXC], int C, float mx) {
  Sum ssum = 0;
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    const float e = (c < C) ? (FAST ? __expf(z[c] - mx) : expf(z[c] - mx)) : 0.f;
    z[c] = e;
    ssum += (Sum)e;
  }
  return ssum;
}
// the two together: the numerators of the softmax and their sum
template <int MAXC, typename Sum, bool FAST = false>
__device__ __forceinline__ Sum softmax_exp(float (&z)[MAXC], int C) {
  return exp_sum<MAXC, Sum, FAST>(z, C, logit_max<MAXC>(z, C));
}

// Subpixel tile in LDS: PB consecutive pixels of one row of the UNshuffled tensor u [N,H,W,C*r*r], element (pixel, ch,
// pq = p * r + q) at pixel * C * (r*r + 1) + ch * (r*r + 1) + pq, as in phase_shift_lds_kernel.  The channel stride is
// odd: lanes that walk along ch, or along pq, touch distinct banks.
// pixels per workgroup: as many as fit 48 KB of LDS (three workgroups per CU), at most cap, at most the row
inline int subpixel_tile_pixels(int W, int C, int r, int cap) {
  int pb = (int)((48u << 10) / ((size_t)C * (r * r + 1) * sizeof(float)));
  if (pb > cap) pb = cap;
  if (pb > W) pb = W;
  return pb;
}
// the evaluation tail's and the mining front's rule: no more than ~1024 shuffled pixels per workgroup, enough workgroups
// per image to fill the device
inline int shuffle_pb(int W, int C, int r) { return subpixel_tile_pixels(W, C, r, (1024 + r * r - 1) / (r * r)); }
struct SubpixelTile {
  int rr, P, LP;  // r*r; the floats of one pixel in u, and in the tile
  __device__ SubpixelTile(int C, int r) : rr(r * r), P(C * rr), LP(C * (rr + 1)) {}
  // logit 0 of output pixel pq of tile pixel px; logit c is c * (rr + 1) floats further
  __device__ int cell(int px, int pq) const { return px * LP + pq; }
  // the cell of float t of the tile's pb * P contiguous floats in u.  Staging: for (t = threadIdx.x; t < pb * P; t += 256)
  // { k = flat_cell(t); tile[k] = u[..]; } — the index BEFORE the load, as an assignment evaluates its right side first
  __device__ int flat_cell(int t) const {
    const int px = t / P, e = t % P;
    return px * LP + (e / rr) * (rr + 1) + e % rr;
  }
};

// Keras categorical_crossentropy clips the renormalised probability with tf.clip_by_value before the log
// (utils.py:130 -> keras/backend/tensorflow_backend.py), and the gradient of clip_by_value is ZERO where its input lies
// outside [1e-7, 1 - 1e-7]: a pixel whose true-class probability has left that interval has a constant loss and hands
// no gradient to any logit; inside it the gradient is (p - onehot).  1.f inside (bounds included, as TF), 0.f outside.
__device__ __forceinline__ float dl3_clip_pass(float q) { return (q >= 1e-7f && q <= 1.f - 1e-7f) ? 1.f : 0.f; }
// The loss normaliser count(w != 0): an integer count in a single process, count_all / world under data parallelism
// (fractional, below 1 when the global count is smaller than the world): only a zero count is replaced (no weight is
// non-zero -> every term is zero anyway)
#define DL3_NNZ_FLOOR 1e-20f

// exponentials -> probabilities in place (z *= 1 / ssum); psum their fp32 sum, pt the probability of label t (0: void)
struct ClassProbs {
  float psum, pt;
};
template <int MAXC>
__device__ __forceinline__ ClassProbs class_probs(float (&z)[MAXC], float ssum, int t) {
  const float inv = 1.f / ssum;
  float psum = 0.f, pt = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    const float p = z[c] * inv;
    z[c] = p;
    psum += p;
    pt = (c == t) ? p : pt;
  }
  return {psum, pt};
}
// The softmax cross-entropy of one pixel behind softmax_exp: z becomes the probabilities; a pixel that counts (the tail of
// a tile does not) with a legal label adds w * -log clip(pt / psum) / nnz to lsum — in ONE statement, as every loss kernel
// wrote it: how the compiler contracts it is part of their results; gs scales (p - onehot) to the gradient.  w is the
// sample weight, zero for a void label.  Returns gs.
template <int MAXC>
__device__ __forceinline__ float xent_pixel(float (&z)[MAXC], int C, float ssum, int t, float w, float inv_nnz, bool counts,
                                            float &lsum) {
  const ClassProbs p = class_probs<MAXC>(z, ssum, t);
  float inside = 1.f;
  if (counts && t >= 0 && t < C) {
    float q = p.pt / p.psum;
    inside = dl3_clip_pass(q);
    q = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
    lsum += -logf(q) * w * inv_nnz;
  }
  return w * inv_nnz * inside;
}

// The focal loss of one pixel, xent_pixel with two more factors: with q the clipped renormalised
// probability of the label and nl = -log q, the pixel adds w * at * (1 - q)^gamma * nl / nnz to lsum and scales (p - onehot)
// by w / nnz * inside * at * mu, mu = (1 - q)^gamma + gamma q (1 - q)^(gamma - 1) nl.  at is alpha at the label (1 where
// there is no alpha: the caller reads it, from LDS), gamma >= 0 is uniform over the launch.  With gamma = 0 and at = 1 both
// factors are exactly 1.f and the pixel is xent_pixel's, operation for operation.
//   1 - q   cancels where q -> 1: above one half it is the renormalised sum of the OTHER classes' probabilities (a sum of
//           positive terms, relative error of a few ulp), below it the subtraction (an absolute error of half an ulp of 1);
//           clipped to the complement of the interval q is clipped to, so (1 - q)^(gamma - 1) stays finite for gamma < 1
//   x^gamma multiplications for gamma in {0, 1, 2, 3, 4}, powf otherwise; x^(gamma - 1) beside it (a quotient for powf)
struct FocalPow {
  float pw, pw1;   // x^gamma, x^(gamma - 1)
};
__device__ __forceinline__ FocalPow focal_pow(float x, float gamma) {
  const int gi = (int)gamma;
  if ((float)gi == gamma && gi <= 4) {   // (uniform)
    float p1 = 1.f;
    for (int i = 1; i < gi; i++) p1 *= x;
    return {gi ? p1 * x : 1.f, p1};   // gamma = 0: mu's second term is 0 * p1
  }
  const float pw = powf(x, gamma);
  return {pw, pw / x};
}
template <int MAXC>
__device__ __forceinline__ float focal_pixel(float (&z)[MAXC], int C, float ssum, int t, float w, float inv_nnz, bool counts,
                                             float at, float gamma, float &lsum) {
  const ClassProbs p = class_probs<MAXC>(z, ssum, t);
  float inside = 1.f, mod = 1.f;
  if (counts && t >= 0 && t < C) {
    float po = 0.f;   // the other classes (z past C - 1 is zero)
#pragma unroll
    for (int c = 0; c < MAXC; c++) po += (c == t) ? 0.f : z[c];
    float q = p.pt / p.psum;
    inside = dl3_clip_pass(q);
    q = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
    // (the lower bound is 1 - the upper bound of q, 2^-23: where q is clipped to 1 - 1e-7f, 1 - q is what the formula says)
    const float omq = fminf(fmaxf(q > 0.5f ? po / p.psum : 1.f - q, 1.f - (1.f - 1e-7f)), 1.f - 1e-7f);
    const FocalPow f = focal_pow(omq, gamma);
    const float nl = -logf(q);
    lsum += nl * (at * f.pw) * w * inv_nnz;
    mod = at * (f.pw + gamma * (q * f.pw1 * nl));
  }
  return w * inv_nnz * inside * mod;
}

// end of a 256-thread workgroup of a loss kernel: the four waves' sums (wave_sum of the lanes' terms) in a fixed order
__device__ __forceinline__ void block_loss_partial(float wsum, float *loss_part) {
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
