// tailmath.h — the per-pixel arithmetic the output head's consumers share (device helpers only): misc.hip (resize and the
// training loss tails), evaltail.hip (evaluation tail), crfunary.hip (CRF unary), mine.hip and jaccard.hip (the fronts of the
// mined and the soft-Jaccard loss) decode the same class scores.
#pragma once
#include "common.h"

// tf.image.resize_bilinear(align_corners=False) of TF 1.x: src = dst * (in/out), no half-pixel offset; lower =
// floor(src), upper = min(lower + 1, in - 1), lerp = src - lower.  Every floating-point step is pinned: no contraction is
// left to the compiler, which used to pick a different form of the weight from one kernel to the next.
//   f   the source coordinate, a ROUNDED product (it feeds floor)
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
  r.wl = __fsub_rn(f, (float)r.lo);
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

// end of a 256-thread workgroup of a loss kernel: the four waves' sums (wave_sum of the lanes' terms) in a fixed order
__device__ __forceinline__ void block_loss_partial(float wsum, float *loss_part) {
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
