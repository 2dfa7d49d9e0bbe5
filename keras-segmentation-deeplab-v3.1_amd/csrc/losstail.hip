// losstail.hip — the training loss tail: sparse_crossentropy_ignoring_last_label with temporal sample weights
// (utils.py:127-130) and the focal loss in the four forms of the tail, one pass over HBM each:
//   plain logits               dl3_softmax_xent                 dl3_focal_xent                 row_kernel<Term, false>
//   the final resize fused in  dl3_upsample_softmax_xent        dl3_upsample_focal_xent        row_kernel<Term, true>
//   ... with the x fold        dl3_upsample_softmax_xent_fold   dl3_upsample_focal_xent_fold   fold_kernel<Term, MAXC, PREF>
//   the unshuffled Subpixel    dl3_shuffle_softmax_xent         dl3_shuffle_focal_xent         shuffle_kernel<Term, MAXC>
// A form has ONE kernel body; the loss is its pixel term (XentTerm, FocalTerm below).  Both losses are pixel-wise with the
// normaliser count(w != 0), so the grid, the staging, the partial sums and the stores of a form do not depend on the term.
// The focal loss per pixel, with q the clipped renormalised probability of the label:
//   l = alpha[t] (1 - q)^gamma (-log q),  L = sum_m w l / nnz,
//   dL/dz[m,k] = (w / nnz) inside alpha[t] mu(q) (p_k - [k = t]),  mu = (1 - q)^gamma + gamma q (1 - q)^(gamma - 1) (-log q)
// With gamma = 0 and alpha null its gradient is the cross-entropy's bit for bit (tests/test_gpu_focal.py pins it).
// No atomics: two runs are bit-identical.  Ordinary vector stores only.  gamma is a launch argument, alpha a device pointer.
#include "tailmath.h"

namespace {

// ---------------------------------------------------------------------------------------------------- the pixel terms
// A term is built from its launch arguments (the kernels take them as a parameter pack between nnz and the gradient, empty
// where the term has none: its absence moves no other argument) and evaluates one pixel behind softmax_exp: z becomes the
// probabilities, the pixel's loss is added to lsum, the scale of (p - onehot) comes back.
//   kProbs   a probs output exists beside the gradient and either may be null (the row kernel; a term without one requires
//            the gradient and carries neither branch)
//   kLds     bytes of static LDS the term adds to a kernel
//   stage()  the barrier behind what the constructor wrote to LDS, for a kernel that has none of its own in front of the
//            first pixel
struct XentTerm {
  static constexpr bool kProbs = true;
  static constexpr size_t kLds = 0;
  float *probs;
  __device__ __forceinline__ XentTerm(int) : probs(nullptr) {}
  __device__ __forceinline__ XentTerm(float *probs_, int) : probs(probs_) {}   // the row kernel
  __device__ __forceinline__ void stage() const {}
  template <int MAXC>
  __device__ __forceinline__ float pixel(float (&z)[MAXC], int C, float ssum, int t, float w, float inv_nnz, bool counts,
                                         float &lsum) const {
    return xent_pixel<MAXC>(z, C, ssum, t, w, inv_nnz, counts, lsum);
  }
};

// alpha staged once per workgroup in LDS (a lane reads it at its own label), 1.f past C - 1 and where there is no alpha
struct FocalTerm {
  static constexpr bool kProbs = false;
  static constexpr size_t kLds = kHeadMaxC * sizeof(float);
  const float *sa;
  float gamma;
  __device__ __forceinline__ FocalTerm(const float *__restrict__ alpha, float gamma_, int C) : gamma(gamma_) {
    __shared__ float table[kHeadMaxC];
    if (threadIdx.x < kHeadMaxC) table[threadIdx.x] = (alpha && (int)threadIdx.x < C) ? alpha[threadIdx.x] : 1.f;
    sa = table;
  }
  __device__ __forceinline__ void stage() const { __syncthreads(); }
  template <int MAXC>
  __device__ __forceinline__ float pixel(float (&z)[MAXC], int C, float ssum, int t, float w, float inv_nnz, bool counts,
                                         float &lsum) const {
    // alpha at the label; a void label never indexes the table (its weight is zero)
    return focal_pixel<MAXC>(z, C, ssum, t, w, inv_nnz, counts, (t >= 0 && t < C) ? sa[t] : 1.f, gamma, lsum);
  }
};

// ------------------------------------------------------------------------------------------------------- the kernels
// The fallback above 32 classes (cross-entropy only), the classes looped over in memory:
// loss_partial[blockIdx.x] = sum over the block's rows of w*(-log clip(p_label))/nnz;
// dlogits = (p - onehot) * w / nnz ; label == C (void) -> the one-hot row is all zero (utils.py:129), so the row
// contributes neither loss nor gradient whatever its sample weight.
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float *__restrict__ x,
                                                           const float *__restrict__ labels,
                                                           const float *__restrict__ weights,
                                                           const float *__restrict__ nnz, float *__restrict__ probs,
                                                           float *__restrict__ dl, float *__restrict__ loss_part,
                                                           long M, int C) {
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  float lsum = 0.f;
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const float *r = x + (size_t)m * C;
    float mx = r[0];
    for (int c = 1; c < C; c++) mx = fmaxf(mx, r[c]);
    float s = 0.f;
    for (int c = 0; c < C; c++) s += expf(r[c] - mx);
    const float inv = 1.f / s;
    const int t = (int)labels[m];
    // void rows (label == C or out of range): the one-hot row is all zero, so loss AND gradient are zero whatever the
    // sample weight (utils.py:129 drops the last one-hot column)
    const float w = (t >= 0 && t < C) ? (weights ? weights[m] : 1.f) : 0.f;
    float psum = 0.f, pt = 0.f;
    for (int c = 0; c < C; c++) {
      const float pc = expf(r[c] - mx) * inv;
      psum += pc;
      if (c == t) pt = pc;
      if (probs) probs[(size_t)m * C + c] = pc;
    }
    float inside = 1.f;
    if (t >= 0 && t < C) {
      // Keras categorical_crossentropy on probabilities: renormalise, clip to [1e-7, 1-1e-7], -log
      float q = pt / psum;
      inside = dl3_clip_pass(q);
      q = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
      lsum += -logf(q) * w * inv_nnz;
    }
    if (dl) {
      const float gs = w * inv_nnz * inside;
      for (int c = 0; c < C; c++) dl[(size_t)m * C + c] = (expf(r[c] - mx) * inv - (c == t ? 1.f : 0.f)) * gs;
    }
  }
  block_loss_partial(wave_sum(lsum), loss_part);
}

// Loss tail, one pass over HBM.  Thread = pixel, logits held in registers (C <= 32); dlogits (and probs) leave
// through an LDS transpose so that the 256 x C floats of a workgroup are stored as contiguous float4s.
// UPSAMPLE: the logits are bilinearly interpolated on the fly from the low-resolution map (the resize_bilinear of
// deeplabv3p.py:439 / utils.py:190 fused in), so the full-resolution logits are never written or re-read.
template <class Term, bool UPSAMPLE, class... TermArgs>
__global__ __launch_bounds__(256) void row_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                  const float *__restrict__ weights, const float *__restrict__ nnz,
                                                  TermArgs... targs, float *__restrict__ dl,
                                                  float *__restrict__ loss_part, long M, int C, int Hi, int Wi, int Ho,
                                                  int Wo, float sy, float sx) {
  constexpr int MAXC = kHeadMaxC;
  __shared__ float tile[256 * MAXC];
  const Term term(targs..., C);
  term.stage();
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  float lsum = 0.f;
  for (long base = (long)blockIdx.x * 256; base < M; base += (long)gridDim.x * 256) {
    const long m = base + threadIdx.x;
    const bool ok = m < M;
    const long mc = ok ? m : M - 1;
    float z[MAXC];
    if (UPSAMPLE) {
      const PixelPos p = split_pixel(mc, Ho, Wo);
      const BilinearTaps taps(x + (size_t)p.n * Hi * Wi * C, p.oy, p.ox, sy, sx, Hi, Wi, C);
      taps.load<MAXC>(z, C, taps.lx.wl, taps.ly.wl);  // the weight TF states
    } else {
      // coalesced copy of the workgroup's 256 x C logits through LDS, then one row per thread (stride C is odd for
      // C = 21: conflict-free)
      const long nrem = min((long)256, M - base) * C;
      for (long i = threadIdx.x; i < nrem; i += 256) tile[i] = x[(size_t)base * C + i];
      __syncthreads();
#pragma unroll
      for (int c = 0; c < MAXC; c++) z[c] = tile[(ok ? threadIdx.x : 0) * C + min(c, C - 1)];
      __syncthreads();
    }
    const float ssum = softmax_exp<MAXC, float>(z, C);
    const int t = (int)labels[mc];
    const float w = (t >= 0 && t < C) ? (weights ? weights[mc] : 1.f) : 0.f;  // void rows: zero loss and gradient
    const float gs = term.template pixel<MAXC>(z, C, ssum, t, w, inv_nnz, ok, lsum);  // z: the probabilities
    const long nrem = min((long)256, M - base) * C;
    if constexpr (Term::kProbs) {
      if (term.probs) {
#pragma unroll
        for (int c = 0; c < MAXC; c++)
          if (c < C) tile[threadIdx.x * C + c] = z[c];
        __syncthreads();
        for (long i = threadIdx.x; i < nrem; i += 256) term.probs[(size_t)base * C + i] = tile[i];
        __syncthreads();
      }
    }
    if (!Term::kProbs || dl) {
#pragma unroll
      for (int c = 0; c < MAXC; c++)
        if (c < C) tile[threadIdx.x * C + c] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
      __syncthreads();
      for (long i = threadIdx.x; i < nrem; i += 256) dl[(size_t)base * C + i] = tile[i];
      __syncthreads();
    }
  }
  block_loss_partial(wave_sum(lsum), loss_part);
}

// prefetching form of the fold kernel: source floats per thread and source row, and output pixels per thread
constexpr int kPrefFloats = 12, kPrefPixels = 2;
// The training tail in one pass per output ROW: a workgroup owns output row (n, oy); phase 1 interpolates the
// low-resolution logits, evaluates softmax / loss / dlogits for the Wo pixels of the row and leaves dlogits in LDS;
// phase 2 folds the row onto the Wi input columns (the x half of the transposed bilinear resize, fixed summation
// order).  The full-resolution dlogits [N,Ho,Wo,C] (704 MB at 32x512x512x21) never exist: the kernel writes the
// x-folded rows [N,Ho,Wi,C] (8x smaller) and dl3_resize_bilinear_bwd_rows finishes with the y half.
// The two low-resolution logit rows an output row interpolates between are staged in LDS first: the 4 x C neighbour
// reads per pixel then come from LDS instead of the texture-address path (8 neighbouring pixels share them).
template <class Term, int MAXC, bool PREF, class... TermArgs>
__global__ __launch_bounds__(256, 2) void fold_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                      const float *__restrict__ weights, const float *__restrict__ nnz,
                                                      TermArgs... targs, float *__restrict__ xfold,
                                                      float *__restrict__ loss_part, int N, int C, int Hi, int Wi, int Ho,
                                                      int Wo, float sy, float sx) {
  extern __shared__ __attribute__((aligned(16))) float fold_tile[];  // [Wo][C] dlogits of the row, [2][Wi][C] source rows, [Wo] x lerp table
  float *src = fold_tile + (size_t)Wo * C;
  float *xw = src + 2 * (size_t)Wi * C;  // fractional x weight of every output column
  int *xlo = (int *)(xw + Wo);           // its lower source column
  for (int ox = threadIdx.x; ox < Wo; ox += 256) {
    const Lerp lx = tf1_lerp(ox, sx, Wi);
    xw[ox] = lx.w;
    xlo[ox] = lx.lo;
  }
  const Term term(targs..., C);
  term.stage();
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  float lsum = 0.f;
  // PREF (2 * Wi * C <= 2 * 256 * kPrefFloats source floats, Wo <= 256 * kPrefPixels pixels per row — the host checks): a row's global
  // operands — its two source rows, its labels and weights — are requested one row AHEAD into registers and only stored
  // to the LDS / consumed when their row starts.  Three workgroups of four waves per CU (52 KB of LDS each for a 512 x 21 row
  // over 32 source columns) hide little of a row's dependent round trips (source rows, labels inside phase 1).  Measured
  // (round 4, call 24, B=128: 65536 rows): 1.54 -> 1.36 ms per step; bit-identical results (tests).
  // (named registers, not arrays: the arrays stayed in scratch — 112 B per lane — whatever the indexing)
  static_assert(kPrefFloats == 12 && kPrefPixels == 2, "three float4 per thread and source row, two pixels per thread");
  float4 plo0, plo1, plo2, phi0, phi1, phi2;
  float plab0, plab1, pwt0, pwt1;
  plo0 = plo1 = plo2 = phi0 = phi1 = phi2 = make_float4(0.f, 0.f, 0.f, 0.f);
  plab0 = plab1 = pwt0 = pwt1 = 0.f;
  const int nq = Wi * C / 4;
  auto prefetch = [&](int row) __attribute__((always_inline)) {
    const int n = row / Ho, oy = row - n * Ho;
    const Lerp ly = tf1_lerp(oy, sy, Hi);
    const float4 *blo = reinterpret_cast<const float4 *>(x + ((size_t)n * Hi + ly.lo) * Wi * C);
    const float4 *bhi = reinterpret_cast<const float4 *>(x + ((size_t)n * Hi + ly.hi) * Wi * C);
    const int i0 = min((int)threadIdx.x, nq - 1), i1 = min((int)threadIdx.x + 256, nq - 1), i2 = min((int)threadIdx.x + 512, nq - 1);
    plo0 = blo[i0]; phi0 = bhi[i0];
    plo1 = blo[i1]; phi1 = bhi[i1];
    plo2 = blo[i2]; phi2 = bhi[i2];
    const size_t m0 = (size_t)row * Wo + min((int)threadIdx.x, Wo - 1), m1 = (size_t)row * Wo + min((int)threadIdx.x + 256, Wo - 1);
    plab0 = labels[m0]; plab1 = labels[m1];
    pwt0 = weights ? weights[m0] : 1.f; pwt1 = weights ? weights[m1] : 1.f;
  };
  if (PREF && (int)blockIdx.x < N * Ho) prefetch(blockIdx.x);
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {
    const int n = row / Ho, oy = row - n * Ho;
    const Lerp ly = tf1_lerp(oy, sy, Hi);
    float clab0 = 0.f, clab1 = 0.f, cwt0 = 0.f, cwt1 = 0.f;
    if constexpr (PREF) {
      float4 *s4lo = reinterpret_cast<float4 *>(src), *s4hi = reinterpret_cast<float4 *>(src + Wi * C);
      const int i0 = threadIdx.x, i1 = threadIdx.x + 256, i2 = threadIdx.x + 512;
      if (i0 < nq) { s4lo[i0] = plo0; s4hi[i0] = phi0; }
      if (i1 < nq) { s4lo[i1] = plo1; s4hi[i1] = phi1; }
      if (i2 < nq) { s4lo[i2] = plo2; s4hi[i2] = phi2; }
      clab0 = plab0; clab1 = plab1; cwt0 = pwt0; cwt1 = pwt1;
    } else {
      const float *b = x + (size_t)n * Hi * Wi * C;
      for (int i = threadIdx.x; i < Wi * C; i += 256) {
        src[i] = b[(size_t)ly.lo * Wi * C + i];
        src[Wi * C + i] = b[(size_t)ly.hi * Wi * C + i];
      }
    }
    __syncthreads();
    if (PREF && row + (int)gridDim.x < N * Ho) prefetch(row + gridDim.x);
    // one output pixel: interpolate, softmax, loss, dlogits into the LDS row (labf / wf: its label and sample weight)
    auto pixel = [&](int ox, float labf, float wf) __attribute__((always_inline)) {
      const BilinearTaps taps(src, ly, ox, sx, Wi, C);
      float z[MAXC];
      taps.load<MAXC>(z, C, taps.lx.w, ly.w);  // the resize kernels' weight
      const float ssum = softmax_exp<MAXC, float, true>(z, C);
      const int t = (int)labf;
      const float w = (t >= 0 && t < C) ? wf : 0.f;  // void rows: zero loss and gradient
      const float gs = term.template pixel<MAXC>(z, C, ssum, t, w, inv_nnz, true, lsum);
#pragma unroll
      for (int c = 0; c < MAXC; c++)
        if (c < C) fold_tile[ox * C + c] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
    };
    if constexpr (PREF) {
      // (a real loop: unrolled, the scheduler hoists every LDS operand of the row's pixels and spills — 256 VGPRs + scratch
      // against 65 for the loop)
#pragma nounroll
      for (int j = 0; j < 2; j++) {
        const int ox = threadIdx.x + 256 * j;
        if (ox < Wo) pixel(ox, j == 0 ? clab0 : clab1, j == 0 ? cwt0 : cwt1);
      }
    } else {
      for (int ox = threadIdx.x; ox < Wo; ox += 256) {
        const size_t m = (size_t)row * Wo + ox;
        pixel(ox, labels[m], weights ? weights[m] : 1.f);
      }
    }
    __syncthreads();
    // x fold: work item = (input column, group of 3 channels); the lerp of an output column comes from the table
    float *orow = xfold + (size_t)row * Wi * C;
    const int CG = (C + 2) / 3;
    for (int i = threadIdx.x; i < Wi * CG; i += 256) {
      const int ix = i / CG, c0 = (i - ix * CG) * 3;
      int ox0 = (int)floorf((float)(ix - 1) / sx) - 1, ox1 = (int)ceilf((float)(ix + 1) / sx) + 1;
      ox0 = max(ox0, 0);
      ox1 = min(ox1, Wo - 1);
      const int c1 = min(c0 + 1, C - 1), c2 = min(c0 + 2, C - 1);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      for (int ox = ox0; ox <= ox1; ++ox) {
        const int lo = xlo[ox], hi = min(lo + 1, Wi - 1);
        const float w = xw[ox];
        const float wx = (lo == ix ? 1.f - w : 0.f) + (hi == ix ? w : 0.f);
        const float *t = fold_tile + ox * C;
        a0 += wx * t[c0];
        a1 += wx * t[c1];
        a2 += wx * t[c2];
      }
      orow[ix * C + c0] = a0;
      if (c0 + 1 < C) orow[ix * C + c0 + 1] = a1;
      if (c0 + 2 < C) orow[ix * C + c0 + 2] = a2;
    }
    __syncthreads();
  }
  block_loss_partial(wave_sum(lsum), loss_part);
}

// Subpixel head, training tail in one pass (round 3): the loss evaluated straight on the UNshuffled output
// of the Subpixel convolution.  out[n, ia*r+q, ib*r+p, ch] = u[n, ia, ib, ch*r*r + p*r + q] (subpixel.py:81-87), so the C
// logits of one output pixel sit r*r floats apart in u: a workgroup stages PB consecutive pixels of one row (n, ia) of u
// in LDS (coalesced; element (pixel, ch, pq) at pixel*C*(r*r+1) + ch*(r*r+1) + pq as in phase_shift_lds_kernel), every
// thread evaluates output pixels (pixel, pq) from there (lanes = consecutive pq: conflict-free), writes the gradient
// back into the same LDS cells, and the tile leaves coalesced as du in u's own layout — the shuffled logits, the
// shuffled gradient and both phase-shift passes (4 x 2.8 GB at 128 x 512 x 512 x 21) never touch HBM.
template <class Term, int MAXC, class... TermArgs>
__global__ __launch_bounds__(256) void shuffle_kernel(const float *__restrict__ u, const float *__restrict__ labels,
                                                      const float *__restrict__ weights, const float *__restrict__ nnz,
                                                      TermArgs... targs, float *__restrict__ du,
                                                      float *__restrict__ loss_part, int H, int W, int C, int r, int PB) {
  extern __shared__ float tile[];
  const SubpixelTile T(C, r);
  const int rr = T.rr, P = T.P;
  const int wblocks = (W + PB - 1) / PB;
  const int ib0 = (blockIdx.x % wblocks) * PB;
  const long row = blockIdx.x / wblocks;  // n * H + ia
  const int ia = (int)(row % H);
  const long n = row / H;
  const int pb = min(PB, W - ib0);
  const size_t flat = ((size_t)row * W + ib0) * P;
  for (int t = threadIdx.x; t < pb * P; t += 256) { const int k = T.flat_cell(t); tile[k] = u[flat + t]; }
  const Term term(targs..., C);  // (what it stages waits at the tile's barrier)
  __syncthreads();
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  const int Wr = W * r;
  float lsum = 0.f;
  for (int o = threadIdx.x; o < pb * rr; o += 256) {
    const int px = o / rr, pq = o % rr, pp = pq / r, q = pq % r;
    float *cell = tile + T.cell(px, pq);
    float z[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = cell[min(c, C - 1) * (rr + 1)];
    const float ssum = softmax_exp<MAXC, float>(z, C);
    const size_t m = ((size_t)n * H * r + (size_t)ia * r + q) * Wr + (size_t)(ib0 + px) * r + pp;  // output pixel
    const int t = (int)labels[m];
    const float w = (t >= 0 && t < C) ? (weights ? weights[m] : 1.f) : 0.f;  // void rows: zero loss and gradient
    const float gs = term.template pixel<MAXC>(z, C, ssum, t, w, inv_nnz, true, lsum);
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) cell[c * (rr + 1)] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < pb * P; t += 256) { const int k = T.flat_cell(t); du[flat + t] = tile[k]; }
  block_loss_partial(wave_sum(lsum), loss_part);
}

// ------------------------------------------------------------------------------------------------------ the launchers
// one per body, behind the entry point's own argument checks; targs are the term's launch arguments
template <class Term, bool UPSAMPLE, class... TermArgs>
int launch_rows(const char *who, const float *x, const float *labels, const float *weights, const float *nnz, float *dl,
                float *loss_partial, long M, int C, int Hi, int Wi, int Ho, int Wo, void *stream, TermArgs... targs) {
  const float sy = UPSAMPLE ? (float)Hi / (float)Ho : 0.f, sx = UPSAMPLE ? (float)Wi / (float)Wo : 0.f;
  hipLaunchKernelGGL((row_kernel<Term, UPSAMPLE, TermArgs...>), dim3(dl3_rows_partials((int)M)), dim3(256), 0,
                     (hipStream_t)stream, x, labels, weights, nnz, targs..., dl, loss_partial, M, C, Hi, Wi, Ho, Wo, sy, sx);
  DL3_LAUNCH_CHECK(who);
  return DL3_OK;
}

template <class Term, class... TermArgs>
int launch_fold(const char *who, const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                float *dlogits_xfold, float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo, int C, void *stream,
                TermArgs... targs) {
  const size_t lds = (((size_t)Wo + 2 * (size_t)Wi) * C + 2 * (size_t)Wo) * sizeof(float);
  DL3_UNSUPPORTED(lds + Term::kLds > 64 * 1024, "%s: (%d + 2*%d) x %d floats%s exceed 64 KB of LDS", who, Wo, Wi, C,
                  Term::kLds ? " and alpha" : "");
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  const dim3 grid(dl3_xent_fold_partials(N, Ho));
  const char *pe = getenv("DL3_XENT_PREF");  // 0 = every row requests its own operands (tuning / test aid)
  // (float4 requests and LDS stores: source rows of whole float4s, 16-byte aligned; the source tile starts Wo * C floats in)
  const bool pref = (long)Wi * C <= 256L * kPrefFloats && Wo <= 256 * kPrefPixels && (Wi * C) % 4 == 0 &&
                    ((long)Wo * C) % 4 == 0 && aligned16(logits_lo) && !(pe && atoi(pe) == 0);
#define DL3_FOLD(MAXC_, PREF_)                                                                                       \
  hipLaunchKernelGGL((fold_kernel<Term, MAXC_, PREF_, TermArgs...>), grid, dim3(256), lds, (hipStream_t)stream,      \
                     logits_lo, labels, weights, nnz, targs..., dlogits_xfold, loss_partial, N, C, Hi, Wi, Ho, Wo, sy, sx)
  if (C <= 24) { if (pref) DL3_FOLD(24, true); else DL3_FOLD(24, false); }
  else { if (pref) DL3_FOLD(32, true); else DL3_FOLD(32, false); }
#undef DL3_FOLD
  DL3_LAUNCH_CHECK(who);
  return DL3_OK;
}

template <class Term, class... TermArgs>
int launch_shuffle(const char *who, const float *u, const float *labels, const float *weights, const float *nnz, float *du,
                   float *loss_partial, int N, int H, int W, int C, int r, void *stream, TermArgs... targs) {
  const int P = dl3_shuffle_xent_partials(N, H, W, C, r);
  DL3_UNSUPPORTED(P <= 0, "%s: a pixel of %d x %d x %d floats does not fit the LDS tile", who, C, r, r);
  const int PB = subpixel_tile_pixels(W, C, r, 8);
  const size_t lds = (size_t)PB * C * (r * r + 1) * sizeof(float);
#define DL3_SHUFFLE(MAXC_)                                                                                            \
  hipLaunchKernelGGL((shuffle_kernel<Term, MAXC_, TermArgs...>), dim3(P), dim3(256), lds, (hipStream_t)stream, u, labels, \
                     weights, nnz, targs..., du, loss_partial, H, W, C, r, PB)
  if (C <= 24) DL3_SHUFFLE(24); else DL3_SHUFFLE(32);
#undef DL3_SHUFFLE
  DL3_LAUNCH_CHECK(who);
  return DL3_OK;
}

int check_focal(const char *who, int C, float gamma) {
  DL3_CHECK_ARG(gamma >= 0.f && gamma <= 3.4e38f, "%s: gamma must be finite and >= 0, got %g", who, (double)gamma);
  DL3_UNSUPPORTED(C > kHeadMaxC, "%s: C=%d > 32", who, C);
  return DL3_OK;
}

}  // namespace

extern "C" int dl3_shuffle_xent_partials(int N, int H, int W, int C, int r) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || r <= 0) return 0;
  const int PB = subpixel_tile_pixels(W, C, r, 8);
  if (PB < 1) return 0;
  const long blocks = (long)N * H * dl3_cdiv(W, PB);
  return blocks < (1L << 30) ? (int)blocks : 0;
}

extern "C" int dl3_xent_fold_partials(int N, int Ho) {
  const long rows = (long)N * Ho;
  if (rows <= 0) return 0;
  return (int)(rows < 4096 ? rows : 4096);
}

extern "C" int dl3_softmax_xent(const float *logits, const float *labels, const float *weights, const float *nnz,
                                float *probs, float *dlogits, float *loss_partial, int M, int C, void *stream) {
  DL3_CHECK_ARG(logits && labels && nnz && loss_partial && M > 0 && C > 0, "softmax_xent: bad argument");
  if (C <= kHeadMaxC)
    return launch_rows<XentTerm, false>("softmax_xent", logits, labels, weights, nnz, dlogits, loss_partial, M, C, 0, 0, 0,
                                        0, stream, probs);
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(dl3_rows_partials(M)), dim3(256), 0, (hipStream_t)stream, logits, labels,
                     weights, nnz, probs, dlogits, loss_partial, (long)M, C);
  DL3_LAUNCH_CHECK("softmax_xent");
  return DL3_OK;
}

extern "C" int dl3_focal_xent(const float *logits, const float *labels, const float *weights, const float *nnz,
                              const float *alpha, float gamma, float *dlogits, float *loss_partial, int M, int C,
                              void *stream) {
  DL3_CHECK_ARG(logits && labels && nnz && dlogits && loss_partial && M > 0 && C > 0, "focal_xent: bad argument");
  if (int rc = check_focal("focal_xent", C, gamma)) return rc;
  return launch_rows<FocalTerm, false>("focal_xent", logits, labels, weights, nnz, dlogits, loss_partial, M, C, 0, 0, 0, 0,
                                       stream, alpha, gamma);
}

extern "C" int dl3_upsample_softmax_xent(const float *logits_lo, const float *labels, const float *weights,
                                         const float *nnz, float *probs, float *dlogits, float *loss_partial, int N,
                                         int Hi, int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "upsample_softmax_xent: bad argument");
  DL3_UNSUPPORTED(C > kHeadMaxC, "upsample_softmax_xent: C=%d > 32 (use resize_bilinear_fwd + softmax_xent)", C);
  return launch_rows<XentTerm, true>("upsample_softmax_xent", logits_lo, labels, weights, nnz, dlogits, loss_partial,
                                     (long)N * Ho * Wo, C, Hi, Wi, Ho, Wo, stream, probs);
}

extern "C" int dl3_upsample_focal_xent(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                                       const float *alpha, float gamma, float *dlogits, float *loss_partial, int N, int Hi,
                                       int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && dlogits && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 &&
                    C > 0 && (long)N * Ho * Wo <= 0x7fffffffL,
                "upsample_focal_xent: bad argument");
  if (int rc = check_focal("upsample_focal_xent", C, gamma)) return rc;
  return launch_rows<FocalTerm, true>("upsample_focal_xent", logits_lo, labels, weights, nnz, dlogits, loss_partial,
                                      (long)N * Ho * Wo, C, Hi, Wi, Ho, Wo, stream, alpha, gamma);
}

extern "C" int dl3_upsample_softmax_xent_fold(const float *logits_lo, const float *labels, const float *weights,
                                              const float *nnz, float *dlogits_xfold, float *loss_partial, int N,
                                              int Hi, int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && dlogits_xfold && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 &&
                    Wo > 0 && C > 0,
                "upsample_softmax_xent_fold: bad argument");
  DL3_UNSUPPORTED(C > kHeadMaxC, "upsample_softmax_xent_fold: C=%d > 32", C);
  return launch_fold<XentTerm>("upsample_softmax_xent_fold", logits_lo, labels, weights, nnz, dlogits_xfold, loss_partial,
                               N, Hi, Wi, Ho, Wo, C, stream);
}

extern "C" int dl3_upsample_focal_xent_fold(const float *logits_lo, const float *labels, const float *weights,
                                            const float *nnz, const float *alpha, float gamma, float *dlogits_xfold,
                                            float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo, int C,
                                            void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && dlogits_xfold && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 &&
                    Wo > 0 && C > 0,
                "upsample_focal_xent_fold: bad argument");
  if (int rc = check_focal("upsample_focal_xent_fold", C, gamma)) return rc;
  return launch_fold<FocalTerm>("upsample_focal_xent_fold", logits_lo, labels, weights, nnz, dlogits_xfold, loss_partial, N,
                                Hi, Wi, Ho, Wo, C, stream, alpha, gamma);
}

extern "C" int dl3_shuffle_softmax_xent(const float *u, const float *labels, const float *weights, const float *nnz,
                                        float *du, float *loss_partial, int N, int H, int W, int C, int r,
                                        void *stream) {
  DL3_CHECK_ARG(u && labels && nnz && du && loss_partial && N > 0 && H > 0 && W > 0 && C > 0 && r > 0,
                "shuffle_softmax_xent: bad argument");
  DL3_UNSUPPORTED(C > kHeadMaxC, "shuffle_softmax_xent: C=%d > 32 (use phase_shift + softmax_xent)", C);
  return launch_shuffle<XentTerm>("shuffle_softmax_xent", u, labels, weights, nnz, du, loss_partial, N, H, W, C, r, stream);
}

extern "C" int dl3_shuffle_focal_xent(const float *u, const float *labels, const float *weights, const float *nnz,
                                      const float *alpha, float gamma, float *du, float *loss_partial, int N, int H, int W,
                                      int C, int r, void *stream) {
  DL3_CHECK_ARG(u && labels && nnz && du && loss_partial && N > 0 && H > 0 && W > 0 && C > 0 && r > 0,
                "shuffle_focal_xent: bad argument");
  if (int rc = check_focal("shuffle_focal_xent", C, gamma)) return rc;
  return launch_shuffle<FocalTerm>("shuffle_focal_xent", u, labels, weights, nnz, du, loss_partial, N, H, W, C, r, stream,
                                   alpha, gamma);
}
