// focal.hip — the focal loss in every form of the training loss tail: per pixel, with q the clipped
// renormalised probability of the label as misc.hip's loss kernels form it,
//   l = alpha[t] (1 - q)^gamma (-log q),  L = sum_m w l / nnz,
//   dL/dz[m,k] = (w / nnz) inside alpha[t] mu(q) (p_k - [k = t]),  mu = (1 - q)^gamma + gamma q (1 - q)^(gamma - 1) (-log q)
// The loss is pixel-wise and keeps the cross-entropy's normaliser, so each of the four kernels below is its counterpart in
// misc.hip — the same grid, the same staging, the same partial sums, the same stores — with tailmath.h's focal_pixel where
// that one calls xent_pixel, and alpha staged once per workgroup in LDS (a lane reads it at its own label).  With
// gamma = 0 and alpha null the gradient is the counterpart's bit for bit (tests/test_gpu_focal.py pins it).
//   dl3_focal_xent                 xent32_kernel<false>   materialised logits, dlogits through an LDS transpose
//   dl3_upsample_focal_xent        xent32_kernel<true>    the final resize fused in (TF's stated weight)
//   dl3_upsample_focal_xent_fold   xent32_fold_kernel     both variants, with and without the one-row-ahead prefetch
//   dl3_shuffle_focal_xent         shuffle_xent_kernel    the unshuffled Subpixel output, du in its own layout
// No atomics: two runs are bit-identical.  Ordinary vector stores only.  gamma is a launch argument, alpha a device pointer.
#include "tailmath.h"

namespace {

// alpha -> LDS, 1.f past C - 1 and where there is no alpha; the barrier is the caller's first use
__device__ __forceinline__ void stage_alpha(float *sa, const float *__restrict__ alpha, int C) {
  if (threadIdx.x < kHeadMaxC) sa[threadIdx.x] = (alpha && (int)threadIdx.x < C) ? alpha[threadIdx.x] : 1.f;
  __syncthreads();
}
// alpha at the label; a void label never indexes the table (its weight is zero)
__device__ __forceinline__ float alpha_at(const float *sa, int t, int C) { return (t >= 0 && t < C) ? sa[t] : 1.f; }

// thread = pixel, logits in registers; dlogits leave through an LDS transpose (xent32_kernel without the probs output)
template <bool UPSAMPLE>
__global__ __launch_bounds__(256) void focal32_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                      const float *__restrict__ weights, const float *__restrict__ nnz,
                                                      const float *__restrict__ alpha, float gamma, float *__restrict__ dl,
                                                      float *__restrict__ loss_part, long M, int C, int Hi, int Wi, int Ho,
                                                      int Wo, float sy, float sx) {
  constexpr int MAXC = kHeadMaxC;
  __shared__ float tile[256 * MAXC];
  __shared__ float sa[kHeadMaxC];
  stage_alpha(sa, alpha, C);
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
    const float gs = focal_pixel<MAXC>(z, C, ssum, t, w, inv_nnz, ok, alpha_at(sa, t, C), gamma, lsum);
    const long nrem = min((long)256, M - base) * C;
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) tile[threadIdx.x * C + c] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
    __syncthreads();
    for (long i = threadIdx.x; i < nrem; i += 256) dl[(size_t)base * C + i] = tile[i];
    __syncthreads();
  }
  block_loss_partial(wave_sum(lsum), loss_part);
}

constexpr int kPS = 12;  // prefetching form of the row kernel: source floats per thread and source row ...
constexpr int kPP = 2;   // ... and output pixels per thread (misc.hip's XENT_PS, XENT_PP)

// one workgroup per output row: interpolate, softmax, loss, dlogits into the LDS row, then the row folded onto the Wi
// input columns (xent32_fold_kernel, both variants: see there for the staging, the prefetch and the fold)
template <int MAXC, bool PREF>
__global__ __launch_bounds__(256, 2) void focal32_fold_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                              const float *__restrict__ weights,
                                                              const float *__restrict__ nnz, const float *__restrict__ alpha,
                                                              float gamma, float *__restrict__ xfold,
                                                              float *__restrict__ loss_part, int N, int C, int Hi, int Wi,
                                                              int Ho, int Wo, float sy, float sx) {
  extern __shared__ __attribute__((aligned(16))) float fold_tile[];  // [Wo][C] dlogits of the row, [2][Wi][C] source rows, [Wo] x lerp table
  __shared__ float sa[kHeadMaxC];
  float *src = fold_tile + (size_t)Wo * C;
  float *xw = src + 2 * (size_t)Wi * C;  // fractional x weight of every output column
  int *xlo = (int *)(xw + Wo);           // its lower source column
  for (int ox = threadIdx.x; ox < Wo; ox += 256) {
    const Lerp lx = tf1_lerp(ox, sx, Wi);
    xw[ox] = lx.w;
    xlo[ox] = lx.lo;
  }
  stage_alpha(sa, alpha, C);
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  float lsum = 0.f;
  static_assert(kPS == 12 && kPP == 2, "three float4 per thread and source row, two pixels per thread");
  float4 plo0, plo1, plo2, phi0, phi1, phi2;   // (named registers, not arrays: arrays stayed in scratch there)
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
    auto pixel = [&](int ox, float labf, float wf) __attribute__((always_inline)) {
      const BilinearTaps taps(src, ly, ox, sx, Wi, C);
      float z[MAXC];
      taps.load<MAXC>(z, C, taps.lx.w, ly.w);  // the resize kernels' weight
      const float ssum = softmax_exp<MAXC, float, true>(z, C);
      const int t = (int)labf;
      const float w = (t >= 0 && t < C) ? wf : 0.f;  // void rows: zero loss and gradient
      const float gs = focal_pixel<MAXC>(z, C, ssum, t, w, inv_nnz, true, alpha_at(sa, t, C), gamma, lsum);
#pragma unroll
      for (int c = 0; c < MAXC; c++)
        if (c < C) fold_tile[ox * C + c] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
    };
    if constexpr (PREF) {
#pragma nounroll
      for (int j = 0; j < 2; j++) {   // (a real loop: unrolled, the counterpart spilled)
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

// the unshuffled Subpixel output: a tile of PB pixels of one row of u in LDS, the gradient written back into the same
// cells, the tile leaves as du in u's layout (shuffle_xent_kernel)
template <int MAXC>
__global__ __launch_bounds__(256) void shuffle_focal_kernel(const float *__restrict__ u, const float *__restrict__ labels,
                                                            const float *__restrict__ weights,
                                                            const float *__restrict__ nnz, const float *__restrict__ alpha,
                                                            float gamma, float *__restrict__ du,
                                                            float *__restrict__ loss_part, int H, int W, int C, int r,
                                                            int PB) {
  extern __shared__ float tile[];
  __shared__ float sa[kHeadMaxC];
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
  stage_alpha(sa, alpha, C);
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
    const float gs = focal_pixel<MAXC>(z, C, ssum, t, w, inv_nnz, true, alpha_at(sa, t, C), gamma, lsum);
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) cell[c * (rr + 1)] = (z[c] - (c == t ? 1.f : 0.f)) * gs;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < pb * P; t += 256) { const int k = T.flat_cell(t); du[flat + t] = tile[k]; }
  block_loss_partial(wave_sum(lsum), loss_part);
}

int check_focal(const char *who, int C, float gamma) {
  DL3_CHECK_ARG(gamma >= 0.f && gamma <= 3.4e38f, "%s: gamma must be finite and >= 0, got %g", who, (double)gamma);
  DL3_UNSUPPORTED(C > kHeadMaxC, "%s: C=%d > 32", who, C);
  return DL3_OK;
}

}  // namespace

extern "C" int dl3_focal_xent(const float *logits, const float *labels, const float *weights, const float *nnz,
                              const float *alpha, float gamma, float *dlogits, float *loss_partial, int M, int C,
                              void *stream) {
  DL3_CHECK_ARG(logits && labels && nnz && dlogits && loss_partial && M > 0 && C > 0, "focal_xent: bad argument");
  if (int rc = check_focal("focal_xent", C, gamma)) return rc;
  hipLaunchKernelGGL((focal32_kernel<false>), dim3(dl3_rows_partials(M)), dim3(256), 0, (hipStream_t)stream, logits, labels,
                     weights, nnz, alpha, gamma, dlogits, loss_partial, (long)M, C, 0, 0, 0, 0, 0.f, 0.f);
  DL3_LAUNCH_CHECK("focal_xent");
  return DL3_OK;
}

extern "C" int dl3_upsample_focal_xent(const float *logits_lo, const float *labels, const float *weights, const float *nnz,
                                       const float *alpha, float gamma, float *dlogits, float *loss_partial, int N, int Hi,
                                       int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && dlogits && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 &&
                    C > 0 && (long)N * Ho * Wo <= 0x7fffffffL,
                "upsample_focal_xent: bad argument");
  if (int rc = check_focal("upsample_focal_xent", C, gamma)) return rc;
  const long M = (long)N * Ho * Wo;
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  hipLaunchKernelGGL((focal32_kernel<true>), dim3(dl3_rows_partials((int)M)), dim3(256), 0, (hipStream_t)stream, logits_lo,
                     labels, weights, nnz, alpha, gamma, dlogits, loss_partial, M, C, Hi, Wi, Ho, Wo, sy, sx);
  DL3_LAUNCH_CHECK("upsample_focal_xent");
  return DL3_OK;
}

extern "C" int dl3_upsample_focal_xent_fold(const float *logits_lo, const float *labels, const float *weights,
                                            const float *nnz, const float *alpha, float gamma, float *dlogits_xfold,
                                            float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo, int C,
                                            void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && dlogits_xfold && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 &&
                    Wo > 0 && C > 0,
                "upsample_focal_xent_fold: bad argument");
  if (int rc = check_focal("upsample_focal_xent_fold", C, gamma)) return rc;
  // the counterpart's rule, with room for alpha beside the row
  const size_t lds = (((size_t)Wo + 2 * (size_t)Wi) * C + 2 * (size_t)Wo) * sizeof(float);
  DL3_UNSUPPORTED(lds + kHeadMaxC * sizeof(float) > 64 * 1024,
                  "upsample_focal_xent_fold: (%d + 2*%d) x %d floats and alpha exceed 64 KB of LDS", Wo, Wi, C);
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  const dim3 grid(dl3_xent_fold_partials(N, Ho));
  const char *pe = getenv("DL3_XENT_PREF");  // 0 = every row requests its own operands (tuning / test aid)
  const bool pref = (long)Wi * C <= 256L * kPS && Wo <= 256 * kPP && (Wi * C) % 4 == 0 && ((long)Wo * C) % 4 == 0 &&
                    aligned16(logits_lo) && !(pe && atoi(pe) == 0);
#define DL3_FOCAL(MAXC_, PREF_)                                                                                         \
  hipLaunchKernelGGL((focal32_fold_kernel<MAXC_, PREF_>), grid, dim3(256), lds, (hipStream_t)stream, logits_lo, labels, \
                     weights, nnz, alpha, gamma, dlogits_xfold, loss_partial, N, C, Hi, Wi, Ho, Wo, sy, sx)
  if (C <= 24) { if (pref) DL3_FOCAL(24, true); else DL3_FOCAL(24, false); }
  else { if (pref) DL3_FOCAL(32, true); else DL3_FOCAL(32, false); }
#undef DL3_FOCAL
  DL3_LAUNCH_CHECK("upsample_focal_xent_fold");
  return DL3_OK;
}

extern "C" int dl3_shuffle_focal_xent(const float *u, const float *labels, const float *weights, const float *nnz,
                                      const float *alpha, float gamma, float *du, float *loss_partial, int N, int H, int W,
                                      int C, int r, void *stream) {
  DL3_CHECK_ARG(u && labels && nnz && du && loss_partial && N > 0 && H > 0 && W > 0 && C > 0 && r > 0,
                "shuffle_focal_xent: bad argument");
  if (int rc = check_focal("shuffle_focal_xent", C, gamma)) return rc;
  const int P = dl3_shuffle_xent_partials(N, H, W, C, r);
  DL3_UNSUPPORTED(P <= 0, "shuffle_focal_xent: a pixel of %d x %d x %d floats does not fit the LDS tile", C, r, r);
  const int PB = subpixel_tile_pixels(W, C, r, 8);
  const size_t lds = (size_t)PB * C * (r * r + 1) * sizeof(float);
  if (C <= 24)
    hipLaunchKernelGGL(shuffle_focal_kernel<24>, dim3(P), dim3(256), lds, (hipStream_t)stream, u, labels, weights, nnz, alpha,
                       gamma, du, loss_partial, H, W, C, r, PB);
  else
    hipLaunchKernelGGL(shuffle_focal_kernel<32>, dim3(P), dim3(256), lds, (hipStream_t)stream, u, labels, weights, nnz, alpha,
                       gamma, du, loss_partial, H, W, C, r, PB);
  DL3_LAUNCH_CHECK("shuffle_focal_xent");
  return DL3_OK;
}
