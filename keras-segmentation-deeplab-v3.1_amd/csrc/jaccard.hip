// jaccard.hip — the soft-Jaccard term next to the training cross-entropy: step loss CE + lambda * L_J,
//   u[b,m] = (w != 0 and label < C), p = softmax(z) (plain: no renormalise, no clip), y the one-hot label (void: zero)
//   I = sum_m u p y, S = sum_m u p, Y = sum_m u y, U = S + Y - I per (image, class); present = Y > 0; J = I / U
//   L_J = 1 - mean over the classes present somewhere of (mean over the images that hold the class of J)
// The term is not pixel-wise — a pixel's gradient needs the sums of its whole image — so the step takes three launches:
//   dl3_jaccard_sums_{plain,bilinear}         per-workgroup partial rows [B][P][3][C] in double, a workgroup inside ONE image
//   dl3_jaccard_coef                          folds them in a fixed order; kappa = present / (n_c n_legal), A = -kappa / U,
//                                             Bc = kappa I / U^2, coef[B][C][2] = (A, Bc) rounded to float once; lambda * L_J
//   dl3_{,upsample_}softmax_xent_jaccard      the cross-entropy tail of losstail.hip, the same arithmetic, plus
//                                             lambda u p_k (G_k - sum_c p_c G_c), G_c = A[c] at the label, else Bc[c]
// No atomics: two runs are bit-identical.  Ordinary vector stores only.
#include "tailmath.h"

namespace {

constexpr int kMaxHW = 1 << 30;   // pixels of one image: the 32-bit pixel index plus a grid stride stays in range

// a workgroup stays inside one image: B images share `total` workgroups of per_block pixels each
inline int per_image_blocks(long HW, int per_block, int B, int total) {
  return dl3_blocks(HW, per_block, (total + B - 1) / B);
}

// ---------------------------------------------------------------------------------------------------------------------
// sums pass.  grid = (P, B): workgroup (p, b) walks the pixels p*256 + tid, + P*256, ... of image b.  A lane keeps S and I
// per class in double and Y as an integer; the exponentials are fp32 (expf of z - max).  The four waves' sums meet in LDS
// and are added in wave order.
// ---------------------------------------------------------------------------------------------------------------------
template <int MAXC, bool UPSAMPLE>
__global__ __launch_bounds__(256) void jaccard_sums_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                           const float *__restrict__ weights,
                                                           double *__restrict__ partials, int HW, int C, int Hi, int Wi,
                                                           int Wo, float sy, float sx) {
  __shared__ double red[4][3 * MAXC];
  const int b = blockIdx.y;
  double accS[MAXC], accI[MAXC];
  int accY[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; c++) { accS[c] = 0.0; accI[c] = 0.0; accY[c] = 0; }
  const float *lab = labels + (size_t)b * HW;
  const float *wgt = weights ? weights + (size_t)b * HW : nullptr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const int t = (int)lab[i];
    const float w = wgt ? wgt[i] : 1.f;
    if (!(t >= 0 && t < C) || w == 0.f) continue;   // u = 0: nothing to add (NaN weights count, as in dl3_count_nonzero)
    float z[MAXC];
    // (own text on purpose, here and in the loss kernel below: with tailmath.h's BilinearTaps / softmax_exp / xent_pixel
    // the bilinear instantiations of both measured 2 - 4 % slower; as written they compile to the streams they had)
    if (UPSAMPLE) {
      const int oy = i / Wo, ox = i - oy * Wo;
      const Lerp ly = tf1_lerp(oy, sy, Hi), lx = tf1_lerp(ox, sx, Wi);
      const float *s = x + (size_t)b * Hi * Wi * C;
      const float *tl = s + ((size_t)ly.lo * Wi + lx.lo) * C, *tr = s + ((size_t)ly.lo * Wi + lx.hi) * C;
      const float *bl = s + ((size_t)ly.hi * Wi + lx.lo) * C, *br = s + ((size_t)ly.hi * Wi + lx.hi) * C;
#pragma unroll
      for (int c = 0; c < MAXC; c++) z[c] = bilerp_logit(tl, tr, bl, br, c, C, lx.wl, ly.wl);
    } else {
      const float *r = x + ((size_t)b * HW + i) * C;
#pragma unroll
      for (int c = 0; c < MAXC; c++) z[c] = r[min(c, C - 1)];
    }
    // the exponentials are fp32; their sum and the quotient are double (the accumulators are anyway: one fused
    // multiply-add per class where an add would stand), so p enters the sums without a rounding of its own
    float mx = z[0];
#pragma unroll
    for (int c = 1; c < MAXC; c++) mx = fmaxf(mx, (c < C) ? z[c] : z[0]);
    double ssum = 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      z[c] = (c < C) ? expf(z[c] - mx) : 0.f;
      ssum += (double)z[c];
    }
    const double inv = 1.0 / ssum;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      accS[c] = fma((double)z[c], inv, accS[c]);
      accI[c] = fma((c == t) ? (double)z[c] : 0.0, inv, accI[c]);
      accY[c] += (c == t);
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    const double i_ = wave_sum(accI[c]), s_ = wave_sum(accS[c]);
    const int y_ = wave_sum(accY[c]);
    if (lane == 0) {
      red[wv][c] = i_;
      red[wv][MAXC + c] = s_;
      red[wv][2 * MAXC + c] = (double)y_;
    }
  }
  __syncthreads();
  double *row = partials + ((size_t)b * gridDim.x + blockIdx.x) * 3 * C;   // [3][C]: I, S, Y
  for (int j = threadIdx.x; j < 3 * C; j += 256) {
    const int k = j / C, c = j - k * C;
    row[j] = ((red[0][k * MAXC + c] + red[1][k * MAXC + c]) + red[2][k * MAXC + c]) + red[3][k * MAXC + c];
  }
}

// sums[b][c][k] = sum over p of partials[b][p][k][c], ascending p.  grid = B
__global__ __launch_bounds__(128) void jaccard_fold_kernel(const double *__restrict__ partials, double *__restrict__ sums,
                                                           int P, int C) {
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < 3 * C; j += 128) {
    const int k = j / C, c = j - k * C;
    double s = 0.0;
    for (int p = 0; p < P; p++) s += partials[((size_t)b * P + p) * 3 * C + j];
    sums[((size_t)b * C + c) * 3 + k] = s;
  }
}

// one workgroup: thread c owns class c (n_c and the class's mean J, ascending b), thread 0 the mean over the classes
// (ascending c); then the table.  Everything in double; coef is rounded to float once.
__global__ __launch_bounds__(256) void jaccard_coef_kernel(const double *__restrict__ sums, float *__restrict__ coef,
                                                           double *__restrict__ stats, float *__restrict__ loss_row,
                                                           float lambda, int B, int C) {
  __shared__ double cls[kHeadMaxC];
  __shared__ int ncls[kHeadMaxC];
  __shared__ int s_legal;
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    int n = 0;
    double js = 0.0;
    for (int b = 0; b < B; b++) {
      const double *s = sums + ((size_t)b * C + c) * 3;
      const double I = s[0], S = s[1], Y = s[2];
      if (Y > 0.0) {
        n++;
        js += I / (S + Y - I);
      }
    }
    ncls[c] = n;
    cls[c] = n ? js / (double)n : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int legal = 0;
    double acc = 0.0;
    for (int c = 0; c < C; c++)
      if (ncls[c] > 0) { legal++; acc += cls[c]; }
    s_legal = legal;
    const double lj = legal ? 1.0 - acc / (double)legal : 0.0;   // an all-void batch: L_J = 0, zero gradient
    stats[0] = lj;
    stats[1] = (double)legal;
    stats[2] = (double)lambda * lj;
    if (loss_row) *loss_row = (float)((double)lambda * lj);
  }
  __syncthreads();
  const int legal = s_legal;
  for (int j = threadIdx.x; j < B * C; j += 256) {
    const int c = j % C;
    const double *s = sums + (size_t)j * 3;
    const double I = s[0], S = s[1], Y = s[2];
    double A = 0.0, Bc = 0.0;
    if (Y > 0.0) {   // then legal >= 1, n_c >= 1 and U >= Y >= 1
      const double kappa = 1.0 / ((double)ncls[c] * (double)legal), U = S + Y - I;
      A = -kappa / U;
      Bc = kappa * I / (U * U);
    }
    coef[2 * j] = (float)A;
    coef[2 * j + 1] = (float)Bc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// loss + gradient: the cross-entropy row_kernel of losstail.hip — thread = pixel, logits in registers, dlogits leave through an LDS
// transpose — over grid = (P, B), so that a workgroup stays inside one image and stages that image's 2C coefficients
// once.  The cross-entropy half repeats that kernel's arithmetic operation for operation (with an all-zero table the
// gradient is its gradient bit for bit); loss_part carries the cross-entropy alone.
// ---------------------------------------------------------------------------------------------------------------------
template <bool UPSAMPLE>
__global__ __launch_bounds__(256) void xent32_jaccard_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                             const float *__restrict__ weights,
                                                             const float *__restrict__ nnz, const float *__restrict__ coef,
                                                             float lambda, float *__restrict__ dl,
                                                             float *__restrict__ loss_part, int HW, int C, int Hi, int Wi,
                                                             int Wo, float sy, float sx) {
  constexpr int MAXC = kHeadMaxC;
  __shared__ float tile[256 * MAXC];
  __shared__ float cA[MAXC], cB[MAXC];
  __shared__ float red[4];
  const int b = blockIdx.y;
  if (threadIdx.x < MAXC) {
    const int c = threadIdx.x;
    cA[c] = c < C ? coef[((size_t)b * C + c) * 2] : 0.f;
    cB[c] = c < C ? coef[((size_t)b * C + c) * 2 + 1] : 0.f;
  }
  __syncthreads();
  const float inv_nnz = 1.f / fmaxf(*nnz, DL3_NNZ_FLOOR);
  const float *lab = labels + (size_t)b * HW;
  const float *wgt = weights ? weights + (size_t)b * HW : nullptr;
  float lsum = 0.f;
  for (int base = blockIdx.x * 256; base < HW; base += gridDim.x * 256) {
    const int i = base + threadIdx.x;
    const bool ok = i < HW;
    const int ic = ok ? i : HW - 1;
    const int nrem = min(256, HW - base) * C;
    const size_t row0 = ((size_t)b * HW + base) * C;
    float z[MAXC];
    if (UPSAMPLE) {
      const int oy = ic / Wo, ox = ic - oy * Wo;
      const Lerp ly = tf1_lerp(oy, sy, Hi), lx = tf1_lerp(ox, sx, Wi);
      const float *s = x + (size_t)b * Hi * Wi * C;
      const float *tl = s + ((size_t)ly.lo * Wi + lx.lo) * C, *tr = s + ((size_t)ly.lo * Wi + lx.hi) * C;
      const float *bl = s + ((size_t)ly.hi * Wi + lx.lo) * C, *br = s + ((size_t)ly.hi * Wi + lx.hi) * C;
#pragma unroll
      for (int c = 0; c < MAXC; c++) z[c] = bilerp_logit(tl, tr, bl, br, c, C, lx.wl, ly.wl);
    } else {
      for (int j = threadIdx.x; j < nrem; j += 256) tile[j] = x[row0 + j];
      __syncthreads();
#pragma unroll
      for (int c = 0; c < MAXC; c++) z[c] = tile[(ok ? threadIdx.x : 0) * C + min(c, C - 1)];
      __syncthreads();
    }
    float mx = z[0];
#pragma unroll
    for (int c = 1; c < MAXC; c++) mx = fmaxf(mx, (c < C) ? z[c] : z[0]);
    float ssum = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      z[c] = (c < C) ? expf(z[c] - mx) : 0.f;
      ssum += z[c];
    }
    const float inv = 1.f / ssum;
    const int t = (int)lab[ic];
    const bool legal = t >= 0 && t < C;
    const float w = legal ? (wgt ? wgt[ic] : 1.f) : 0.f;  // void rows: zero loss and gradient
    float psum = 0.f, pt = 0.f, dotb = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      z[c] *= inv;  // probability
      psum += z[c];
      pt = (c == t) ? z[c] : pt;
      dotb += z[c] * cB[c];
    }
    float inside = 1.f;
    if (ok && legal) {
      float q = pt / psum;
      inside = dl3_clip_pass(q);
      q = fminf(fmaxf(q, 1e-7f), 1.f - 1e-7f);
      lsum += -logf(q) * w * inv_nnz;
    }
    const float gs = w * inv_nnz * inside;
    // the Jaccard half: lambda u p_k (G_k - sum_c p_c G_c); G differs from Bc at the label only
    const float at = legal ? cA[t] : 0.f, bt = legal ? cB[t] : 0.f;
    const float dot = dotb + pt * (at - bt);
    const float js = (w != 0.f) ? lambda : 0.f;   // lambda u
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) {
        const float ce = (z[c] - (c == t ? 1.f : 0.f)) * gs;
        const float jk = js * (z[c] * ((c == t ? at : cB[c]) - dot));
        // a zero term is not added: +0 would turn a cross-entropy gradient of -0 into +0
        tile[threadIdx.x * C + c] = (jk != 0.f) ? ce + jk : ce;
      }
    __syncthreads();
    for (int j = threadIdx.x; j < nrem; j += 256) dl[row0 + j] = tile[j];
    __syncthreads();
  }
  const float wsum = wave_sum(lsum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

inline int sums_blocks(int B, long HW) { return per_image_blocks(HW, 256 * 8, B, 2048); }
inline int loss_blocks(int B, long HW) { return per_image_blocks(HW, 256, B, 1024); }

template <bool UPSAMPLE>
int launch_sums(const float *x, const float *labels, const float *weights, double *partials, int B, int HW, int C, int Hi,
                int Wi, int Wo, float sy, float sx, hipStream_t st) {
  dim3 grid(sums_blocks(B, HW), B);
#define DL3_JSUMS(MAXC)                                                                                               \
  hipLaunchKernelGGL((jaccard_sums_kernel<MAXC, UPSAMPLE>), grid, dim3(256), 0, st, x, labels, weights, partials, HW, C, \
                     Hi, Wi, Wo, sy, sx)
  DL3_DISPATCH_MAXC(C, DL3_JSUMS);
#undef DL3_JSUMS
  return DL3_OK;
}

// B images of HW pixels: B fits grid.y, a pixel index plus a grid stride and the flat index B * HW fit 32 bits
int check_images(const char *who, int B, long HW) {
  DL3_CHECK_ARG(B <= 65535 && HW <= kMaxHW && B * HW <= 0x7fffffffL, "%s: %d images of %ld pixels exceed the grid", who, B,
                HW);
  return DL3_OK;
}
int check_lambda(const char *who, float lambda) {
  DL3_CHECK_ARG(lambda >= 0.f && lambda <= 3.4e38f, "%s: lambda must be finite and >= 0, got %g", who, (double)lambda);
  return DL3_OK;
}

}  // namespace

extern "C" int dl3_jaccard_partials(int B, int HW) { return (B > 0 && HW > 0) ? sums_blocks(B, HW) : 0; }
extern "C" int dl3_jaccard_loss_partials(int B, int HW) { return (B > 0 && HW > 0) ? B * loss_blocks(B, HW) : 0; }

extern "C" int dl3_jaccard_sums_plain(const float *logits, const float *labels, const float *weights, double *partials,
                                      int B, int HW, int C, void *stream) {
  DL3_CHECK_ARG(logits && labels && partials && B > 0 && HW > 0 && C > 0, "jaccard_sums_plain: bad argument");
  if (int rc = check_images("jaccard_sums_plain", B, HW)) return rc;
  DL3_UNSUPPORTED(C > kHeadMaxC, "jaccard_sums_plain: C=%d > 32", C);
  launch_sums<false>(logits, labels, weights, partials, B, HW, C, 0, 0, 0, 0.f, 0.f, (hipStream_t)stream);
  DL3_LAUNCH_CHECK("jaccard_sums_plain");
  return DL3_OK;
}

extern "C" int dl3_jaccard_sums_bilinear(const float *logits_lo, const float *labels, const float *weights,
                                         double *partials, int N, int Hi, int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && partials && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "jaccard_sums_bilinear: bad argument");
  if (int rc = check_images("jaccard_sums_bilinear", N, (long)Ho * Wo)) return rc;
  DL3_UNSUPPORTED(C > kHeadMaxC, "jaccard_sums_bilinear: C=%d > 32 (use resize_bilinear_fwd + jaccard_sums_plain)", C);
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  launch_sums<true>(logits_lo, labels, weights, partials, N, Ho * Wo, C, Hi, Wi, Wo, sy, sx, (hipStream_t)stream);
  DL3_LAUNCH_CHECK("jaccard_sums_bilinear");
  return DL3_OK;
}

extern "C" int dl3_jaccard_coef(const double *partials, int P, int B, int C, float lambda, double *sums, float *coef,
                                double *stats, float *loss_row, void *stream) {
  DL3_CHECK_ARG(partials && sums && coef && stats && P > 0 && B > 0 && C > 0, "jaccard_coef: bad argument");
  if (int rc = check_lambda("jaccard_coef", lambda)) return rc;
  DL3_UNSUPPORTED(C > kHeadMaxC, "jaccard_coef: C=%d > 32", C);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(jaccard_fold_kernel, dim3(B), dim3(128), 0, st, partials, sums, P, C);
  hipLaunchKernelGGL(jaccard_coef_kernel, dim3(1), dim3(256), 0, st, sums, coef, stats, loss_row, lambda, B, C);
  DL3_LAUNCH_CHECK("jaccard_coef");
  return DL3_OK;
}

extern "C" int dl3_softmax_xent_jaccard(const float *logits, const float *labels, const float *weights, const float *nnz,
                                        const float *coef, float lambda, float *dlogits, float *loss_partial, int B,
                                        int HW, int C, void *stream) {
  DL3_CHECK_ARG(logits && labels && nnz && coef && dlogits && loss_partial && B > 0 && HW > 0 && C > 0,
                "softmax_xent_jaccard: bad argument");
  if (int rc = check_images("softmax_xent_jaccard", B, HW)) return rc;
  if (int rc = check_lambda("softmax_xent_jaccard", lambda)) return rc;
  DL3_UNSUPPORTED(C > kHeadMaxC, "softmax_xent_jaccard: C=%d > 32", C);
  hipLaunchKernelGGL((xent32_jaccard_kernel<false>), dim3(loss_blocks(B, HW), B), dim3(256), 0, (hipStream_t)stream, logits,
                     labels, weights, nnz, coef, lambda, dlogits, loss_partial, HW, C, 0, 0, 0, 0.f, 0.f);
  DL3_LAUNCH_CHECK("softmax_xent_jaccard");
  return DL3_OK;
}

extern "C" int dl3_upsample_softmax_xent_jaccard(const float *logits_lo, const float *labels, const float *weights,
                                                 const float *nnz, const float *coef, float lambda, float *dlogits,
                                                 float *loss_partial, int N, int Hi, int Wi, int Ho, int Wo, int C,
                                                 void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && nnz && coef && dlogits && loss_partial && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 &&
                    Wo > 0 && C > 0,
                "upsample_softmax_xent_jaccard: bad argument");
  if (int rc = check_images("upsample_softmax_xent_jaccard", N, (long)Ho * Wo)) return rc;
  if (int rc = check_lambda("upsample_softmax_xent_jaccard", lambda)) return rc;
  DL3_UNSUPPORTED(C > kHeadMaxC, "upsample_softmax_xent_jaccard: C=%d > 32", C);
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  const int HW = Ho * Wo;
  hipLaunchKernelGGL((xent32_jaccard_kernel<true>), dim3(loss_blocks(N, HW), N), dim3(256), 0, (hipStream_t)stream,
                     logits_lo, labels, weights, nnz, coef, lambda, dlogits, loss_partial, HW, C, Hi, Wi, Wo, sy, sx);
  DL3_LAUNCH_CHECK("upsample_softmax_xent_jaccard");
  return DL3_OK;
}
