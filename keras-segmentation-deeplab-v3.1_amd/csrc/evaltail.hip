// evaltail.hip — the evaluation tail: validation loss sums, metric counts, confusion matrix and (optionally) the argmax
// mask from the LOW-resolution logits plus labels in one pass.  The evaluation twin of the training tails in losstail.hip
// (dl3_upsample_softmax_xent_fold, dl3_shuffle_softmax_xent): the full-resolution logits / probabilities never exist.
//   bilinear  logits_lo [N,Hi,Wi,C] -> TF1 legacy bilinear resize in registers (bit-identical to dl3_resize_bilinear_fwd)
//   shuffle   u [N,H,W,C*r*r]       -> Subpixel._phase_shift by index (a pure permutation)
//   plain     logits [N*HW,C]       -> any other graph, and C > 32
// Per pixel: the expression of dl3_softmax_xent (softmax, Keras' renormalise + clip to [1e-7, 1-1e-7], void label -> 0)
// and the first-maximum argmax of dl3_argmax.  Float sums: per-workgroup partials (double), folded per image in a fixed
// order in double by a second launch — no float atomics, two runs are bit-identical.  Integer counts: a per-workgroup
// LDS histogram (LDS integer atomics), then ONE global integer atomic per non-zero bin per workgroup — integer sums do
// not depend on arrival order.
#include "tailmath.h"

namespace {

constexpr int kMaxClasses = 255;   // dl3_seg_counts' limit; the plain form serves it
constexpr int kBand = 8;           // output rows per workgroup (bilinear form)
constexpr int kStageBytes = 48 * 1024;

// (the bilinear form's weights, tailmath.h: the MASK has to reproduce dl3_resize_bilinear_fwd bit for bit and takes .w, the
// loss follows the formula TF states — its logits are interpolated with .wl)
// a lane's running sums.  The loss terms are fp32 values; they are ADDED in double (one v_fma_f64 per pixel), so that
// what is left of the result's error is the per-pixel arithmetic alone and not the order of a float32 summation
struct Acc {
  double lsum;
  int nz;
};

// one pixel with its C <= MAXC logits in registers: argmax (first maximum), loss term, histogram bins
template <int MAXC>
__device__ __forceinline__ int eval_pixel(float (&z)[MAXC], int C, float labf, float wf, Acc &a, int *hist, bool conf,
                                          int am_given = -1) {
  float mx = z[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < MAXC; c++)
    if (c < C && z[c] > mx) { mx = z[c]; am = c; }
  if (am_given >= 0) am = am_given;   // bilinear form: the prediction comes from the bit-pinned logits
  const float ssum = exp_sum<MAXC, float>(z, C, mx);
  const int t = (int)labf;
  const bool tok = (t >= 0 && t < C);
  const ClassProbs p = class_probs<MAXC>(z, ssum, t);
  if (tok) {
    // Keras categorical_crossentropy on probabilities: renormalise, clip to [1e-7, 1-1e-7], -log
    // (the quotient and the logarithm in double: one of each per pixel, and the sum is then as good as its fp32 terms)
    double q = (double)p.pt / (double)p.psum;
    q = fmin(fmax(q, 1e-7), 1.0 - 1e-7);
    a.lsum += -log(q) * (double)wf;
  }
  a.nz += (wf != 0.f);
  if (tok) {
    atomicAdd(&hist[t], 1);
    if (t == am) atomicAdd(&hist[2 * C + t], 1);
    if (conf) atomicAdd(&hist[3 * C + t * C + am], 1);
  }
  atomicAdd(&hist[C + am], 1);
  return am;
}

// end of a workgroup: its loss partial, its share of count(w != 0), its non-zero histogram bins
__device__ __forceinline__ void flush(Acc a, const int *hist, int C, int n, double *part_slot, int *nnz, int *counts,
                                      long long *conf, bool conf_in_lds) {
  __shared__ double red[4];
  __shared__ int redn[4];
  const double ls = wave_sum(a.lsum);
  const int nz = wave_sum(a.nz);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = ls;
    redn[threadIdx.x >> 6] = nz;
  }
  __syncthreads();   // also orders the LDS histogram atomics before the reads below
  if (threadIdx.x == 0) {
    *part_slot = ((red[0] + red[1]) + red[2]) + red[3];
    const int tot = redn[0] + redn[1] + redn[2] + redn[3];
    if (tot) atomicAdd(&nnz[n], tot);
  }
  for (int i = threadIdx.x; i < 3 * C; i += 256)
    if (hist[i]) atomicAdd(&counts[n * 3 * C + i], hist[i]);
  if (conf && conf_in_lds)
    for (int i = threadIdx.x; i < C * C; i += 256)
      if (hist[3 * C + i])
        atomicAdd(reinterpret_cast<unsigned long long *>(conf) + i, (unsigned long long)hist[3 * C + i]);
}

// ---------------------------------------------------------------------------------------------------------------------
// bilinear form.  grid = (bands of kBand output rows, N).  The two source rows an output row interpolates between are
// staged in LDS (re-staged only when they change: 8 output rows share them at 64 -> 512).  VEC = 4: a lane owns four
// neighbouring pixels — one 16-byte load of labels, one of weights, one 16-byte store of the mask.
// ---------------------------------------------------------------------------------------------------------------------
template <int MAXC, int VEC>
__global__ __launch_bounds__(256) void eval_bilinear_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                            const float *__restrict__ weights, double *__restrict__ part,
                                                            int *__restrict__ nnz, int *__restrict__ counts,
                                                            long long *__restrict__ conf, int *__restrict__ mask, int Hi,
                                                            int Wi, int Ho, int Wo, int C, float sy, float sx) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *src = smem;                                  // [2][Wi][C]
  int *hist = reinterpret_cast<int *>(smem + 2 * Wi * C);  // [3][C] + [C][C]
  const int n = blockIdx.y;
  const int oy0 = blockIdx.x * kBand, oy1 = min(oy0 + kBand, Ho);
  const int nh = 3 * C + (conf ? C * C : 0);
  for (int i = threadIdx.x; i < nh; i += 256) hist[i] = 0;
  const float *xb = x + (size_t)n * Hi * Wi * C;
  Acc a = {0.0, 0};
  const int G = (Wo + VEC - 1) / VEC;   // lane items per output row
  for (int oyA = oy0; oyA < oy1;) {
    // the rows of the band that interpolate between the same two source rows share one staging and one item space
    const Lerp lyA = tf1_lerp(oyA, sy, Hi);
    int oyB = oyA + 1;
    while (oyB < oy1) {
      const Lerp l = tf1_lerp(oyB, sy, Hi);
      if (l.lo != lyA.lo || l.hi != lyA.hi) break;
      ++oyB;
    }
    __syncthreads();   // uniform over the workgroup: everybody is done with the previous pair of rows
    for (int i = threadIdx.x; i < Wi * C; i += 256) {
      src[i] = xb[(size_t)lyA.lo * Wi * C + i];
      src[Wi * C + i] = xb[(size_t)lyA.hi * Wi * C + i];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (oyB - oyA) * G; idx += 256) {
      const int ro = idx / G, g = idx - ro * G;
      const int oy = oyA + ro;
      const Lerp ly = tf1_lerp(oy, sy, Hi);
      const size_t row = ((size_t)n * Ho + oy) * Wo;
      float lab[VEC], wt[VEC];
      int mk[VEC];
      if constexpr (VEC == 4) {
        const f32x4 l4 = ld4(labels + row + g * 4);
        lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
        if (weights) {
          const f32x4 w4 = ld4(weights + row + g * 4);
          wt[0] = w4.x; wt[1] = w4.y; wt[2] = w4.z; wt[3] = w4.w;
        } else {
          wt[0] = wt[1] = wt[2] = wt[3] = 1.f;
        }
      } else {
        lab[0] = labels[row + g];
        wt[0] = weights ? weights[row + g] : 1.f;
      }
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const int ox = g * VEC + k;
        const BilinearTaps taps(src, ly, ox, sx, Wi, C);
        const Lerp &lx = taps.lx;
        float z[MAXC];
        float mmx = 0.f;
        int am = 0;
#pragma unroll
        for (int c = 0; c < MAXC; c++) {
          const int cc = min(c, C - 1);
          const float a0 = taps.tl[cc], a1 = taps.tr[cc], b0 = taps.bl[cc], b1 = taps.br[cc];
          const float zm = bilerp(a0, a1, b0, b1, lx.w, ly.w);   // dl3_resize_bilinear_fwd's value
          if (c == 0) mmx = zm;
          else if (c < C && zm > mmx) { mmx = zm; am = c; }
          z[c] = bilerp(a0, a1, b0, b1, lx.wl, ly.wl);
        }
        mk[k] = eval_pixel<MAXC>(z, C, lab[k], wt[k], a, hist, conf != nullptr, am);
      }
      if (mask) {
        if constexpr (VEC == 4) {
          *reinterpret_cast<int4 *>(mask + row + g * 4) = make_int4(mk[0], mk[1], mk[2], mk[3]);
        } else {
          mask[row + g] = mk[0];
        }
      }
    }
    oyA = oyB;
  }
  flush(a, hist, C, n, part + (size_t)n * gridDim.x + blockIdx.x, nnz, counts, conf, true);
}

// ---------------------------------------------------------------------------------------------------------------------
// shuffle form.  out[n, ia*r+q, ib*r+p, ch] = u[n, ia, ib, ch*r*r + p*r + q]  (subpixel.py:81-87).  grid = (H * tiles of
// PB pixels of an unshuffled row, N): the tile is read as PB * C*r*r contiguous floats and laid out in LDS with an odd
// channel stride (r*r + 1), as dl3_phase_shift's LDS kernel does; a lane then owns one shuffled pixel, and consecutive
// lanes walk along a shuffled image row (coalesced labels / weights / mask).
// ---------------------------------------------------------------------------------------------------------------------
template <int MAXC>
__global__ __launch_bounds__(256) void eval_shuffle_kernel(const float *__restrict__ u, const float *__restrict__ labels,
                                                           const float *__restrict__ weights, double *__restrict__ part,
                                                           int *__restrict__ nnz, int *__restrict__ counts,
                                                           long long *__restrict__ conf, int *__restrict__ mask, int H,
                                                           int W, int C, int r, int PB) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const SubpixelTile T(C, r);
  const int rr = T.rr, P = T.P;
  float *tile = smem;                                   // [PB][C][rr + 1]
  int *hist = reinterpret_cast<int *>(smem + PB * T.LP);
  const int n = blockIdx.y;
  const int wblocks = (W + PB - 1) / PB;
  const int ia = blockIdx.x / wblocks, ib0 = (blockIdx.x - ia * wblocks) * PB;
  const int pb = min(PB, W - ib0);
  const int nh = 3 * C + (conf ? C * C : 0);
  for (int i = threadIdx.x; i < nh; i += 256) hist[i] = 0;
  const float *srcp = u + (((size_t)n * H + ia) * W + ib0) * P;
  for (int t = threadIdx.x; t < pb * P; t += 256) { const int k = T.flat_cell(t); tile[k] = srcp[t]; }
  __syncthreads();
  Acc a = {0.0, 0};
  const int run = pb * r;   // shuffled pixels of the tile along one image row
  const size_t Wr = (size_t)W * r;
  for (int idx = threadIdx.x; idx < r * run; idx += 256) {
    const int q = idx / run, v = idx - q * run;
    const int px = v / r, p = v - px * r;
    const size_t m = ((size_t)n * H * r + (size_t)ia * r + q) * Wr + (size_t)ib0 * r + v;
    const float *tp = tile + T.cell(px, p * r + q);
    float z[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = tp[min(c, C - 1) * (rr + 1)];
    const int am = eval_pixel<MAXC>(z, C, labels[m], weights ? weights[m] : 1.f, a, hist, conf != nullptr);
    if (mask) mask[m] = am;
  }
  flush(a, hist, C, n, part + (size_t)n * gridDim.x + blockIdx.x, nnz, counts, conf, true);
}

// ---------------------------------------------------------------------------------------------------------------------
// plain form: materialised logits [N*HW][C], any C <= 255.  One pixel per lane, its row read from memory twice (maximum,
// then the sum) — the fallback path.  The confusion bins live in LDS for C <= 32 and go straight to global integer
// atomics above that.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_plain_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                         const float *__restrict__ weights, double *__restrict__ part,
                                                         int *__restrict__ nnz, int *__restrict__ counts,
                                                         long long *__restrict__ conf, int *__restrict__ mask, int HW,
                                                         int C) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int *hist = reinterpret_cast<int *>(smem);
  const int n = blockIdx.y;
  const bool lds_conf = conf && C <= kHeadMaxC;
  const int nh = 3 * C + (lds_conf ? C * C : 0);
  for (int i = threadIdx.x; i < nh; i += 256) hist[i] = 0;
  __syncthreads();
  Acc a = {0.0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const size_t m = (size_t)n * HW + i;
    const float *row = x + m * C;
    float mx = row[0];
    int am = 0;
    for (int c = 1; c < C; c++)
      if (row[c] > mx) { mx = row[c]; am = c; }
    float ssum = 0.f;
    for (int c = 0; c < C; c++) ssum += expf(row[c] - mx);
    const float inv = 1.f / ssum;
    const int t = (int)labels[m];
    const bool tok = (t >= 0 && t < C);
    const float wf = weights ? weights[m] : 1.f;
    float psum = 0.f;
    for (int c = 0; c < C; c++) psum += expf(row[c] - mx) * inv;
    if (tok) {
      double q = (double)(expf(row[t] - mx) * inv) / (double)psum;
      q = fmin(fmax(q, 1e-7), 1.0 - 1e-7);
      a.lsum += -log(q) * (double)wf;
      atomicAdd(&hist[t], 1);
      if (t == am) atomicAdd(&hist[2 * C + t], 1);
      if (lds_conf) atomicAdd(&hist[3 * C + t * C + am], 1);
      else if (conf) atomicAdd(reinterpret_cast<unsigned long long *>(conf) + (size_t)t * C + am, 1ull);
    }
    a.nz += (wf != 0.f);
    atomicAdd(&hist[C + am], 1);
    if (mask) mask[m] = am;
  }
  flush(a, hist, C, n, part + (size_t)n * gridDim.x + blockIdx.x, nnz, counts, conf, lds_conf);
}

// loss_sum[n] = sum of the image's P partials: lane l adds partials l, l + 64, ... in double, then a fixed butterfly
__global__ __launch_bounds__(64) void eval_fold_kernel(const double *__restrict__ part, int P, double *__restrict__ loss_sum) {
  const double *p = part + (size_t)blockIdx.x * P;
  double s = 0.0;
  for (int i = threadIdx.x; i < P; i += 64) s += p[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss_sum[blockIdx.x] = s;
}

inline int hist_ints(int C, bool conf) { return 3 * C + (conf ? C * C : 0); }

inline int plain_chunks(int HW) {
  int c = dl3_cdiv(HW, 256 * 4);
  if (c < 1) c = 1;
  if (c > 256) c = 256;
  return c;
}

int check_common(const char *who, const void *x, const void *labels, const void *partials, const void *loss_sum,
                 const void *nnz, const void *counts, int N, int C, int maxc) {
  DL3_CHECK_ARG(x && labels && partials && loss_sum && nnz && counts && N > 0, "%s: bad argument", who);
  DL3_CHECK_ARG(C > 0 && C <= maxc, "%s: classes must be in 1..%d, got %d", who, maxc, C);
  return DL3_OK;
}

// nnz and counts start at zero every call (a kernel, not a memset: the launch sequence is captured into a hipGraph)
__global__ __launch_bounds__(256) void eval_zero_kernel(int *__restrict__ nnz, int n0, int *__restrict__ counts, int n1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n0) nnz[i] = 0;
  if (i < n1) counts[i] = 0;
}

void begin(int *nnz, int *counts, int N, int C, hipStream_t st) {
  const int n1 = N * 3 * C;
  hipLaunchKernelGGL(eval_zero_kernel, dim3(dl3_cdiv(n1, 256)), dim3(256), 0, st, nnz, N, counts, n1);
}

}  // namespace

extern "C" int dl3_eval_tail_bilinear_partials(int N, int Hi, int Wi, int Ho, int Wo, int C) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || C > kHeadMaxC) return 0;
  if ((size_t)2 * Wi * C * 4 > (size_t)kStageBytes) return 0;
  return dl3_cdiv(Ho, kBand);
}

extern "C" int dl3_eval_tail_bilinear(const float *logits_lo, const float *labels, const float *weights, double *partials,
                                      double *loss_sum, int *nnz, int *counts, long long *confusion, int *mask, int N,
                                      int Hi, int Wi, int Ho, int Wo, int C, void *stream) {
  int rc = check_common("eval_tail_bilinear", logits_lo, labels, partials, loss_sum, nnz, counts, N, C, kHeadMaxC);
  if (rc != DL3_OK) return rc;
  const int P = dl3_eval_tail_bilinear_partials(N, Hi, Wi, Ho, Wo, C);
  DL3_UNSUPPORTED(P <= 0, "eval_tail_bilinear: %dx%d -> %dx%d x %d is not supported by the fused form (use "
                  "resize_bilinear_fwd + eval_tail_plain)", Hi, Wi, Ho, Wo, C);
  hipStream_t st = (hipStream_t)stream;
  begin(nnz, counts, N, C, st);
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  const size_t lds = ((size_t)2 * Wi * C + hist_ints(C, confusion != nullptr)) * 4;
  const bool vec = (Wo % 4 == 0) && aligned16(labels) && (!weights || aligned16(weights)) && (!mask || aligned16(mask));
  dim3 grid(P, N);
#define DL3_EVAL_BIL(MAXC, VEC)                                                                                      \
  hipLaunchKernelGGL((eval_bilinear_kernel<MAXC, VEC>), grid, dim3(256), lds, st, logits_lo, labels, weights, partials, \
                     nnz, counts, confusion, mask, Hi, Wi, Ho, Wo, C, sy, sx)
#define DL3_EVAL_BIL_VEC(MAXC) if (vec) DL3_EVAL_BIL(MAXC, 4); else DL3_EVAL_BIL(MAXC, 1)
  DL3_DISPATCH_MAXC(C, DL3_EVAL_BIL_VEC);
#undef DL3_EVAL_BIL_VEC
#undef DL3_EVAL_BIL
  hipLaunchKernelGGL(eval_fold_kernel, dim3(N), dim3(64), 0, st, partials, P, loss_sum);
  DL3_LAUNCH_CHECK("eval_tail_bilinear");
  return DL3_OK;
}

extern "C" int dl3_eval_tail_shuffle_partials(int N, int H, int W, int C, int r) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > kHeadMaxC || r <= 0) return 0;
  const int pb = shuffle_pb(W, C, r);
  if (pb < 1) return 0;
  return H * dl3_cdiv(W, pb);
}

extern "C" int dl3_eval_tail_shuffle(const float *u, const float *labels, const float *weights, double *partials,
                                     double *loss_sum, int *nnz, int *counts, long long *confusion, int *mask, int N,
                                     int H, int W, int C, int r, void *stream) {
  int rc = check_common("eval_tail_shuffle", u, labels, partials, loss_sum, nnz, counts, N, C, kHeadMaxC);
  if (rc != DL3_OK) return rc;
  const int P = dl3_eval_tail_shuffle_partials(N, H, W, C, r);
  DL3_UNSUPPORTED(P <= 0, "eval_tail_shuffle: a pixel of %d x %d x %d floats does not fit the LDS tile (use phase_shift + "
                  "eval_tail_plain)", C, r, r);
  hipStream_t st = (hipStream_t)stream;
  begin(nnz, counts, N, C, st);
  const int pb = shuffle_pb(W, C, r);
  const size_t lds = ((size_t)pb * C * (r * r + 1) + hist_ints(C, confusion != nullptr)) * 4;
  dim3 grid(P, N);
#define DL3_EVAL_SHF(MAXC)                                                                                          \
  hipLaunchKernelGGL((eval_shuffle_kernel<MAXC>), grid, dim3(256), lds, st, u, labels, weights, partials, nnz, counts, \
                     confusion, mask, H, W, C, r, pb)
  DL3_DISPATCH_MAXC(C, DL3_EVAL_SHF);
#undef DL3_EVAL_SHF
  hipLaunchKernelGGL(eval_fold_kernel, dim3(N), dim3(64), 0, st, partials, P, loss_sum);
  DL3_LAUNCH_CHECK("eval_tail_shuffle");
  return DL3_OK;
}

extern "C" int dl3_eval_tail_plain_partials(int N, int HW, int C) {
  if (N <= 0 || HW <= 0 || C <= 0 || C > kMaxClasses) return 0;
  return plain_chunks(HW);
}

extern "C" int dl3_eval_tail_plain(const float *logits, const float *labels, const float *weights, double *partials,
                                   double *loss_sum, int *nnz, int *counts, long long *confusion, int *mask, int N, int HW,
                                   int C, void *stream) {
  int rc = check_common("eval_tail_plain", logits, labels, partials, loss_sum, nnz, counts, N, C, kMaxClasses);
  if (rc != DL3_OK) return rc;
  DL3_CHECK_ARG(HW > 0, "eval_tail_plain: bad argument");
  const int P = plain_chunks(HW);
  hipStream_t st = (hipStream_t)stream;
  begin(nnz, counts, N, C, st);
  const size_t lds = (size_t)hist_ints(C, confusion != nullptr && C <= kHeadMaxC) * 4;
  hipLaunchKernelGGL(eval_plain_kernel, dim3(P, N), dim3(256), lds, st, logits, labels, weights, partials, nnz, counts,
                     confusion, mask, HW, C);
  hipLaunchKernelGGL(eval_fold_kernel, dim3(N), dim3(64), 0, st, partials, P, loss_sum);
  DL3_LAUNCH_CHECK("eval_tail_plain");
  return DL3_OK;
}
