// mine.hip — online hard-example mining in front of the training loss tails (DeepLab's top_k_percent_pixels /
// hard_example_mining_step, restated from memory of deeplab/utils/train_utils.py): the step trains on the k largest
// per-pixel losses only.  Three passes produce what the loss kernels of losstail.hip already take as device pointers, mined
// sample weights w' and a mined normaliser n':
//   dl3_pixel_xent_{plain,bilinear,shuffle}   v[m] = w[m] * -log clip(p_label, 1e-7, 1 - 1e-7), 0 for a void label, from
//                                             the same three sources the training tails read
//   dl3_topk_threshold                        k from the schedule (device step counter), tau = the k-th largest v: a radix
//                                             select over the bit patterns of the non-negative floats, digits 11 + 11 + 10
//   dl3_mine_weights                          w' = w where v >= tau and v > 0, else 0; n' = count, in integers
// Integer atomics only (LDS histograms, one global atomic per non-empty bin per workgroup; integer sums do not depend on
// arrival order): two runs are bit-identical, and ties at tau are all kept.
#include "tailmath.h"

namespace {

constexpr int kBins = 2048;      // bins of the widest digit (11 bits): 8 KB of LDS per workgroup
constexpr int kHistThreads = 1024;
// workspace (32-bit words): 16 words of state, then the three digit histograms
enum { S_K = 0, S_RANK = 1, S_PREFIX = 2, S_TAU = 3, S_COUNT = 4, S_WORDS = 16 };   // S_COUNT: Engine.MINE_WS_COUNT
constexpr int kWsWords = S_WORDS + 3 * kBins;
__host__ __device__ constexpr int digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bins(int pass) { return pass == 2 ? 1024 : 2048; }

// ---------------------------------------------------------------------------------------------------------------------
// per-pixel loss.  One pixel with its C <= MAXC logits in registers.  The exponentials are fp32 (accurate expf), their sum,
// the quotient and the logarithm are double (once per pixel, as the evaluation tail does: fp32 logf carries a one-sided
// bias); -log is rounded to fp32 once and v = w * l is ONE fp32 product.  Whatever is not > 0 — a void label, a zero
// weight, a product that underflowed, -0, NaN — is stored as +0, so that v's bit pattern orders as an unsigned integer.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float finish_pixel(float et, double ssum, float wf) {
  double q = (double)et / ssum;
  q = fmin(fmax(q, 1e-7), 1.0 - 1e-7);
  const float l = (float)(-log(q));
  const float v = __fmul_rn(wf, l);
  return v > 0.f ? v : 0.f;
}
template <int MAXC>
__device__ __forceinline__ float pixel_loss(float (&z)[MAXC], int C, float labf, float wf) {
  const int t = (int)labf;
  const float mx = logit_max<MAXC>(z, C);
  // (not softmax_exp: only the label's exponential is kept, so that the others need no register past the sum — kept in
  // place for a later select, they cost pixel_shuffle_kernel<32> 15 VGPRs and its 64-register step)
  double ssum = 0.0;
  float et = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    const float e = (c < C) ? expf(z[c] - mx) : 0.f;
    ssum += (double)e;
    et = (c == t) ? e : et;
  }
  if (!(t >= 0 && t < C)) return 0.f;
  return finish_pixel(et, ssum, wf);
}

// plain form: materialised logits [M][C], any C.  One pixel per lane, its row read twice (maximum, then the sum).
__global__ __launch_bounds__(256) void pixel_plain_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                          const float *__restrict__ weights, float *__restrict__ v,
                                                          long M, int C) {
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const int t = (int)labels[m];
    float out = 0.f;
    if (t >= 0 && t < C) {
      const float *r = x + (size_t)m * C;
      float mx = r[0];
      for (int c = 1; c < C; c++) mx = fmaxf(mx, r[c]);
      double ssum = 0.0;
      for (int c = 0; c < C; c++) ssum += (double)expf(r[c] - mx);
      out = finish_pixel(expf(r[t] - mx), ssum, weights ? weights[m] : 1.f);
    }
    v[m] = out;
  }
}

// bilinear form: the low-resolution logits in front of the final resize, interpolated in registers with the weight TF
// states (.wl) — the logits dl3_upsample_softmax_xent's loss sees.  Thread = output pixel.
template <int MAXC>
__global__ __launch_bounds__(256) void pixel_bilinear_kernel(const float *__restrict__ x, const float *__restrict__ labels,
                                                             const float *__restrict__ weights, float *__restrict__ v,
                                                             long M, int C, int Hi, int Wi, int Ho, int Wo, float sy,
                                                             float sx) {
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const PixelPos p = split_pixel(m, Ho, Wo);
    const BilinearTaps taps(x + (size_t)p.n * Hi * Wi * C, p.oy, p.ox, sy, sx, Hi, Wi, C);
    float z[MAXC];
    taps.load<MAXC>(z, C, taps.lx.wl, taps.ly.wl);
    v[m] = pixel_loss<MAXC>(z, C, labels[m], weights ? weights[m] : 1.f);
  }
}

// shuffle form: the UNshuffled output u [N,H,W,C*r*r] of the Subpixel convolution.  grid = (H * tiles of PB pixels of an
// unshuffled row, N); the tile is staged in LDS in the SubpixelTile layout, a lane owns one shuffled pixel and consecutive
// lanes walk along a shuffled image row (coalesced labels / weights / v), as dl3_eval_tail_shuffle does.
template <int MAXC>
__global__ __launch_bounds__(256) void pixel_shuffle_kernel(const float *__restrict__ u, const float *__restrict__ labels,
                                                            const float *__restrict__ weights, float *__restrict__ v,
                                                            int H, int W, int C, int r, int PB) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const SubpixelTile T(C, r);
  const int rr = T.rr, P = T.P;
  const int n = blockIdx.y;
  const int wblocks = (W + PB - 1) / PB;
  const int ia = blockIdx.x / wblocks, ib0 = (blockIdx.x - ia * wblocks) * PB;
  const int pb = min(PB, W - ib0);
  const float *srcp = u + (((size_t)n * H + ia) * W + ib0) * P;
  for (int t = threadIdx.x; t < pb * P; t += 256) { const int k = T.flat_cell(t); tile[k] = srcp[t]; }
  __syncthreads();
  const int run = pb * r;   // shuffled pixels of the tile along one image row
  const size_t Wr = (size_t)W * r;
  for (int idx = threadIdx.x; idx < r * run; idx += 256) {
    const int q = idx / run, s = idx - q * run;
    const int px = s / r, p = s - px * r;
    const size_t m = ((size_t)n * H * r + (size_t)ia * r + q) * Wr + (size_t)ib0 * r + s;
    const float *tp = tile + T.cell(px, p * r + q);
    float z[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = tp[min(c, C - 1) * (rr + 1)];
    v[m] = pixel_loss<MAXC>(z, C, labels[m], weights ? weights[m] : 1.f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// selection
// ---------------------------------------------------------------------------------------------------------------------
// the histograms, the count and the state start at zero every call (a kernel, not a memset: the launches are captured)
__global__ __launch_bounds__(256) void mine_zero_kernel(unsigned int *__restrict__ ws) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kWsWords) ws[i] = 0u;
}

// one histogram increment per valid lane; a wave whose valid lanes all hit ONE bin (zeros of a void region, equal values)
// adds their count once instead of serialising 64 LDS atomics on one address.  Called by every lane of the wave.
__device__ __forceinline__ void hist_add(unsigned int *h, unsigned int bin, bool valid) {
  const unsigned long long act = __ballot(valid);
  if (act == 0ull) return;   // wave-uniform
  const int first = __ffsll((long long)act) - 1;
  const unsigned int b0 = (unsigned int)__shfl((int)bin, first, 64);
  const unsigned long long same = __ballot(valid && bin == b0);
  if (same == act) {         // wave-uniform
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[b0], (unsigned int)__popcll(act));
  } else if (valid) {
    atomicAdd(&h[bin], 1u);
  }
}

// digit histogram of pass PASS over the values whose higher digits equal the prefix the earlier passes chose
template <int PASS>
__global__ __launch_bounds__(kHistThreads) void mine_hist_kernel(const float *__restrict__ v, long N,
                                                                 unsigned int *__restrict__ ws) {
  __shared__ unsigned int h[kBins];
  constexpr int shift = digit_shift(PASS), bins = digit_bins(PASS);
  unsigned int *hist = ws + S_WORDS + PASS * kBins;
  // k == 0 selects nothing: the later passes have no prefix to refine
  if (PASS > 0 && ws[S_K] == 0u) return;
  const unsigned int prefix = PASS > 0 ? ws[S_PREFIX] : 0u;
  constexpr int up = PASS == 0 ? 0 : digit_shift(PASS - 1);   // bits above this digit: bits >> up
  for (int i = threadIdx.x; i < bins; i += kHistThreads) h[i] = 0u;
  __syncthreads();
  const unsigned int *bits = reinterpret_cast<const unsigned int *>(v);
  // wave-uniform trip count: every lane reaches hist_add
  for (long base = (long)blockIdx.x * kHistThreads; base < N; base += (long)gridDim.x * kHistThreads) {
    const long i = base + threadIdx.x;
    const bool ok = i < N;
    const unsigned int b = ok ? bits[i] : 0u;
    const bool valid = ok && (PASS == 0 || (b >> up) == prefix);
    hist_add(h, (b >> shift) & (unsigned int)(bins - 1), valid);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kHistThreads)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// the schedule, every operation ONE rounded float32 operation (no contraction): the numpy-float32 oracle gives the same k
__device__ __forceinline__ unsigned int schedule_k(float p, int S, unsigned long long s, long N) {
  float pct = p;
  if (S > 0) {
    const float ratio = fminf(1.f, __fdiv_rn((float)s, (float)S));
    pct = __fadd_rn(__fmul_rn(ratio, p), __fsub_rn(1.f, ratio));
  }
  const float x = __fmul_rn(pct, (float)N);       // 0 <= x <= 2^31: the conversion below is in range
  const long k = (long)truncf(x);
  return (unsigned int)(k > N ? N : k);
}

// the small fold that picks the bin: one workgroup of 256 threads walks the pass's histogram from the top; the bin in
// which the cumulative count reaches the rank holds the k-th largest value.  Pass 0 computes k first.
template <int PASS>
__global__ __launch_bounds__(256) void mine_pick_kernel(unsigned int *__restrict__ ws, float p, int S,
                                                        const unsigned long long *__restrict__ step, long N,
                                                        int *__restrict__ k_out, float *__restrict__ tau_out) {
  constexpr int bins = digit_bins(PASS), per = bins / 256;
  __shared__ unsigned int wtot[4];
  __shared__ unsigned int s_rank;
  const unsigned int *hist = ws + S_WORDS + PASS * kBins;
  if (PASS == 0) {
    if (threadIdx.x == 0) s_rank = schedule_k(p, S, step ? step[0] : 0ull, N);
  } else if (threadIdx.x == 0) {
    s_rank = ws[S_RANK];
  }
  __syncthreads();
  const unsigned int rank = s_rank;   // >= 1 below: the k-th largest among the values that share the prefix
  const unsigned int k = PASS == 0 ? rank : ws[S_K];
  if (k == 0u) {                      // uniform over the workgroup
    if (threadIdx.x == 0 && PASS == 0) {
      ws[S_K] = 0u;
      *k_out = 0;
      *tau_out = __builtin_inff();    // nothing is selected: dl3_mine_weights looks at k
    }
    return;
  }
  // thread t owns bins [top - per*t - (per-1), top - per*t], the highest first
  const int top = bins - 1 - per * (int)threadIdx.x;
  unsigned int own = 0;
#pragma unroll
  for (int j = 0; j < per; j++) own += hist[top - j];
  unsigned int inc = own;             // inclusive scan over the workgroup, in thread order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int up = (unsigned int)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wtot[wv] = inc;
  __syncthreads();
  for (int w = 0; w < wv; w++) inc += wtot[w];
  const unsigned int exc = inc - own;
  if (exc < rank && rank <= inc) {    // exactly one thread: the total is >= rank
    unsigned int cum = exc;
    int bin = top;
    for (int j = 0; j < per; j++) {
      const unsigned int c = hist[top - j];
      if (cum + c >= rank) { bin = top - j; break; }
      cum += c;
    }
    const unsigned int prefix = ((PASS == 0 ? 0u : ws[S_PREFIX]) << (PASS == 2 ? 10 : 11)) | (unsigned int)bin;
    ws[S_PREFIX] = prefix;
    ws[S_RANK] = rank - cum;
    if (PASS == 0) {
      ws[S_K] = k;
      *k_out = (int)k;
    }
    if (PASS == 2) {
      ws[S_TAU] = prefix;
      *tau_out = __uint_as_float(prefix);
    }
  }
}

// w' = w where (v >= tau and v > 0), else 0; the count goes to ws[S_COUNT] (one integer atomic per workgroup)
__global__ __launch_bounds__(256) void mine_weights_kernel(const float *__restrict__ v, const float *__restrict__ w,
                                                           const float *__restrict__ tau, const int *__restrict__ k,
                                                           float *__restrict__ wout, unsigned int *__restrict__ ws,
                                                           long N) {
  __shared__ unsigned int red[4];
  const float t = *tau;
  const bool any = *k > 0;
  unsigned int c = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const float vi = v[i];
    const bool m = any && vi >= t && vi > 0.f;
    wout[i] = m ? (w ? w[i] : 1.f) : 0.f;
    c += m;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int tot = red[0] + red[1] + red[2] + red[3];
    if (tot) atomicAdd(&ws[S_COUNT], tot);
  }
}
// ... converted once (the integer stays in the workspace for Engine.mining_record)
__global__ void mine_count_kernel(const unsigned int *__restrict__ ws, float *__restrict__ nnz) {
  *nnz = (float)ws[S_COUNT];
}

}  // namespace

extern "C" int dl3_pixel_xent_plain(const float *logits, const float *labels, const float *weights, float *v, int M,
                                    int C, void *stream) {
  DL3_CHECK_ARG(logits && labels && v && M > 0 && C > 0, "pixel_xent_plain: bad argument");
  hipLaunchKernelGGL(pixel_plain_kernel, dim3(dl3_blocks(M, 256, 8192)), dim3(256), 0, (hipStream_t)stream, logits,
                     labels, weights, v, (long)M, C);
  DL3_LAUNCH_CHECK("pixel_xent_plain");
  return DL3_OK;
}

extern "C" int dl3_pixel_xent_bilinear(const float *logits_lo, const float *labels, const float *weights, float *v, int N,
                                       int Hi, int Wi, int Ho, int Wo, int C, void *stream) {
  DL3_CHECK_ARG(logits_lo && labels && v && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "pixel_xent_bilinear: bad argument");
  DL3_UNSUPPORTED(C > kHeadMaxC, "pixel_xent_bilinear: C=%d > 32 (use resize_bilinear_fwd + pixel_xent_plain)", C);
  const long M = (long)N * Ho * Wo;
  DL3_CHECK_ARG(M <= 0x7fffffffL, "pixel_xent_bilinear: %ld pixels exceed 2^31 - 1", M);
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  dim3 grid(dl3_blocks(M, 256, 16384));
#define DL3_PIX_BIL(MAXC)                                                                                            \
  hipLaunchKernelGGL((pixel_bilinear_kernel<MAXC>), grid, dim3(256), 0, (hipStream_t)stream, logits_lo, labels, weights, \
                     v, M, C, Hi, Wi, Ho, Wo, sy, sx)
  DL3_DISPATCH_MAXC(C, DL3_PIX_BIL);
#undef DL3_PIX_BIL
  DL3_LAUNCH_CHECK("pixel_xent_bilinear");
  return DL3_OK;
}

extern "C" int dl3_pixel_xent_shuffle(const float *u, const float *labels, const float *weights, float *v, int N, int H,
                                      int W, int C, int r, void *stream) {
  DL3_CHECK_ARG(u && labels && v && N > 0 && H > 0 && W > 0 && C > 0 && r > 0, "pixel_xent_shuffle: bad argument");
  DL3_UNSUPPORTED(C > kHeadMaxC, "pixel_xent_shuffle: C=%d > 32 (use phase_shift + pixel_xent_plain)", C);
  const int pb = shuffle_pb(W, C, r);
  DL3_UNSUPPORTED(pb < 1, "pixel_xent_shuffle: a pixel of %d x %d x %d floats does not fit the LDS tile", C, r, r);
  DL3_CHECK_ARG((long)N * H * r * W * r <= 0x7fffffffL, "pixel_xent_shuffle: more than 2^31 - 1 pixels");
  const size_t lds = (size_t)pb * C * (r * r + 1) * 4;
  dim3 grid(H * dl3_cdiv(W, pb), N);
#define DL3_PIX_SHF(MAXC)                                                                                          \
  hipLaunchKernelGGL((pixel_shuffle_kernel<MAXC>), grid, dim3(256), lds, (hipStream_t)stream, u, labels, weights, v, H, \
                     W, C, r, pb)
  DL3_DISPATCH_MAXC(C, DL3_PIX_SHF);
#undef DL3_PIX_SHF
  DL3_LAUNCH_CHECK("pixel_xent_shuffle");
  return DL3_OK;
}

extern "C" size_t dl3_topk_workspace_bytes(int N) { return N > 0 ? (size_t)kWsWords * 4 : 0; }

extern "C" int dl3_topk_threshold(const float *v, int N, float p, int S, const unsigned long long *step, void *ws,
                                  size_t ws_bytes, int *k, float *tau, void *stream) {
  DL3_CHECK_ARG(v && ws && k && tau && N > 0, "topk_threshold: bad argument");
  DL3_CHECK_ARG(p > 0.f && p <= 1.f && S >= 0, "topk_threshold: p must be in (0, 1] and S >= 0, got %g, %d", (double)p, S);
  DL3_CHECK_ARG(ws_bytes >= dl3_topk_workspace_bytes(N), "topk_threshold: workspace of %zu bytes, %zu needed", ws_bytes,
                dl3_topk_workspace_bytes(N));
  hipStream_t st = (hipStream_t)stream;
  unsigned int *w = (unsigned int *)ws;
  // one workgroup of 1024 threads per CU or two: few workgroups keep the global atomics per pass low (bins x workgroups)
  dim3 hgrid(dl3_blocks(N, kHistThreads * 8, 512));
  hipLaunchKernelGGL(mine_zero_kernel, dim3(dl3_cdiv(kWsWords, 256)), dim3(256), 0, st, w);
  hipLaunchKernelGGL(mine_hist_kernel<0>, hgrid, dim3(kHistThreads), 0, st, v, (long)N, w);
  hipLaunchKernelGGL(mine_pick_kernel<0>, dim3(1), dim3(256), 0, st, w, p, S, step, (long)N, k, tau);
  hipLaunchKernelGGL(mine_hist_kernel<1>, hgrid, dim3(kHistThreads), 0, st, v, (long)N, w);
  hipLaunchKernelGGL(mine_pick_kernel<1>, dim3(1), dim3(256), 0, st, w, p, S, step, (long)N, k, tau);
  hipLaunchKernelGGL(mine_hist_kernel<2>, hgrid, dim3(kHistThreads), 0, st, v, (long)N, w);
  hipLaunchKernelGGL(mine_pick_kernel<2>, dim3(1), dim3(256), 0, st, w, p, S, step, (long)N, k, tau);
  DL3_LAUNCH_CHECK("topk_threshold");
  return DL3_OK;
}

extern "C" int dl3_mine_weights(const float *v, const float *weights, const float *tau, const int *k, float *w_out,
                                float *nnz_out, void *ws, int N, void *stream) {
  DL3_CHECK_ARG(v && tau && k && w_out && nnz_out && ws && N > 0, "mine_weights: bad argument");
  hipStream_t st = (hipStream_t)stream;
  unsigned int *w = (unsigned int *)ws;
  hipLaunchKernelGGL(mine_weights_kernel, dim3(dl3_blocks(N, 256 * 8, 2048)), dim3(256), 0, st, v, weights, tau, k,
                     w_out, w, (long)N);
  hipLaunchKernelGGL(mine_count_kernel, dim3(1), dim3(1), 0, st, w, nnz_out);
  DL3_LAUNCH_CHECK("mine_weights");
  return DL3_OK;
}
