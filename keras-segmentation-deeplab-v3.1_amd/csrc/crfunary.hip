// crfunary.hip — the dense CRF's unary energies from the network's own class scores ("softmax unary"):
// pydensecrf.utils.unary_from_softmax [pydensecrf-semantics] on the device, U = -log(clip(scale p + (1 - scale) / C)),
// written as the planar U[B][C][N] that dl3_crf_inference reads.  Three input forms, the ones of evaltail.hip:
//   plain     x [B][N][C]            materialised logits, or probabilities (is_prob)
//   bilinear  logits_lo [B][Hi][Wi][C] -> the TF1 legacy bilinear resize in registers, bit-identical to
//             dl3_resize_bilinear_fwd (tailmath.h: the fused weight .w)
//   shuffle   u [B][H][W][C*r*r]     -> Subpixel._phase_shift by index
// One kernel: a workgroup owns 256 consecutive pixels of one image, a lane one pixel with its C <= 32 scores in
// registers.  Consecutive lanes own consecutive pixels, so class c of a wave is one 256-byte run of plane c; where N is a
// multiple of four the workgroup's [C][256] tile is turned in LDS and leaves as 16-byte stores.  The per-pixel row of C
// floats is never written.  Nothing is accumulated across lanes: two runs are bit-identical.
//
// Arithmetic: subtract-max, expf and the sum in fp32; the quotient, scale, clip and the logarithm in double, rounded to
// fp32 once (the form the accuracy test of tests/test_gpu_crf_unary.py asks for: see DESIGN.md §9).  -log, clip and
// scale are monotone, so the arg-min of U is the first-maximum argmax of the scores unless the clip ties them.
#include "tailmath.h"

namespace {

// (kHeadMaxC classes at most: dl3_crf_inference's label limit too)
constexpr int kPix = 256;    // pixels per workgroup

enum { kPlain = 0, kBilinear = 1, kShuffle = 2 };

struct Geom {
  int a, b, c, d;     // bilinear: Hi, Wi, Ho, Wo; shuffle: H, W, r, -
  float sy, sx;       // bilinear: Hi / Ho, Wi / Wo
};

// scores of one pixel -> its unary energies, in place
template <int MAXC>
__device__ __forceinline__ void unary_pixel(float (&z)[MAXC], int C, int is_prob, float scale, double unif, float clip) {
  double inv = 1.0;
  if (!is_prob) {
    inv = 1.0 / (double)softmax_exp<MAXC, float>(z, C);
  }
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    if (c < C) {
      double p = (double)z[c] * inv;
      if (scale > 0.f) p = fma((double)scale, p, unif);
      if (clip > 0.f) p = fmin(fmax(p, (double)clip), 1.0);
      z[c] = (float)(-log(p));
    }
  }
}

template <int MAXC, int FORM>
__global__ __launch_bounds__(kPix) void crf_unary_kernel(const float *__restrict__ x, float *__restrict__ U, int N, int C,
                                                         Geom g, int is_prob, float scale, double unif, float clip,
                                                         int vec_in, int vec_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // plain: [256][C | 1] in, then [C][256] out
  const int tid = threadIdx.x, b = blockIdx.y;
  const int i0 = blockIdx.x * kPix;
  const int npix = min(kPix, N - i0);
  const int i = i0 + min(tid, npix - 1);   // lanes past the image recompute its last pixel and store nothing
  float z[MAXC];
  if constexpr (FORM == kPlain) {
    // the workgroup's rows are npix * C contiguous floats: read coalesced, laid out with an odd row stride so that the
    // per-lane row reads touch distinct banks
    const int CP = C | 1;
    const float *src = x + ((size_t)b * N + i0) * C;
    if (vec_in) {
      for (int t = tid; t < npix * C / 4; t += kPix) {
        const f32x4 v = ld4(src + 4 * t);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int e = 4 * t + k, px = e / C;
          smem[px * CP + (e - px * C)] = v[k];
        }
      }
    } else {
      for (int t = tid; t < npix * C; t += kPix) {
        const int px = t / C;
        smem[px * CP + (t - px * C)] = src[t];
      }
    }
    __syncthreads();
    const float *row = smem + min(tid, npix - 1) * CP;
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = row[min(c, C - 1)];
    __syncthreads();   // the tile is reused for the output
  } else if constexpr (FORM == kBilinear) {
    const int Hi = g.a, Wi = g.b, Wo = g.d;
    const int oy = i / Wo, ox = i - oy * Wo;
    const BilinearTaps taps(x + (size_t)b * Hi * Wi * C, oy, ox, g.sy, g.sx, Hi, Wi, C);
    taps.load<MAXC>(z, C, taps.lx.w, taps.ly.w);   // dl3_resize_bilinear_fwd's weight
  } else {
    // out[n, ia*r+q, ib*r+p, ch] = u[n, ia, ib, ch*r*r + p*r + q]  (dl3_phase_shift)
    const int H = g.a, W = g.b, r = g.c, rr = r * r;
    const int Wr = W * r;
    const int Y = i / Wr, X = i - Y * Wr;
    const int ia = Y / r, q = Y - ia * r, ib = X / r, p = X - ib * r;
    const float *up = x + (((size_t)b * H + ia) * W + ib) * ((size_t)C * rr) + p * r + q;
#pragma unroll
    for (int c = 0; c < MAXC; c++) z[c] = up[(size_t)min(c, C - 1) * rr];
  }

  unary_pixel<MAXC>(z, C, FORM == kPlain ? is_prob : 0, scale, unif, clip);

  float *Ub = U + (size_t)b * C * N;
  if (!vec_out) {
    if (tid < npix) {
#pragma unroll
      for (int c = 0; c < MAXC; c++)
        if (c < C) Ub[(size_t)c * N + i] = z[c];
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < MAXC; c++)
    if (c < C) smem[c * kPix + tid] = z[c];
  __syncthreads();
  // N % 4 == 0: a group of four pixels is inside the image or outside it as a whole
  for (int t = tid; t < C * (kPix / 4); t += kPix) {
    const int c = t / (kPix / 4), j = (t - c * (kPix / 4)) * 4;
    if (j < npix) st4(Ub + (size_t)c * N + i0 + j, ld4(smem + c * kPix + j));
  }
}

template <int FORM>
int launch(const char *who, const float *x, float *U, int B, int N, int C, Geom g, int is_prob, float scale, float clip,
           void *stream) {
  DL3_CHECK_ARG(x && U, "%s: null pointer", who);
  DL3_CHECK_ARG(B > 0 && N > 0 && C > 0, "%s: B, N, C must be positive, got %d, %d, %d", who, B, N, C);
  DL3_UNSUPPORTED(C > kHeadMaxC, "%s: at most %d classes, got %d", who, kHeadMaxC, C);
  // every index of the kernel fits an int, the batch fits grid.y
  DL3_CHECK_ARG(N <= (1 << 25) && B <= 65535, "%s: B = %d, N = %d is too large", who, B, N);
  DL3_CHECK_ARG(scale <= 1.f && clip < 1.f, "%s: scale must be <= 1 and clip < 1, got %g, %g", who, (double)scale,
                (double)clip);
  const double unif = scale > 0.f ? (1.0 - (double)scale) / C : 0.0;
  const int vec_out = (N % 4 == 0) && aligned16(U);
  const int vec_in = FORM == kPlain && ((long long)N * C) % 4 == 0 && aligned16(x);
  const int CP = C | 1;
  const size_t lds = (size_t)kPix * (FORM == kPlain ? CP : (vec_out ? C : 0)) * sizeof(float);
  const dim3 grid(dl3_cdiv(N, kPix), B), block(kPix);
  hipStream_t st = (hipStream_t)stream;
#define DL3_UNARY(MAXC)                                                                                              \
  hipLaunchKernelGGL((crf_unary_kernel<MAXC, FORM>), grid, block, lds, st, x, U, N, C, g, is_prob, scale, unif, clip, \
                     vec_in, vec_out)
  DL3_DISPATCH_MAXC(C, DL3_UNARY);
#undef DL3_UNARY
  DL3_LAUNCH_CHECK(who);
  return DL3_OK;
}

}  // namespace

extern "C" int dl3_crf_unary_plain(const float *x, int is_prob, float *U, int B, int N, int C, float scale, float clip,
                                   void *stream) {
  DL3_CHECK_ARG(is_prob == 0 || is_prob == 1, "crf_unary_plain: is_prob must be 0 or 1, got %d", is_prob);
  const Geom g = {0, 0, 0, 0, 0.f, 0.f};
  return launch<kPlain>("crf_unary_plain", x, U, B, N, C, g, is_prob, scale, clip, stream);
}

extern "C" int dl3_crf_unary_bilinear(const float *logits_lo, float *U, int B, int Hi, int Wi, int Ho, int Wo, int C,
                                      float scale, float clip, void *stream) {
  DL3_CHECK_ARG(Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "crf_unary_bilinear: sizes must be positive, got %dx%d -> %dx%d", Hi,
                Wi, Ho, Wo);
  DL3_CHECK_ARG((long long)Ho * Wo <= (1 << 25) && (long long)Hi * Wi <= (1 << 25),
                "crf_unary_bilinear: %dx%d -> %dx%d is too large", Hi, Wi, Ho, Wo);
  const Geom g = {Hi, Wi, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo};
  return launch<kBilinear>("crf_unary_bilinear", logits_lo, U, B, Ho * Wo, C, g, 0, scale, clip, stream);
}

extern "C" int dl3_crf_unary_shuffle(const float *u, float *U, int B, int H, int W, int C, int r, float scale, float clip,
                                     void *stream) {
  DL3_CHECK_ARG(H > 0 && W > 0 && r > 0, "crf_unary_shuffle: H, W, r must be positive, got %d, %d, %d", H, W, r);
  DL3_CHECK_ARG((long long)H * r * W * r <= (1 << 25), "crf_unary_shuffle: %dx%d x %d is too large", H, W, r);
  const Geom g = {H, W, r, 0, 0.f, 0.f};
  return launch<kShuffle>("crf_unary_shuffle", u, U, B, H * r * W * r, C, g, 0, scale, clip, stream);
}
