// trimap.hip — the trimap experiment of the DeepLabV3+ paper on the device: a clamped distance transform
// on the label maps and a confusion histogram per boundary band.
//   ring[b][y][x] = the smallest integer w >= 0 such that a seed of image b lies within distance w of (y, x), clamped to
//                   wmax + 1 ("beyond").  Seeds: void pixels and / or pixels with a 4-neighbour of another label value.
//   band[bin][t][p] += 1 for a legal label t and a prediction p in 0..C-1, bin = the first k with ring <= widths[k], else K.
// The distance is separable:
//   pass A  trimap_rows_kernel   h[b][y][x] = horizontal distance to the nearest seed of the row, clamped, one byte a pixel.
//           A wave ballots the seed bits of 64 pixels into one 64-bit word; a workgroup holds the words of its 256 pixels and
//           of ceil(wmax / 64) words on either side in LDS, and a lane finds its two distances with ffs / clz on two 64-bit
//           windows cut out of them — no serial scan.
//   pass B  trimap_cols_kernel   ring = min over |dy| <= wmax of combine(|dy|, h[y + dy][x]); combine = max (Chebyshev) or
//           dy^2 + h^2 (Euclidean, ring = ceil(sqrt) decided in integers).  The clamp is exact: a seed within distance wmax
//           has |dx| <= wmax.  A lane owns 4 neighbouring pixels of kRows rows: one dword of h per source row, a wave reads
//           256 contiguous bytes.
// The workspace rows have a pitch of W rounded up to 4 bytes, so every dword of h is aligned whatever W is; the pad bytes
// hold "beyond".  Only integer arithmetic and integer atomics: two runs are bit-identical.
#include "common.h"

namespace {

constexpr int kMaxWidth = 254;     // ring values fit a byte with wmax + 1 = "beyond"
constexpr int kMaxBands = 8;
constexpr int kMaxClasses = 255;
constexpr int kLdsClasses = 32;    // the banded histogram lives in LDS up to here: 9 * 32 * 32 ints = 36 KB
constexpr int kChunk = 256;        // pixels of a row per workgroup item (pass A)
constexpr int kMaxHalo = 4;        // ceil(254 / 64) words on either side
constexpr int kRows = 4;           // output rows per lane (pass B)
constexpr int kFar = 1 << 30;      // "no seed seen" (above every distance, squared or not)

// a label value as the seed rule compares it: 0..C-1, everything else is void = C
__device__ __forceinline__ int label_value(float f, int C) {
  const int t = (int)f;
  return (t >= 0 && t < C) ? t : C;
}

// ---------------------------------------------------------------------------------------------------------------------
// pass A.  item = (image, row, chunk of 256 pixels); grid-stride over the items.  words[1 + j] holds the seed bits of the
// pixels x0 + (j - halo) * 64 .. + 63 (bits of pixels outside the row are 0); words[0] and the word behind the last one
// stay 0, so that the window arithmetic below never indexes outside the array.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trimap_rows_kernel(const float *__restrict__ labels, unsigned char *__restrict__ h,
                                                          int B, int H, int W, int Wp, int C, int wmax, int seeds,
                                                          int chunks, int items) {
  __shared__ unsigned long long words[4 + 2 * kMaxHalo + 2];
  const int halo = (wmax + 63) >> 6;
  const int nwords = 4 + 2 * halo;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int far = wmax + 1;
  if (threadIdx.x < 4 + 2 * kMaxHalo + 2) words[threadIdx.x] = 0ull;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int chunk = item % chunks;
    const int row = item / chunks;          // b * H + y
    const int y = row % H;
    const int x0 = chunk * kChunk;
    const float *lrow = labels + (size_t)row * W;
    __syncthreads();   // the previous item's words have been read (and the zero fill is done)
    for (int j = wave; j < nwords; j += 4) {
      const int x = x0 + (j - halo) * 64 + lane;
      const bool in = (x >= 0 && x < W);
      bool seed = false;
      int v = C;
      if (in) v = label_value(lrow[x], C);
      // the horizontal neighbours from the neighbouring lanes; lanes 0 and 63 load theirs
      int vl = __shfl_up(v, 1, 64), vr = __shfl_down(v, 1, 64);
      if (in) {
        if (seeds & DL3_TRIMAP_SEED_VOID) seed = (v == C);
        if (seeds & DL3_TRIMAP_SEED_EDGES) {
          if (lane == 0 && x > 0) vl = label_value(lrow[x - 1], C);
          if (lane == 63 && x < W - 1) vr = label_value(lrow[x + 1], C);
          if (x > 0) seed |= (vl != v);
          if (x < W - 1) seed |= (vr != v);
          if (y > 0) seed |= (label_value(lrow[x - W], C) != v);
          if (y < H - 1) seed |= (label_value(lrow[x + W], C) != v);
        }
      }
      const unsigned long long bits = __ballot(seed);
      if (lane == 0) words[1 + j] = bits;
    }
    __syncthreads();
    // the lane's pixel is bit p of the word array proper (words + 1)
    const int x = x0 + threadIdx.x;
    const int p = halo * 64 + threadIdx.x;
    const int wi = 1 + (p >> 6), sh = p & 63;
    int d = far;
    // to the right (the pixel itself included): windows of 64 bits that start at p, p + 64, ...
    for (int k = 0; k <= halo; k++) {
      unsigned long long win = words[wi + k] >> sh;
      if (sh) win |= words[wi + k + 1] << (64 - sh);
      if (win) { d = min(d, 64 * k + (int)__builtin_ctzll(win)); break; }
    }
    // to the left: windows of 64 bits that end at p, p - 64, ...
    for (int k = 0; k <= halo; k++) {
      unsigned long long win = words[wi - k] << (63 - sh);
      if (sh != 63) win |= words[wi - k - 1] >> (sh + 1);
      if (win) { d = min(d, 64 * k + (int)__builtin_clzll(win)); break; }
    }
    if (x >= W) d = far;   // the pad bytes of the pitch
    // four lanes' bytes in one dword store (x0 and the pitch are multiples of 4)
    unsigned int pack = (unsigned int)d;
    pack |= (unsigned int)__shfl_down(d, 1, 64) << 8;
    pack |= (unsigned int)__shfl_down(d, 2, 64) << 16;
    pack |= (unsigned int)__shfl_down(d, 3, 64) << 24;
    if ((lane & 3) == 0 && x < Wp) *reinterpret_cast<unsigned int *>(h + (size_t)row * Wp + x) = pack;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pass B.  item = (image, band of kRows rows, group of 4 pixels); consecutive lanes take consecutive groups.  acc holds the
// running minimum: a distance (Chebyshev) or a squared distance (Euclidean).
// ---------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void trimap_cols_kernel(const unsigned char *__restrict__ h, unsigned char *__restrict__ rings,
                                                          int H, int W, int Wp, int wmax, int bands, long long items) {
  const int G = Wp >> 2;
  const int far = wmax + 1;
  const unsigned int far4 = (unsigned int)far * 0x01010101u;
  for (long long item = (long long)blockIdx.x * 256 + threadIdx.x; item < items; item += (long long)gridDim.x * 256) {
    const int g = (int)(item % G);
    const long long rb = item / G;
    const int band = (int)(rb % bands), b = (int)(rb / bands);
    const int y0 = band * kRows;
    const int s0 = max(y0 - wmax, 0), s1 = min(y0 + kRows - 1 + wmax, H - 1);
    const unsigned char *hb = h + (size_t)b * H * Wp + (size_t)g * 4;
    int acc[kRows][4];
#pragma unroll
    for (int r = 0; r < kRows; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) acc[r][k] = kFar;
    for (int s = s0; s <= s1; s++) {
      const unsigned int q = *reinterpret_cast<const unsigned int *>(hb + (size_t)s * Wp);
      if (q == far4) continue;   // no seed near any of the four pixels in this row
#pragma unroll
      for (int r = 0; r < kRows; r++) {
        const int dy = abs(s - (y0 + r));
        if (dy > wmax) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int hx = (int)((q >> (8 * k)) & 255u);
          int c;
          if (METRIC == DL3_TRIMAP_CHEBYSHEV) c = max(dy, hx);
          else c = (hx > wmax) ? kFar : dy * dy + hx * hx;
          acc[r][k] = min(acc[r][k], c);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRows; r++) {
      const int y = y0 + r;
      if (y >= H) break;
      unsigned int out[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        int v = acc[r][k];
        if (METRIC == DL3_TRIMAP_EUCLIDEAN) {
          if (v > wmax * wmax) v = far;
          else {
            // the smallest r with r^2 >= v (v <= 254^2: the float root is within one of it)
            int t = (int)sqrtf((float)v);
            while (t * t < v) t++;
            while (t > 0 && (t - 1) * (t - 1) >= v) t--;
            v = t;
          }
        }
        out[k] = (unsigned int)min(v, far);
      }
      unsigned char *o = rings + ((size_t)b * H + y) * W + (size_t)g * 4;
      if (g * 4 + 3 < W && ((uintptr_t)o & 3) == 0) {
        *reinterpret_cast<unsigned int *>(o) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (g * 4 + k < W) o[k] = (unsigned char)out[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the banded confusion histogram.  Per workgroup an LDS histogram [K + 1][C][C] of ints (C <= 32), then one global 64-bit
// integer atomic per non-zero bin; above 32 classes straight global integer atomics, as the evaluation tail's plain form.
// VEC: a lane takes 4 neighbouring pixels (16 + 16 + 4 bytes); the host picks it when all three pointers allow it.
// ---------------------------------------------------------------------------------------------------------------------
struct Widths {
  int w[kMaxBands];
};

template <bool VEC, bool LDS>
__global__ __launch_bounds__(256) void trimap_confusion_kernel(const int *__restrict__ pred, const float *__restrict__ labels,
                                                               const unsigned char *__restrict__ rings,
                                                               long long *__restrict__ band, int n, int C, Widths widths,
                                                               int K) {
  extern __shared__ __attribute__((aligned(16))) int hist[];   // LDS form: [(K + 1) * C * C]
  __shared__ unsigned char bin_of[256];
  {
    int k = 0;
    while (k < K && (int)threadIdx.x > widths.w[k]) k++;
    bin_of[threadIdx.x] = (unsigned char)k;
  }
  const int nh = (K + 1) * C * C;
  if (LDS)
    for (int i = threadIdx.x; i < nh; i += 256) hist[i] = 0;
  __syncthreads();
  unsigned long long *gband = reinterpret_cast<unsigned long long *>(band);
  auto count = [&](int p, float lf, unsigned int ring) {
    const int t = (int)lf;
    if (t >= 0 && t < C && p >= 0 && p < C) {
      const int i = ((int)bin_of[ring] * C + t) * C + p;
      if (LDS) atomicAdd(&hist[i], 1);
      else atomicAdd(gband + i, 1ull);
    }
  };
  if (VEC) {
    const int n4 = n >> 2;
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
      const int4 p = *reinterpret_cast<const int4 *>(pred + (size_t)i * 4);
      const f32x4 l = ld4(labels + (size_t)i * 4);
      const unsigned int r = *reinterpret_cast<const unsigned int *>(rings + (size_t)i * 4);
      count(p.x, l.x, r & 255u);
      count(p.y, l.y, (r >> 8) & 255u);
      count(p.z, l.z, (r >> 16) & 255u);
      count(p.w, l.w, r >> 24);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (n & 3)) {
      const int i = (n4 << 2) + threadIdx.x;
      count(pred[i], labels[i], rings[i]);
    }
  } else {
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) count(pred[i], labels[i], rings[i]);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += 256)
      if (hist[i]) atomicAdd(gband + i, (unsigned long long)hist[i]);
  }
}

inline bool sizes_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1ll << 31);
}

}  // namespace

extern "C" size_t dl3_trimap_workspace_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W)) return 0;
  return (size_t)B * H * (((size_t)W + 3) & ~(size_t)3);
}

extern "C" int dl3_trimap_rings(const float *labels, unsigned char *rings, void *workspace, int B, int H, int W, int C,
                                int wmax, int metric, int seeds, void *stream) {
  DL3_CHECK_ARG(labels && rings && workspace, "trimap_rings: null pointer");
  DL3_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "trimap_rings: the workspace must be 4-byte aligned");
  DL3_CHECK_ARG(sizes_ok(B, H, W), "trimap_rings: B, H, W must be positive with B*H*W < 2^31, got %d x %d x %d", B, H, W);
  DL3_CHECK_ARG(C >= 1 && C <= kMaxClasses, "trimap_rings: classes must be in 1..%d, got %d", kMaxClasses, C);
  DL3_CHECK_ARG(wmax >= 1 && wmax <= kMaxWidth, "trimap_rings: wmax must be in 1..%d, got %d", kMaxWidth, wmax);
  DL3_CHECK_ARG(metric == DL3_TRIMAP_CHEBYSHEV || metric == DL3_TRIMAP_EUCLIDEAN, "trimap_rings: unknown metric %d", metric);
  DL3_CHECK_ARG(seeds >= 1 && seeds <= 3, "trimap_rings: the seed mask must be in 1..3, got %d", seeds);
  hipStream_t st = (hipStream_t)stream;
  const int Wp = (W + 3) & ~3;
  unsigned char *h = static_cast<unsigned char *>(workspace);
  const int chunks = dl3_cdiv(W, kChunk);
  const long long items_a = (long long)B * H * chunks;   // <= B*H*W < 2^31
  hipLaunchKernelGGL(trimap_rows_kernel, dim3(dl3_blocks((long)items_a, 1, 65536)), dim3(256), 0, st, labels, h, B, H, W, Wp,
                     C, wmax, seeds, chunks, (int)items_a);
  const int bands = dl3_cdiv(H, kRows);
  const long long items_b = (long long)B * bands * (Wp >> 2);
  const dim3 grid(dl3_blocks((long)items_b, 256, 8192));
  if (metric == DL3_TRIMAP_CHEBYSHEV)
    hipLaunchKernelGGL((trimap_cols_kernel<DL3_TRIMAP_CHEBYSHEV>), grid, dim3(256), 0, st, h, rings, H, W, Wp, wmax, bands,
                       items_b);
  else
    hipLaunchKernelGGL((trimap_cols_kernel<DL3_TRIMAP_EUCLIDEAN>), grid, dim3(256), 0, st, h, rings, H, W, Wp, wmax, bands,
                       items_b);
  DL3_LAUNCH_CHECK("trimap_rings");
  return DL3_OK;
}

extern "C" int dl3_trimap_confusion(const int *pred, const float *labels, const unsigned char *rings, long long *band, int B,
                                    int H, int W, int C, const int *widths, int K, void *stream) {
  DL3_CHECK_ARG(pred && labels && rings && band && widths, "trimap_confusion: null pointer");
  DL3_CHECK_ARG(sizes_ok(B, H, W), "trimap_confusion: B, H, W must be positive with B*H*W < 2^31, got %d x %d x %d", B, H, W);
  DL3_CHECK_ARG(C >= 1 && C <= kMaxClasses, "trimap_confusion: classes must be in 1..%d, got %d", kMaxClasses, C);
  DL3_CHECK_ARG(K >= 1 && K <= kMaxBands, "trimap_confusion: 1 to %d widths, got %d", kMaxBands, K);
  Widths wd;
  for (int k = 0; k < kMaxBands; k++) wd.w[k] = 0;
  for (int k = 0; k < K; k++) {
    DL3_CHECK_ARG(widths[k] >= 1 && widths[k] <= kMaxWidth && (k == 0 || widths[k] > widths[k - 1]),
                  "trimap_confusion: widths must be strictly increasing in 1..%d, got %d at %d", kMaxWidth, widths[k], k);
    wd.w[k] = widths[k];
  }
  hipStream_t st = (hipStream_t)stream;
  const int n = B * H * W;
  const bool vec = aligned16(pred) && aligned16(labels) && ((uintptr_t)rings & 3) == 0;
  const bool lds = C <= kLdsClasses;
  const size_t smem = lds ? (size_t)(K + 1) * C * C * sizeof(int) : 0;
  const dim3 grid(dl3_blocks(n, 256 * 16, 512));
#define DL3_TRIMAP_CONF(VEC, LDS)                                                                                       \
  hipLaunchKernelGGL((trimap_confusion_kernel<VEC, LDS>), grid, dim3(256), smem, st, pred, labels, rings, band, n, C, wd, K)
  if (vec && lds) DL3_TRIMAP_CONF(true, true);
  else if (vec) DL3_TRIMAP_CONF(true, false);
  else if (lds) DL3_TRIMAP_CONF(false, true);
  else DL3_TRIMAP_CONF(false, false);
#undef DL3_TRIMAP_CONF
  DL3_LAUNCH_CHECK("trimap_confusion");
  return DL3_OK;
}
