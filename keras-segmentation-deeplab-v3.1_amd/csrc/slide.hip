// slide.hip — sliding-window inference: the three element-wise passes around the forward plan.
//   dl3_slide_gather      windows k0 .. k0+nw-1 of ONE image [Hi][Wi][3] (float32 or uint8) -> float32 [nw][H][W][3]
//   dl3_slide_accumulate  their probabilities [nw][H][W][C], weighted, folded into the image's canvas acc[Hi][Wi][C]
//   dl3_slide_finalize    canvas / weight sum -> probabilities and / or the first-maximum arg-max at image size
// The window grid is arithmetic (include/dl3.h): per axis n = ceil((max(size, win) - win) / stride) + 1 windows, window k
// at min(k stride, max(size, win) - win), so no launch needs a table.  Every operation is a separately rounded fp32
// operation in one order — per canvas element, over its covering windows in ascending k: t = w p; acc = acc + t — and
// this file switches contraction OFF (`#pragma clang fp contract(off)`), as tta.hip does and for its reason.
//
// dl3_slide_accumulate is an HBM stream over the canvas rows the launch's windows touch.  The windows of a launch are
// consecutive in k, so they lie in grid rows ky_first .. ky_last: the launch walks canvas rows origin(ky_first) ..
// origin(ky_last) + H - 1 and of each the columns [X0, X1) — the span of its windows where they share one grid row, the
// whole row otherwise.  A workgroup owns one canvas row's 256 * C consecutive floats of that span, cut on 16-byte
// boundaries of the ADDRESS (the up to three floats in front of the row span's first boundary and behind its last one are
// scalars of the row's first / last workgroup).  One lane per pixel first writes the pixel's window range on the x axis
// into LDS (empty where no window OF THIS LAUNCH covers the pixel: such elements are neither read nor written); a lane
// then owns four consecutive floats and folds EVERY covering window of the launch into them itself, in ascending k: an
// element is touched by one lane only, there are no atomics, and the order of its adds does not depend on how the
// window sequence was cut into launches.  Canvas traffic is 16-byte loads and stores wherever all four floats are
// covered; window probabilities are 4-byte loads (consecutive lanes read consecutive floats of the same window row).
#include <algorithm>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 256;          // canvas pixels (rows of C floats) per workgroup
constexpr int kPixLds = kPix + 8;  // + the partial pixels at either end of a run that starts / ends inside a pixel

typedef f32x4 f32x4_a4 __attribute__((aligned(4)));   // a 16-byte load at 4-byte alignment

struct Axis {
  int n, win, stride, last;   // windows, window extent, stride, origin of the last window = max(size, win) - win
};
inline Axis make_axis(int size, int win, int stride) {
  const int last = std::max(size, win) - win;
  Axis a = {(last + stride - 1) / stride + 1, win, stride, last};
  return a;
}
__host__ __device__ __forceinline__ int ax_origin(const Axis &a, int k) {
  const int o = k * a.stride;   // < last + stride
  return o < a.last ? o : a.last;
}
// the windows covering coordinate p are ax_lo(p) .. ax_hi(p): origins grow with k
__device__ __forceinline__ int ax_lo(const Axis &a, int p) {
  const int k = p < a.win ? 0 : (p - a.win) / a.stride + 1;
  return min(k, a.n - 1);
}
__device__ __forceinline__ int ax_hi(const Axis &a, int p) { return p >= a.last ? a.n - 1 : p / a.stride; }
__device__ __forceinline__ float ax_weight(const Axis &a, int r, int blend) {
  return blend == DL3_SLIDE_PYRAMID ? (float)min(r + 1, a.win - r) : 1.f;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void slide_gather_kernel(const T *__restrict__ src, float *__restrict__ dst, Axis ay,
                                                                Axis ax, int Hi, int Wi, int k0, long long total,
                                                                float pad_value) {
  const int HW = ay.win * ax.win;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kThreads) {
    const int j = (int)(g / HW);
    const int rc = (int)(g - (long long)j * HW);
    const int r = rc / ax.win, c = rc - r * ax.win;
    const int k = k0 + j, ky = k / ax.n, kx = k - ky * ax.n;
    const int y = ax_origin(ay, ky) + r, x = ax_origin(ax, kx) + c;
    float *d = dst + (size_t)g * 3;
    if (y < Hi && x < Wi) {
      const T *s = src + ((size_t)y * Wi + x) * 3;
#pragma unroll
      for (int i = 0; i < 3; i++) d[i] = (float)s[i];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) d[i] = pad_value;
    }
  }
}

struct Geom {
  Axis ay, ax;
  int Hi, Wi, C, blend;
  int k0, k1;      // the launch's windows (finalize: the whole grid)
  int ya, X0, R;   // first canvas row, first column and columns per row of the launch
};

__device__ __forceinline__ bool in_launch(const Geom &g, int kylo, int kyhi, int kxlo, int kxhi) {
  bool any = false;
  for (int ky = kylo; ky <= kyhi; ky++)
    for (int kx = kxlo; kx <= kxhi; kx++) {
      const int k = ky * g.ax.n + kx;
      any |= k >= g.k0 && k < g.k1;
    }
  return any;
}

// ws + the weights of the windows k0 <= k < k1 that cover pixel (y, x), in ascending k
__device__ __forceinline__ float fold_weights(const Geom &g, int y, int x, int kylo, int kyhi, int kxlo, int kxhi, float ws) {
  for (int ky = kylo; ky <= kyhi; ky++) {
    const float wy = ax_weight(g.ay, y - ax_origin(g.ay, ky), g.blend);
    for (int kx = kxlo; kx <= kxhi; kx++) {
      const int k = ky * g.ax.n + kx;
      if (k < g.k0 || k >= g.k1) continue;
      const float w = wy * ax_weight(g.ax, x - ax_origin(g.ax, kx), g.blend);
      ws = ws + w;
    }
  }
  return ws;
}

// v + the weighted probabilities of channel ch of the launch's windows that cover pixel (y, x), in ascending k
__device__ __forceinline__ float fold_probs(const float *__restrict__ probs, const Geom &g, int y, int x, int ch, int kylo,
                                            int kyhi, int kxlo, int kxhi, float v) {
  for (int ky = kylo; ky <= kyhi; ky++) {
    const int r = y - ax_origin(g.ay, ky);
    const float wy = ax_weight(g.ay, r, g.blend);
    for (int kx = kxlo; kx <= kxhi; kx++) {
      const int k = ky * g.ax.n + kx;
      if (k < g.k0 || k >= g.k1) continue;
      const int c = x - ax_origin(g.ax, kx);
      const float w = wy * ax_weight(g.ax, c, g.blend);
      const int wp = ((k - g.k0) * g.ay.win + r) * g.ax.win + c;   // < nw * H * W < 2^31
      const float t = w * probs[(size_t)wp * g.C + ch];
      v = v + t;
    }
  }
  return v;
}

// one workgroup: canvas row ya + blockIdx.x / bpr, chunk blockIdx.x % bpr of its span
__global__ __launch_bounds__(kThreads) void slide_accumulate_kernel(const float *__restrict__ probs, float *__restrict__ acc,
                                                                    float *__restrict__ wsum, Geom g, int bpr) {
  __shared__ int plo[kPixLds], phi[kPixLds];   // the pixel's window range on the x axis; lo > hi: not in this launch
  const int tid = threadIdx.x, C = g.C;
  const int row = blockIdx.x / bpr, chunk = blockIdx.x - row * bpr;
  const int y = g.ya + row;
  const int kylo = ax_lo(g.ay, y), kyhi = ax_hi(g.ay, y);
  float *arow = acc + ((size_t)y * g.Wi + g.X0) * C;   // the row's span: L floats at any 4-byte alignment
  const int L = g.R * C;
  const int head = min((int)((4 - (((uintptr_t)arow >> 2) & 3)) & 3), L);
  const int nvec = (L - head) / 4;
  const int run4 = kPix * C / 4;
  const bool is_first = chunk == 0, is_last = chunk == bpr - 1;
  const int v_beg = min(chunk * run4, nvec);
  const int nv = min(run4, nvec - v_beg);
  const int e_beg = is_first ? 0 : head + 4 * v_beg;
  const int e_end = is_last ? L : head + 4 * (v_beg + nv);
  if (e_end <= e_beg) return;   // the whole workgroup
  const int p_beg = e_beg / C;
  const int npix = (e_end - 1) / C - p_beg + 1;   // <= kPix + 7
  for (int i = tid; i < npix; i += kThreads) {
    const int x = g.X0 + p_beg + i;
    int lo = ax_lo(g.ax, x), hi = ax_hi(g.ax, x);
    if (!in_launch(g, kylo, kyhi, lo, hi)) {
      lo = 1;
      hi = 0;
    } else if (wsum) {
      const int e0 = (p_beg + i) * C;   // the pixel belongs to the workgroup that owns its first float
      if (e0 >= e_beg && e0 < e_end) {
        float *w = wsum + (size_t)y * g.Wi + x;
        *w = fold_weights(g, y, x, kylo, kyhi, lo, hi, *w);
      }
    }
    plo[i] = lo;
    phi[i] = hi;
  }
  __syncthreads();

  for (int t = tid; t < nv; t += kThreads) {
    const int e = head + 4 * (v_beg + t);
    const int rel = e - p_beg * C;
    const int lp0 = rel / C, c0 = rel - lp0 * C;
    bool all = true, any = false;
    {
      int lp = lp0, c = c0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool cov = plo[lp] <= phi[lp];
        all &= cov;
        any |= cov;
        if (++c == C) {
          c = 0;
          lp++;
        }
      }
    }
    if (!any) continue;
    int lp = lp0, c = c0;
    if (all) {
      f32x4 v = ld4(arow + e);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        v[k] = fold_probs(probs, g, y, g.X0 + p_beg + lp, c, kylo, kyhi, plo[lp], phi[lp], v[k]);
        if (++c == C) {
          c = 0;
          lp++;
        }
      }
      st4(arow + e, v);
    } else {   // a group on the edge of the launch's windows: its covered floats one by one
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (plo[lp] <= phi[lp])
          arow[e + k] = fold_probs(probs, g, y, g.X0 + p_beg + lp, c, kylo, kyhi, plo[lp], phi[lp], arow[e + k]);
        if (++c == C) {
          c = 0;
          lp++;
        }
      }
    }
  }
  // scalars in front of the span's first boundary and behind its last group
  int e = -1;
  if (is_first && tid < head) e = tid;
  const int t_beg = head + 4 * nvec;
  if (is_last && tid >= 4 && tid - 4 < L - t_beg) e = t_beg + tid - 4;
  if (e >= 0) {
    const int px = e / C, lp = px - p_beg;
    if (plo[lp] <= phi[lp]) arow[e] = fold_probs(probs, g, y, g.X0 + px, e - px * C, kylo, kyhi, plo[lp], phi[lp], arow[e]);
  }
}

__device__ __forceinline__ float pixel_wsum(const float *__restrict__ wsum, const Geom &g, int gp) {
  if (wsum) return wsum[gp];
  const int y = gp / g.Wi, x = gp - y * g.Wi;
  return fold_weights(g, y, x, ax_lo(g.ay, y), ax_hi(g.ay, y), ax_lo(g.ax, x), ax_hi(g.ax, x), 0.f);
}

// mask = first maximum of acc / ws; runs in front of the probabilities kernel, which may overwrite acc
__global__ __launch_bounds__(kThreads) void slide_mask_kernel(const float *__restrict__ acc, const float *__restrict__ wsum,
                                                              int *__restrict__ mask, Geom g, int npixels) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < npixels; p += (long long)gridDim.x * kThreads) {
    const float ws = pixel_wsum(wsum, g, (int)p);
    const float *r = acc + (size_t)p * g.C;
    float mx = r[0] / ws;   // IEEE division: hipcc's default for fp32
    int am = 0;
    for (int c = 1; c < g.C; c++) {
      const float q = r[c] / ws;
      if (q > mx) {
        mx = q;
        am = c;
      }
    }
    mask[p] = am;
  }
}

// out = acc / ws over total = Hi * Wi * C floats, cut on the 16-byte boundaries of `out` (tta_accumulate_kernel's scheme);
// out may be acc itself: an element is read and written by one lane
__global__ __launch_bounds__(kThreads) void slide_probs_kernel(const float *acc, const float *__restrict__ wsum, float *out,
                                                               Geom g, long long total, int head, long long nvec) {
  __shared__ float pws[kPixLds];
  const int tid = threadIdx.x, C = g.C;
  const long long run = (long long)kPix * C;
  const bool is_first = blockIdx.x == 0, is_last = blockIdx.x == gridDim.x - 1;
  const long long e_beg = is_first ? 0 : head + (long long)blockIdx.x * run;
  const long long e_end = is_last ? total : head + ((long long)blockIdx.x + 1) * run;
  const long long p_beg = e_beg / C;
  const int npix = (int)((e_end - 1) / C - p_beg) + 1;   // <= kPix + 7
  for (int i = tid; i < npix; i += kThreads) pws[i] = pixel_wsum(wsum, g, (int)(p_beg + i));
  __syncthreads();

  const long long v_beg = (long long)blockIdx.x * (run / 4);
  const int nv = (int)min((long long)(run / 4), nvec - v_beg);
  for (int t = tid; t < nv; t += kThreads) {
    const long long e = head + 4 * (v_beg + t);
    const int rel = (int)(e - p_beg * C);
    int lp = rel / C, c = rel - lp * C;
    f32x4 v = *reinterpret_cast<const f32x4_a4 *>(acc + e);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] = v[k] / pws[lp];
      if (++c == C) {
        c = 0;
        lp++;
      }
    }
    st4(out + e, v);
  }
  if (is_first && tid < head) out[tid] = acc[tid] / pws[(int)(tid / C - p_beg)];
  const long long t_beg = head + 4 * nvec;
  if (is_last && tid < (int)(total - t_beg)) {
    const long long e = t_beg + tid;
    out[e] = acc[e] / pws[(int)(e / C - p_beg)];
  }
}

// the checks the three entry points share; fills the axes
int slide_axes(const char *who, int Hi, int Wi, int H, int W, int sh, int sw, Axis *ay, Axis *ax) {
  DL3_CHECK_ARG(Hi > 0 && Wi > 0 && H > 0 && W > 0, "%s: sizes must be positive, got image %dx%d, window %dx%d", who, Hi, Wi, H,
                W);
  DL3_CHECK_ARG(sh >= 1 && sh <= H && sw >= 1 && sw <= W, "%s: stride must be in [1, window], got (%d, %d) for window %dx%d", who,
                sh, sw, H, W);
  // every pixel index of the image and of a window fits an int
  DL3_CHECK_ARG((long long)Hi * Wi < (1ll << 31) && (long long)H * W < (1ll << 31), "%s: image %dx%d / window %dx%d is too large",
                who, Hi, Wi, H, W);
  *ay = make_axis(Hi, H, sh);
  *ax = make_axis(Wi, W, sw);
  DL3_CHECK_ARG((long long)ay->n * ax->n < (1ll << 31), "%s: %d x %d windows are too many", who, ay->n, ax->n);
  return DL3_OK;
}
int slide_windows(const char *who, const Axis &ay, const Axis &ax, int k0, int nw) {
  DL3_CHECK_ARG(nw >= 1, "%s: nw must be at least 1, got %d", who, nw);
  DL3_CHECK_ARG(k0 >= 0 && (long long)k0 + nw <= (long long)ay.n * ax.n, "%s: windows %d .. %lld are outside the grid of %d x %d", who,
                k0, (long long)k0 + nw - 1, ay.n, ax.n);
  DL3_CHECK_ARG((long long)nw * ay.win * ax.win < (1ll << 31), "%s: %d windows of %dx%d are too many for one launch", who, nw,
                ay.win, ax.win);
  return DL3_OK;
}
#define SLIDE_TRY(call)          \
  do {                           \
    const int rc__ = (call);     \
    if (rc__ != DL3_OK) return rc__; \
  } while (0)

}  // namespace

extern "C" int dl3_slide_gather(const void *src, int src_dtype, int Hi, int Wi, int H, int W, int sh, int sw, int k0, int nw,
                                float pad_value, float *dst, void *stream) {
  DL3_CHECK_ARG(src && dst, "slide_gather: null pointer");
  DL3_CHECK_ARG(src_dtype == DL3_TTA_F32 || src_dtype == DL3_TTA_U8, "slide_gather: src_dtype must be 0 (float32) or 1 (uint8), got %d",
                src_dtype);
  Axis ay, ax;
  SLIDE_TRY(slide_axes("slide_gather", Hi, Wi, H, W, sh, sw, &ay, &ax));
  SLIDE_TRY(slide_windows("slide_gather", ay, ax, k0, nw));
  const long long total = (long long)nw * H * W;
  const int grid = (int)std::min<long long>((total + kThreads - 1) / kThreads, 8192);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == DL3_TTA_U8)
    hipLaunchKernelGGL(slide_gather_kernel<unsigned char>, dim3(grid), dim3(kThreads), 0, st, (const unsigned char *)src, dst,
                       ay, ax, Hi, Wi, k0, total, pad_value);
  else
    hipLaunchKernelGGL(slide_gather_kernel<float>, dim3(grid), dim3(kThreads), 0, st, (const float *)src, dst, ay, ax, Hi, Wi,
                       k0, total, pad_value);
  DL3_LAUNCH_CHECK("slide_gather");
  return DL3_OK;
}

extern "C" int dl3_slide_accumulate(const float *probs, float *acc, float *wsum, int Hi, int Wi, int H, int W, int C, int sh,
                                    int sw, int k0, int nw, int blend, void *stream) {
  DL3_CHECK_ARG(probs && acc, "slide_accumulate: null pointer");
  DL3_CHECK_ARG(blend == DL3_SLIDE_UNIFORM || blend == DL3_SLIDE_PYRAMID, "slide_accumulate: blend must be 0 (uniform) or 1 (pyramid), got %d",
                blend);
  DL3_CHECK_ARG(C >= 1, "slide_accumulate: C must be positive, got %d", C);
  Axis ay, ax;
  SLIDE_TRY(slide_axes("slide_accumulate", Hi, Wi, H, W, sh, sw, &ay, &ax));
  SLIDE_TRY(slide_windows("slide_accumulate", ay, ax, k0, nw));
  DL3_CHECK_ARG(((uintptr_t)acc & 3) == 0, "slide_accumulate: acc must be 4-byte aligned");
  // a canvas row's float offsets fit an int
  DL3_CHECK_ARG(C <= (1 << 16) && (long long)Wi * C < (1ll << 31) - 8, "slide_accumulate: rows of %d x %d floats are too long", Wi, C);
  const int kyf = k0 / ax.n, kyl = (k0 + nw - 1) / ax.n;
  const int ya = ax_origin(ay, kyf), yb = std::min(ax_origin(ay, kyl) + H, Hi);
  int X0 = 0, X1 = Wi;
  if (kyf == kyl) {
    X0 = ax_origin(ax, k0 - kyf * ax.n);
    X1 = std::min(ax_origin(ax, k0 + nw - 1 - kyf * ax.n) + W, Wi);
  }
  const Geom g = {ay, ax, Hi, Wi, C, blend, k0, k0 + nw, ya, X0, X1 - X0};
  const int run4 = kPix * C / 4;
  const int bpr = (g.R * C / 4 + run4) / run4;   // >= 1; covers every row's 16-byte groups whatever its alignment
  const long long grid = (long long)(yb - ya) * bpr;
  DL3_CHECK_ARG(grid < (1ll << 31), "slide_accumulate: %d rows of %d x %d floats are too many", yb - ya, g.R, C);
  hipLaunchKernelGGL(slide_accumulate_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, probs, acc, wsum, g,
                     bpr);
  DL3_LAUNCH_CHECK("slide_accumulate");
  return DL3_OK;
}

extern "C" int dl3_slide_finalize(const float *acc, const float *wsum, float *probs_out, int *mask_out, int Hi, int Wi, int H,
                                  int W, int C, int sh, int sw, int blend, void *stream) {
  DL3_CHECK_ARG(acc, "slide_finalize: null pointer");
  DL3_CHECK_ARG(probs_out || mask_out, "slide_finalize: probs_out and mask_out are both NULL");
  DL3_CHECK_ARG(blend == DL3_SLIDE_UNIFORM || blend == DL3_SLIDE_PYRAMID, "slide_finalize: blend must be 0 (uniform) or 1 (pyramid), got %d",
                blend);
  DL3_CHECK_ARG(C >= 1 && C <= (1 << 16), "slide_finalize: C must be in [1, 65536], got %d", C);
  Axis ay, ax;
  SLIDE_TRY(slide_axes("slide_finalize", Hi, Wi, H, W, sh, sw, &ay, &ax));
  DL3_CHECK_ARG(((uintptr_t)acc & 3) == 0 && ((uintptr_t)probs_out & 3) == 0, "slide_finalize: acc and probs_out must be 4-byte aligned");
  const Geom g = {ay, ax, Hi, Wi, C, blend, 0, ay.n * ax.n, 0, 0, Wi};
  const int npixels = Hi * Wi;
  hipStream_t st = (hipStream_t)stream;
  if (mask_out) {
    const int grid = std::min((npixels + kThreads - 1) / kThreads, 16384);
    hipLaunchKernelGGL(slide_mask_kernel, dim3(grid), dim3(kThreads), 0, st, acc, wsum, mask_out, g, npixels);
    DL3_LAUNCH_CHECK("slide_finalize");
  }
  if (probs_out) {
    const long long total = (long long)npixels * C;
    const int head = (int)std::min<long long>((long long)(((16 - ((uintptr_t)probs_out & 15)) & 15) / 4), total);
    const long long nvec = (total - head) / 4;
    const long long run4 = (long long)kPix * C / 4;
    const long long grid = nvec > 0 ? (nvec + run4 - 1) / run4 : 1;
    DL3_CHECK_ARG(grid < (1ll << 31), "slide_finalize: %dx%d x %d is too large", Hi, Wi, C);
    hipLaunchKernelGGL(slide_probs_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, acc, wsum, probs_out, g, total, head,
                       nvec);
    DL3_LAUNCH_CHECK("slide_finalize");
  }
  return DL3_OK;
}
