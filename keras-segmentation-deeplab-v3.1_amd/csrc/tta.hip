// tta.hip — multi-scale and flip inference: the two element-wise passes around the forward plan.
//   dl3_tta_resize_image  raw pixels [B][Hi][Wi][3] (float32 or uint8) -> float32 [B][Ho][Wo][3], optionally mirrored
//   dl3_tta_accumulate    one pass's probabilities [B][Hi][Wi][C] -> resized to [B][Ho][Wo][C] (a mirrored pass is read
//                         mirrored) and stored / added into the fp32 accumulator; the last pass divides by the pass count
// Both are the align_corners=True bilinear of [deeplab-semantics] with every operation a separately rounded fp32
// operation in ONE stated order, so that a host restatement with the same order is bit-identical.  hipcc contracts
// a * b + c into a fused multiply-add by default, and the __fmul_rn / __fadd_rn of its headers are plain inline `*` and
// `+` that contract with each other all the same: this file switches contraction OFF for everything it defines
// (`#pragma clang fp contract(off)` below) and writes the operations as plain C++.
//   scale = fl((in - 1) / (out - 1)) (0 where out == 1);  f = fl(o * scale);  lo = min(int(f), in - 1);
//   hi = min(lo + 1, in - 1);  w = fl(f - lo);  top = tl + (tr - tl) * wx;  bot = bl + (br - bl) * wx;
//   v = top + (bot - top) * wy.
//
// dl3_tta_accumulate is an HBM stream over the accumulator, whose [pixel][C] rows (84 bytes at C = 21) are one
// contiguous run of B * Ho * Wo * C floats: a workgroup owns 256 * C consecutive floats of it, cut on 16-byte
// boundaries of the ADDRESS (up to three floats in front of the first boundary and behind the last one are handled
// as scalars by the first / last workgroup), and moves them as 16-byte loads and stores.  The source coordinates and the
// two weights of each of the pixels the run touches (257 as a rule, never more than 264) are computed once, by one lane each, into LDS; a lane then
// walks its four floats through (pixel, channel) without a division per element.  The four source values of an
// element are 4-byte loads — consecutive lanes read consecutive channels of the same source rows, and each source row
// is read by several output pixels out of L2.  No atomics, nothing accumulated across lanes: two runs are bit-identical.
#include <algorithm>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 256;          // accumulator pixels (rows of C floats) per workgroup
constexpr int kPixLds = kPix + 8;  // + the partial rows at either end of a run that starts / ends inside a row

struct Axis {
  int lo, hi;
  float w;
};
__device__ __forceinline__ Axis tta_axis(int o, float scale, int in_size) {
  const float f = (float)o * scale;
  Axis a;
  a.lo = min((int)f, in_size - 1);
  a.hi = min(a.lo + 1, in_size - 1);
  a.w = f - (float)a.lo;
  return a;
}
__device__ __forceinline__ float tta_lerp(float a, float b, float w) { return a + (b - a) * w; }
__device__ __forceinline__ float tta_bilerp(float tl, float tr, float bl, float br, float wx, float wy) {
  return tta_lerp(tta_lerp(tl, tr, wx), tta_lerp(bl, br, wx), wy);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tta_resize_image_kernel(const T *__restrict__ src, float *__restrict__ dst,
                                                                    int B, int Hi, int Wi, int Ho, int Wo, float sy,
                                                                    float sx, int flip) {
  const long long total = (long long)B * Ho * Wo;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kThreads) {
    const int b = (int)(g / ((long long)Ho * Wo));
    const int r = (int)(g - (long long)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    const Axis ay = tta_axis(oy, sy, Hi), ax = tta_axis(flip ? Wo - 1 - ox : ox, sx, Wi);
    const T *sb = src + (size_t)b * Hi * Wi * 3;
    const T *tl = sb + ((size_t)ay.lo * Wi + ax.lo) * 3, *tr = sb + ((size_t)ay.lo * Wi + ax.hi) * 3;
    const T *bl = sb + ((size_t)ay.hi * Wi + ax.lo) * 3, *br = sb + ((size_t)ay.hi * Wi + ax.hi) * 3;
    float *d = dst + (size_t)g * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) d[c] = tta_bilerp((float)tl[c], (float)tr[c], (float)bl[c], (float)br[c], ax.w, ay.w);
  }
}

struct AccGeom {
  int Hi, Wi, Ho, Wo, C;
  float sy, sx;
  int flip, first;
  float n_last;   // 0: not the last pass
};

// one element of the accumulator from its pixel's LDS record
__device__ __forceinline__ float tta_value(const float *__restrict__ probs, const int *po, const float *pw, int lp, int c,
                                           int C) {
  const int *o = po + 4 * lp;
  const float tl = probs[(size_t)o[0] * C + c], tr = probs[(size_t)o[1] * C + c];
  const float bl = probs[(size_t)o[2] * C + c], br = probs[(size_t)o[3] * C + c];
  return tta_bilerp(tl, tr, bl, br, pw[2 * lp], pw[2 * lp + 1]);
}
__device__ __forceinline__ float tta_finish(float v, float old, const AccGeom &g) {
  if (!g.first) v = old + v;
  if (g.n_last > 0.f) v = v / g.n_last;   // IEEE division: hipcc's default for fp32
  return v;
}

// total = B * Ho * Wo * C floats; head = floats in front of the first 16-byte boundary of acc (0..3, <= total);
// nvec = 16-byte groups behind it; the rest (0..3 floats) is the tail
__global__ __launch_bounds__(kThreads) void tta_accumulate_kernel(const float *__restrict__ probs, float *__restrict__ acc,
                                                                  AccGeom g, long long total, int head, long long nvec) {
  __shared__ int po[4 * kPixLds];     // source pixel index (within the batch) of tl, tr, bl, br
  __shared__ float pw[2 * kPixLds];   // wx, wy
  const int tid = threadIdx.x, C = g.C;
  const long long run = (long long)kPix * C;   // floats per workgroup, a multiple of 4
  const bool is_first = blockIdx.x == 0, is_last = blockIdx.x == gridDim.x - 1;
  const long long e_beg = is_first ? 0 : head + (long long)blockIdx.x * run;
  const long long e_end = is_last ? total : head + ((long long)blockIdx.x + 1) * run;
  const long long p_beg = e_beg / C;
  const int npix = (int)((e_end - 1) / C - p_beg) + 1;   // <= kPix + 7 (head and tail are at most 3 floats each)
  const int HWo = g.Ho * g.Wo;
  for (int i = tid; i < npix; i += kThreads) {
    const long long gp = p_beg + i;
    const int b = (int)(gp / HWo);
    const int r = (int)(gp - (long long)b * HWo);
    const int oy = r / g.Wo, ox = r - oy * g.Wo;
    const Axis ay = tta_axis(oy, g.sy, g.Hi), ax = tta_axis(ox, g.sx, g.Wi);
    // a mirrored pass: source column x sits at index Wi - 1 - x
    const int xl = g.flip ? g.Wi - 1 - ax.lo : ax.lo, xh = g.flip ? g.Wi - 1 - ax.hi : ax.hi;
    const int base = b * g.Hi * g.Wi;
    po[4 * i + 0] = base + ay.lo * g.Wi + xl;
    po[4 * i + 1] = base + ay.lo * g.Wi + xh;
    po[4 * i + 2] = base + ay.hi * g.Wi + xl;
    po[4 * i + 3] = base + ay.hi * g.Wi + xh;
    pw[2 * i + 0] = ax.w;
    pw[2 * i + 1] = ay.w;
  }
  __syncthreads();

  // the 16-byte groups of this workgroup's run
  const long long v_beg = (long long)blockIdx.x * (run / 4);
  const int nv = (int)min((long long)(run / 4), nvec - v_beg);
  for (int t = tid; t < nv; t += kThreads) {
    const long long e = head + 4 * (v_beg + t);
    const int rel = (int)(e - p_beg * C);   // < kPixLds * C: a 32-bit division
    int lp = rel / C, c = rel - lp * C;
    f32x4 v = splat4(0.f);
    if (!g.first) v = ld4(acc + e);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] = tta_finish(tta_value(probs, po, pw, lp, c, C), v[k], g);
      if (++c == C) {
        c = 0;
        lp++;
      }
    }
    st4(acc + e, v);
  }
  // scalars in front of the first boundary and behind the last group
  if (is_first && tid < head) {
    const long long e = tid;
    const long long gp = e / C;
    acc[e] = tta_finish(tta_value(probs, po, pw, (int)(gp - p_beg), (int)(e - gp * C), C), g.first ? 0.f : acc[e], g);
  }
  const long long t_beg = head + 4 * nvec;
  if (is_last && tid < (int)(total - t_beg)) {
    const long long e = t_beg + tid;
    const long long gp = e / C;
    acc[e] = tta_finish(tta_value(probs, po, pw, (int)(gp - p_beg), (int)(e - gp * C), C), g.first ? 0.f : acc[e], g);
  }
}

inline float tta_scale(int in_size, int out_size) { return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f; }

}  // namespace

extern "C" int dl3_tta_resize_image(const void *src, int src_dtype, float *dst, int B, int Hi, int Wi, int Ho, int Wo,
                                    int flip, void *stream) {
  DL3_CHECK_ARG(src && dst, "tta_resize_image: null pointer");
  DL3_CHECK_ARG(src_dtype == DL3_TTA_F32 || src_dtype == DL3_TTA_U8, "tta_resize_image: src_dtype must be 0 (float32) or 1 (uint8), got %d",
                src_dtype);
  DL3_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "tta_resize_image: sizes must be positive, got %d x %dx%d -> %dx%d",
                B, Hi, Wi, Ho, Wo);
  DL3_CHECK_ARG(flip == 0 || flip == 1, "tta_resize_image: flip must be 0 or 1, got %d", flip);
  DL3_CHECK_ARG((long long)B * Hi * Wi * 3 < (1ll << 31) && (long long)B * Ho * Wo * 3 < (1ll << 31),
                "tta_resize_image: %d x %dx%d -> %dx%d is too large", B, Hi, Wi, Ho, Wo);
  const long long total = (long long)B * Ho * Wo;
  const int grid = (int)std::min<long long>((total + kThreads - 1) / kThreads, 8192);
  const float sy = tta_scale(Hi, Ho), sx = tta_scale(Wi, Wo);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == DL3_TTA_U8)
    hipLaunchKernelGGL(tta_resize_image_kernel<unsigned char>, dim3(grid), dim3(kThreads), 0, st, (const unsigned char *)src,
                       dst, B, Hi, Wi, Ho, Wo, sy, sx, flip);
  else
    hipLaunchKernelGGL(tta_resize_image_kernel<float>, dim3(grid), dim3(kThreads), 0, st, (const float *)src, dst, B, Hi, Wi,
                       Ho, Wo, sy, sx, flip);
  DL3_LAUNCH_CHECK("tta_resize_image");
  return DL3_OK;
}

extern "C" int dl3_tta_accumulate(const float *probs, float *acc, int B, int Hi, int Wi, int Ho, int Wo, int C, int flip,
                                  int first, int n_passes_if_last, void *stream) {
  DL3_CHECK_ARG(probs && acc, "tta_accumulate: null pointer");
  DL3_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "tta_accumulate: sizes must be positive, got %d x %dx%d -> %dx%d x %d", B, Hi, Wi, Ho, Wo, C);
  DL3_CHECK_ARG((flip == 0 || flip == 1) && (first == 0 || first == 1), "tta_accumulate: flip and first must be 0 or 1, got %d, %d",
                flip, first);
  DL3_CHECK_ARG(n_passes_if_last >= 0 && n_passes_if_last <= (1 << 24), "tta_accumulate: n_passes_if_last must be in [0, 2^24], got %d",
                n_passes_if_last);
  DL3_CHECK_ARG(((uintptr_t)acc & 3) == 0, "tta_accumulate: acc must be 4-byte aligned");
  // every pixel index fits an int, a workgroup's float offsets are 64-bit
  DL3_CHECK_ARG((long long)B * Hi * Wi < (1ll << 31) && (long long)B * Ho * Wo < (1ll << 31) && C <= (1 << 16),
                "tta_accumulate: %d x %dx%d -> %dx%d x %d is too large", B, Hi, Wi, Ho, Wo, C);
  const long long total = (long long)B * Ho * Wo * C;
  const int head = (int)std::min<long long>((long long)(((16 - ((uintptr_t)acc & 15)) & 15) / 4), total);
  const long long nvec = (total - head) / 4;
  const long long run4 = (long long)kPix * C / 4;
  const long long grid = nvec > 0 ? (nvec + run4 - 1) / run4 : 1;
  DL3_CHECK_ARG(grid < (1ll << 31), "tta_accumulate: %d x %dx%d x %d is too large", B, Ho, Wo, C);
  const AccGeom g = {Hi, Wi, Ho, Wo, C, tta_scale(Hi, Ho), tta_scale(Wi, Wo), flip, first, (float)n_passes_if_last};
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, probs, acc, g, total,
                     head, nvec);
  DL3_LAUNCH_CHECK("tta_accumulate");
  return DL3_OK;
}
