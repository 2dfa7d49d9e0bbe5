// augment.hip — the augmentation chain of the reference's SegmentationGenerator.__getitem__ (utils.py:310-369) on the
// device, between the H2D byte copy and the target preparation.  The host (augment.py) takes every floating-point
// decision per image in float64 — gamma LUT, inverse affine matrix, cv2's fixed-point warp tables, CLAHE interpolation
// weights — and hands them over as flat int / float tables, so the device does integer adds and shifts only.
//   stage 1  : 5x5 Gaussian blur (LDS halo, reflect-101 at the source borders), crop, flips, gamma LUT
//   present  : per-image 256-bit set of the labels in the whole source map (integer atomicOr), only when warping
//   warp     : cv2.warpAffine INTER_LINEAR, 1/32-pixel fixed point, constant-0 border, for the image and the uint8 label
//              map, then the void relabel; writes float32 X, or (CLAHE on) a uint8 YUV image + one LUT per CLAHE tile
//              (one workgroup per tile: histogram, clip / redistribute and the 256-entry LUT stay in LDS)
//   clahe    : bilinear interpolation between the four neighbouring tile LUTs (float32, no contraction), YUV -> BGR,
//              widening to float32
// Integer atomics only: every result is bit-reproducible.
#include "common.h"
#include "augmath.h"

namespace {

constexpr int kTW = 64, kTH = 16;           // stage-1 tile (source pixels of the crop)
constexpr int kHalo = 2;                    // 5x5 stencil
constexpr int kSW = kTW + 2 * kHalo, kSH = kTH + 2 * kHalo;
constexpr int kTiles = 8;                   // CLAHE tile grid (8x8, utils.py:53)

__device__ __forceinline__ int reflect101(int i, int n) {
  // -1 -> 1, n -> n-2; the clamp only guards tile pixels outside the crop, whose values are never used
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ int sat_u8(int v) { return min(max(v, 0), 255); }

// img_params[b] = {blur_on, crop_x, crop_y, hflip, vflip, 0, 0, 0}; lut[b][256]
template <typename TL, bool kFloatOut>
__global__ __launch_bounds__(256) void stage1_kernel(const unsigned char *__restrict__ src, const TL *__restrict__ lsrc,
                                                     int Hs, int Ws, int H, int W, const int *__restrict__ img_params,
                                                     const int *__restrict__ lut, unsigned char *__restrict__ out8,
                                                     float *__restrict__ outf, TL *__restrict__ lout) {
  __shared__ unsigned char tile[kSH * kSW * 3];
  __shared__ int hrow[kSH * kTW * 3];
  __shared__ int slut[256];
  const int b = blockIdx.z;
  const int *pp = img_params + 8 * b;
  const int blur = pp[0], cx = pp[1], cy = pp[2], hf = pp[3], vf = pp[4];
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;  // tile origin in crop coordinates
  const unsigned char *s = src + (size_t)b * Hs * Ws * 3;
  slut[threadIdx.x] = lut[b * 256 + threadIdx.x];
  if (blur) {
    for (int i = threadIdx.x; i < kSH * kSW * 3; i += 256) {
      const int r = i / (kSW * 3), rem = i - r * (kSW * 3), c = rem / 3, ch = rem - c * 3;
      const int sy = reflect101(cy + ty0 - kHalo + r, Hs), sx = reflect101(cx + tx0 - kHalo + c, Ws);
      tile[i] = s[((size_t)sy * Ws + sx) * 3 + ch];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSH * kTW * 3; i += 256) {  // horizontal [1 4 6 4 1]
      const int r = i / (kTW * 3), rem = i - r * (kTW * 3);
      const unsigned char *t = tile + r * kSW * 3 + rem;
      hrow[i] = blur5_row(t);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTH * kTW; i += 256) {
    const int r = i / kTW, c = i - r * kTW;
    const int y = ty0 + r, x = tx0 + c;
    if (y >= H || x >= W) continue;
    const int oy = vf ? H - 1 - y : y, ox = hf ? W - 1 - x : x;
    const size_t o = ((size_t)b * H + oy) * W + ox;
    int v[3];
    for (int ch = 0; ch < 3; ch++) {
      int p;
      if (blur) {  // vertical [1 4 6 4 1]; (sum + 128) >> 8
        p = blur5_col(hrow + r * kTW * 3 + c * 3 + ch, kTW * 3);
      } else {
        p = s[((size_t)(cy + y) * Ws + cx + x) * 3 + ch];
      }
      v[ch] = slut[p];
    }
    if (kFloatOut) {
      outf[o * 3 + 0] = (float)v[0];
      outf[o * 3 + 1] = (float)v[1];
      outf[o * 3 + 2] = (float)v[2];
    } else {
      out8[o * 3 + 0] = (unsigned char)v[0];
      out8[o * 3 + 1] = (unsigned char)v[1];
      out8[o * 3 + 2] = (unsigned char)v[2];
    }
    lout[o] = lsrc[((size_t)b * Hs + cy + y) * Ws + cx + x];
  }
}

// present[b][8]: bit v set when label value v occurs anywhere in the source map (np.unique(label), utils.py:317).
// Each lane gathers its 256-bit set in registers (16-byte loads; the word is chosen by selects, not by a runtime index),
// the wave ORs the eight words together and one lane per wave issues the atomics.
__global__ __launch_bounds__(256) void present_kernel(const unsigned char *__restrict__ lsrc, int n,
                                                      int *__restrict__ present) {
  __shared__ int bits[8];
  const int b = blockIdx.y;
  if (threadIdx.x < 8) bits[threadIdx.x] = 0;
  __syncthreads();
  unsigned m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned char *l1 = lsrc + (size_t)b * n;
  const int n16 = (n & 15) ? 0 : n / 16;  // 16-byte loads only when every image plane is 16-byte aligned
  const uint4 *l16 = reinterpret_cast<const uint4 *>(l1);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) {
    const uint4 q = l16[i];
    const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) present_add(m, (w4[j] >> (8 * k)) & 255u);
  }
  for (int i = 16 * n16 + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) present_add(m, l1[i]);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    unsigned v = m[k];
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicOr(&bits[k], (int)v);
  }
  __syncthreads();
  if (threadIdx.x < 8 && bits[threadIdx.x]) atomicOr(&present[b * 8 + threadIdx.x], bits[threadIdx.x]);
}

// warp tables of image b: adelta[W], bdelta[W], X0[H], Y0[H] at warp_tab + b * 2 * (W + H)
struct WarpTap {
  int o[4];   // byte offsets of the four taps in the image plane, -1 outside the source
  int w[4];
};

__device__ __forceinline__ WarpTap warp_taps(const int *__restrict__ tab, int H, int W, int y, int x) {
  const int X = (tab[2 * W + y] + tab[x]) >> 5, Y = (tab[2 * W + H + y] + tab[W + x]) >> 5;
  const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
  WarpTap t;
  t.w[0] = (32 - fy) * (32 - fx) * 32;
  t.w[1] = (32 - fy) * fx * 32;
  t.w[2] = fy * (32 - fx) * 32;
  t.w[3] = fy * fx * 32;
  const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
  const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
  const int base = sy * W + sx;
  t.o[0] = (y0 && x0) ? base : -1;
  t.o[1] = (y0 && x1) ? base + 1 : -1;
  t.o[2] = (y1 && x0) ? base + W : -1;
  t.o[3] = (y1 && x1) ? base + W + 1 : -1;
  return t;
}

__device__ __forceinline__ int warp_sample(const unsigned char *__restrict__ p, int stride, int ch, const WarpTap &t) {
  int acc = 16384;
#pragma unroll
  for (int k = 0; k < 4; k++) acc += t.o[k] >= 0 ? t.w[k] * (int)p[t.o[k] * stride + ch] : 0;
  return acc >> 15;
}

__device__ __forceinline__ unsigned char warp_label(const unsigned char *__restrict__ l, const WarpTap &t,
                                                    const int *__restrict__ present, int C) {
  const int v = warp_sample(l, 1, 0, t);
  return ((present[v >> 5] >> (v & 31)) & 1) ? (unsigned char)v : (unsigned char)C;
}

// no CLAHE: 4 consecutive pixels per thread -> 12 floats = 3 float4 stores (when the image plane is 16-byte aligned)
__global__ __launch_bounds__(256) void warp_kernel(const unsigned char *__restrict__ img, const unsigned char *__restrict__ lab,
                                                   int H, int W, const int *__restrict__ warp_tab, int warp_label_on,
                                                   const int *__restrict__ present, int C, float *__restrict__ X,
                                                   unsigned char *__restrict__ lout) {
  const int b = blockIdx.y, HW = H * W;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  const int *tab = warp_tab + (size_t)b * 2 * (W + H);
  const unsigned char *ib = img + (size_t)b * HW * 3;
  float v[12];
  unsigned char l[4];
  const int n = min(4, HW - p0);
  for (int k = 0; k < 4; k++) {
    const int p = p0 + (k < n ? k : 0), y = p / W, x = p - y * W;
    const WarpTap t = warp_taps(tab, H, W, y, x);
    v[3 * k + 0] = (float)warp_sample(ib, 3, 0, t);
    v[3 * k + 1] = (float)warp_sample(ib, 3, 1, t);
    v[3 * k + 2] = (float)warp_sample(ib, 3, 2, t);
    if (warp_label_on) l[k] = warp_label(lab + (size_t)b * HW, t, present + 8 * b, C);
  }
  float *xo = X + ((size_t)b * HW + p0) * 3;
  unsigned char *lo = lout + (size_t)b * HW + p0;
  if (n == 4 && (HW & 3) == 0) {
    st4(xo, f32x4{v[0], v[1], v[2], v[3]});
    st4(xo + 4, f32x4{v[4], v[5], v[6], v[7]});
    st4(xo + 8, f32x4{v[8], v[9], v[10], v[11]});
    if (warp_label_on) *reinterpret_cast<uchar4 *>(lo) = make_uchar4(l[0], l[1], l[2], l[3]);
  } else {
    for (int k = 0; k < n; k++) {
      xo[3 * k] = v[3 * k];
      xo[3 * k + 1] = v[3 * k + 1];
      xo[3 * k + 2] = v[3 * k + 2];
      if (warp_label_on) lo[k] = l[k];
    }
  }
}

// cv2 COLOR_BGR2YUV, 8-bit, 14-bit fixed point
__device__ __forceinline__ int yuv_y(int B, int G, int R) { return (4899 * R + 9617 * G + 1868 * B + 8192) >> 14; }

// CLAHE on: one workgroup per (tile, image).  The tile covers the padded plane (reflect-101 bottom / right padding when
// H or W is not a multiple of 8: its pixels are the warped values at the reflected coordinates and count in the
// histogram); real pixels write YUV and the relabelled label.  lut_out[b][64][256].
__global__ __launch_bounds__(256) void warp_clahe_kernel(const unsigned char *__restrict__ img,
                                                         const unsigned char *__restrict__ lab, int H, int W, int th,
                                                         int tw, const int *__restrict__ warp_tab, int warp_label_on,
                                                         const int *__restrict__ present, int C,
                                                         unsigned char *__restrict__ yuv, unsigned char *__restrict__ lout,
                                                         unsigned char *__restrict__ lut_out) {
  __shared__ int hist[256];
  __shared__ int excess;
  const int b = blockIdx.y, tile = blockIdx.x, ty = tile / kTiles, tx = tile - ty * kTiles;
  const int HW = H * W;
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) excess = 0;
  __syncthreads();
  const int *tab = warp_tab + (size_t)b * 2 * (W + H);
  const unsigned char *ib = img + (size_t)b * HW * 3;
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int r = i / tw, py = ty * th + r, px = tx * tw + (i - r * tw);
    const int y = reflect101(py, H), x = reflect101(px, W);
    const WarpTap t = warp_taps(tab, H, W, y, x);
    const int B = warp_sample(ib, 3, 0, t), G = warp_sample(ib, 3, 1, t), R = warp_sample(ib, 3, 2, t);
    const int Y = yuv_y(B, G, R);
    atomicAdd(&hist[Y], 1);
    if (py < H && px < W) {
      const size_t o = (size_t)b * HW + (size_t)py * W + px;
      yuv[o * 3 + 0] = (unsigned char)Y;
      yuv[o * 3 + 1] = (unsigned char)sat_u8(((B - Y) * 8061 + (128 << 14) + 8192) >> 14);
      yuv[o * 3 + 2] = (unsigned char)sat_u8(((R - Y) * 14369 + (128 << 14) + 8192) >> 14);
      if (warp_label_on) lout[o] = warp_label(lab + (size_t)b * HW, t, present + 8 * b, C);
    }
  }
  __syncthreads();
  const int area = th * tw;
  const int clip = max((int)(2.0 * area / 256), 1);
  int h = hist[threadIdx.x];
  if (h > clip) {
    atomicAdd(&excess, h - clip);
    h = clip;
  }
  __syncthreads();
  const int ex = excess, batch = ex / 256, residual = ex - batch * 256;
  h += batch;
  if (residual) {
    const int step = max(256 / residual, 1);
    if (threadIdx.x % step == 0 && threadIdx.x / step < residual) h++;
  }
  hist[threadIdx.x] = h;
  __syncthreads();
  if (threadIdx.x < 64) {  // one wave: inclusive scan, 4 bins per lane
    const int l = threadIdx.x;
    int c0 = hist[4 * l], c1 = c0 + hist[4 * l + 1], c2 = c1 + hist[4 * l + 2], c3 = c2 + hist[4 * l + 3];
    int run = c3;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(run, o, 64);
      if (l >= o) run += u;
    }
    const int off = run - c3;
    const float scale = 255.0f / (float)area;
    unsigned char *lo = lut_out + ((size_t)b * kTiles * kTiles + tile) * 256 + 4 * l;
    const int cs[4] = {c0 + off, c1 + off, c2 + off, c3 + off};
    for (int k = 0; k < 4; k++) lo[k] = (unsigned char)sat_u8((int)__builtin_rintf((float)cs[k] * scale));
  }
}

// CLAHE apply: clahe_i[W*2 + H*2] = tx1, tx2 per x then ty1, ty2 per y (tile indices, clamped);
// clahe_f[2W + 2H] = xa, 1-xa per x then ya, 1-ya per y
__global__ __launch_bounds__(256) void clahe_apply_kernel(const unsigned char *__restrict__ yuv, int H, int W,
                                                          const int *__restrict__ ci, const float *__restrict__ cf,
                                                          const unsigned char *__restrict__ luts,
                                                          float *__restrict__ X) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, HW = H * W;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  const unsigned char *lb = luts + (size_t)b * kTiles * kTiles * 256;
  float v[12];
  const int n = min(4, HW - p0);
  for (int k = 0; k < 4; k++) {
    const int p = p0 + (k < n ? k : 0), y = p / W, x = p - y * W;
    const unsigned char *q = yuv + ((size_t)b * HW + p) * 3;
    const int Y = q[0], U = q[1] - 128, V = q[2] - 128;
    const int tx1 = ci[2 * x], tx2 = ci[2 * x + 1], ty1 = ci[2 * W + 2 * y], ty2 = ci[2 * W + 2 * y + 1];
    const float xa = cf[2 * x], xa1 = cf[2 * x + 1], ya = cf[2 * W + 2 * y], ya1 = cf[2 * W + 2 * y + 1];
    const float l11 = lb[(ty1 * kTiles + tx1) * 256 + Y], l12 = lb[(ty1 * kTiles + tx2) * 256 + Y];
    const float l21 = lb[(ty2 * kTiles + tx1) * 256 + Y], l22 = lb[(ty2 * kTiles + tx2) * 256 + Y];
    // (L11*xa1 + L12*xa)*ya1 + (L21*xa1 + L22*xa)*ya, rounded after every operation
    const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
    const int Yn = sat_u8((int)__builtin_rintf(res));
    v[3 * k + 0] = (float)sat_u8(Yn + ((U * 33292 + 8192) >> 14));
    v[3 * k + 1] = (float)sat_u8(Yn + ((U * -6472 + V * -9519 + 8192) >> 14));
    v[3 * k + 2] = (float)sat_u8(Yn + ((V * 18678 + 8192) >> 14));
  }
  float *xo = X + ((size_t)b * HW + p0) * 3;
  if (n == 4 && (HW & 3) == 0) {
    st4(xo, f32x4{v[0], v[1], v[2], v[3]});
    st4(xo + 4, f32x4{v[4], v[5], v[6], v[7]});
    st4(xo + 8, f32x4{v[8], v[9], v[10], v[11]});
  } else {
    for (int k = 0; k < 3 * n; k++) xo[k] = v[k];
  }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct AugLayout {
  size_t img, lab, present, yuv, luts, total;
};

AugLayout aug_layout(int B, int H, int W, int flags) {
  const bool warp = flags & DL3_AUG_WARP, clahe = flags & DL3_AUG_CLAHE;
  const size_t px = (size_t)B * H * W;
  AugLayout L{};
  size_t o = 0;
  L.img = o;
  if (warp || clahe) o += align256(px * 3);
  L.lab = o;
  if (warp) o += align256(px);
  L.present = o;
  if (warp) o += align256((size_t)B * 8 * sizeof(int));
  L.yuv = o;
  if (clahe) o += align256(px * 3);
  L.luts = o;
  if (clahe) o += align256((size_t)B * kTiles * kTiles * 256);
  L.total = o;
  return L;
}

// present_in: the label sets of the batch from outside (dl3_augment_present), or NULL: taken from `labels` here
int augment_run(const void *images, const void *labels, int label_dtype, int B, int Hs, int Ws, int H, int W, int flags,
                const int *img_params, const int *lut, const int *warp_tab, const int *clahe_i, const float *clahe_f,
                int C, const int *present_in, float *X, void *labels_out, void *workspace, size_t workspace_bytes,
                void *stream) {
  DL3_CHECK_ARG(images && labels && img_params && lut && X && labels_out && B > 0, "augment: bad argument");
  DL3_CHECK_ARG(H >= 3 && W >= 3 && Hs >= H && Ws >= W, "augment: output %dx%d must be at least 3x3 and fit the %dx%d "
                "source (crops larger than the source are not supported)", H, W, Hs, Ws);
  DL3_CHECK_ARG(label_dtype == DL3_LABEL_U8 || label_dtype == DL3_LABEL_I32, "augment: unknown label dtype %d",
                label_dtype);
  DL3_CHECK_ARG((flags & ~(DL3_AUG_WARP | DL3_AUG_CLAHE)) == 0, "augment: unknown flags 0x%x", flags);
  const bool warp = flags & DL3_AUG_WARP, clahe = flags & DL3_AUG_CLAHE;
  // void = C is written only by the warp's relabel, into a uint8 label map
  DL3_CHECK_ARG(C > 0 && (!warp || C <= 255), "augment: classes must be positive (at most 255 when warping), got %d", C);
  DL3_UNSUPPORTED(warp && label_dtype != DL3_LABEL_U8,
                  "augment: the warp interpolates the label map as uint8 (cv2.warpAffine); int32 label maps cannot be "
                  "warped");
  DL3_CHECK_ARG(!(warp || clahe) || warp_tab, "augment: warp / CLAHE need the warp tables");
  DL3_CHECK_ARG(!clahe || (clahe_i && clahe_f), "augment: CLAHE needs its interpolation tables");
  // CLAHE's padded tiles must reflect once: padding (< 8 or == 8) stays below H - 1
  DL3_UNSUPPORTED(clahe && (H < 16 || W < 16), "augment: CLAHE needs an image of at least 16x16, got %dx%d", H, W);
  const AugLayout L = aug_layout(B, H, W, flags);
  DL3_CHECK_ARG(!L.total || (workspace && workspace_bytes >= L.total), "augment: workspace of %zu bytes, needs %zu",
                workspace_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  unsigned char *ws = (unsigned char *)workspace;
  unsigned char *img8 = ws + L.img, *lab8 = ws + L.lab, *yuv = ws + L.yuv, *luts = ws + L.luts;
  const int *present = present_in ? present_in : (const int *)(ws + L.present);
  const dim3 g1(dl3_cdiv(W, kTW), dl3_cdiv(H, kTH), B);
  const bool fout = !(warp || clahe);
  void *lstage = warp ? (void *)lab8 : labels_out;
  if (label_dtype == DL3_LABEL_U8) {
    auto k = fout ? stage1_kernel<unsigned char, true> : stage1_kernel<unsigned char, false>;
    hipLaunchKernelGGL(k, g1, dim3(256), 0, st, (const unsigned char *)images, (const unsigned char *)labels, Hs, Ws, H,
                       W, img_params, lut, img8, X, (unsigned char *)lstage);
  } else {
    auto k = fout ? stage1_kernel<int, true> : stage1_kernel<int, false>;
    hipLaunchKernelGGL(k, g1, dim3(256), 0, st, (const unsigned char *)images, (const int *)labels, Hs, Ws, H, W,
                       img_params, lut, img8, X, (int *)lstage);
  }
  if (warp && !present_in) {
    int *own = (int *)(ws + L.present);
    (void)hipMemsetAsync(own, 0, (size_t)B * 8 * sizeof(int), st);
    const int n = Hs * Ws;
    hipLaunchKernelGGL(present_kernel, dim3(min(max(dl3_cdiv(n, 256 * 64), 1), 64), B), dim3(256), 0, st,
                       (const unsigned char *)labels, n, own);
  }
  if (clahe) {
    const int Hp = (H % kTiles || W % kTiles) ? H + kTiles - H % kTiles : H;
    const int Wp = (H % kTiles || W % kTiles) ? W + kTiles - W % kTiles : W;
    hipLaunchKernelGGL(warp_clahe_kernel, dim3(kTiles * kTiles, B), dim3(256), 0, st, img8, lab8, H, W, Hp / kTiles,
                       Wp / kTiles, warp_tab, (int)warp, present, C, yuv, (unsigned char *)labels_out, luts);
    hipLaunchKernelGGL(clahe_apply_kernel, dim3(dl3_cdiv(H * W, 1024), B), dim3(256), 0, st, yuv, H, W, clahe_i,
                       clahe_f, luts, X);
  } else if (warp) {
    hipLaunchKernelGGL(warp_kernel, dim3(dl3_cdiv(H * W, 1024), B), dim3(256), 0, st, img8, lab8, H, W, warp_tab, 1,
                       present, C, X, (unsigned char *)labels_out);
  }
  DL3_LAUNCH_CHECK("augment");
  return DL3_OK;
}

}  // namespace

extern "C" size_t dl3_augment_workspace_bytes(int B, int H, int W, int flags) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return aug_layout(B, H, W, flags).total;
}

extern "C" int dl3_augment(const void *images, const void *labels, int label_dtype, int B, int Hs, int Ws, int H,
                           int W, int flags, const int *img_params, const int *lut, const int *warp_tab,
                           const int *clahe_i, const float *clahe_f, int C, float *X, void *labels_out,
                           void *workspace, size_t workspace_bytes, void *stream) {
  return augment_run(images, labels, label_dtype, B, Hs, Ws, H, W, flags, img_params, lut, warp_tab, clahe_i, clahe_f, C,
                     nullptr, X, labels_out, workspace, workspace_bytes, stream);
}

extern "C" int dl3_augment_present(const void *images, const void *labels, int label_dtype, int B, int Hs, int Ws, int H,
                                   int W, int flags, const int *img_params, const int *lut, const int *warp_tab,
                                   const int *clahe_i, const float *clahe_f, int C, const int *present, float *X,
                                   void *labels_out, void *workspace, size_t workspace_bytes, void *stream) {
  DL3_CHECK_ARG(present, "augment: dl3_augment_present needs the label sets");
  return augment_run(images, labels, label_dtype, B, Hs, Ws, H, W, flags, img_params, lut, warp_tab, clahe_i, clahe_f, C,
                     present, X, labels_out, workspace, workspace_bytes, stream);
}
