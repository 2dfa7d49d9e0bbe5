// cvresize.hip — cv2.resize in front of the augmentation chain: the reference's default data path resizes every decoded
// image (INTER_LINEAR) and label map (INTER_NEAREST) to the model's size (utils.py:322-324, :421-422).  B source images
// of DIFFERENT sizes lie back to back in one uint8 pool, their label maps in a second pool; one launch per stage, the
// image index a grid dimension, writes the uniform batch dl3_augment reads.
//   blur    : (only when some image draws it) 5x5 Gaussian at the SOURCE size into a workspace laid out like the pool,
//             reflect-101 at each image's own borders
//   present : per-image 256-bit set of the label values of the source-size map (integer atomicOr)
//   resize  : mode 0 — cv2's 8-bit INTER_LINEAR (11-bit coefficients, the two-pass integer rounding) for the image,
//             INTER_NEAREST for the label map; mode 1 — the H x W crop at (crop_x, crop_y)
// The host (augment.resize_tables) takes every floating-point decision — cv2's float32 source coordinates and
// coefficients — and uploads them per distinct source size; the device does integer multiplies, adds and shifts only.
// The descriptors are trusted: the Python wrapper checks pools, sizes and crops before the upload.
#include "common.h"
#include "augmath.h"

namespace {

constexpr int kDesc = 12;                   // ints per image descriptor
constexpr int kTW = 64, kTH = 16;           // blur tile
constexpr int kHalo = 2;
constexpr int kSW = kTW + 2 * kHalo, kSH = kTH + 2 * kHalo;

// cv2's BORDER_REFLECT_101 for any distance from the image (a 1- or 2-pixel image reflects more than once)
__device__ __forceinline__ int reflect101_any(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// desc[b] = {image offset (bytes), label offset (elements), Hs, Ws, blur_on, mode, crop_x, crop_y, table offset, 0, 0, 0}
__global__ __launch_bounds__(256) void blur_ragged_kernel(const unsigned char *__restrict__ pool,
                                                          const int *__restrict__ desc,
                                                          unsigned char *__restrict__ out) {
  __shared__ unsigned char tile[kSH * kSW * 3];
  __shared__ int hrow[kSH * kTW * 3];
  const int *d = desc + kDesc * blockIdx.z;
  const int Hs = d[2], Ws = d[3];
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
  if (!d[4] || tx0 >= Ws || ty0 >= Hs) return;  // uniform over the workgroup
  const unsigned char *s = pool + d[0];
  unsigned char *o = out + d[0];
  for (int i = threadIdx.x; i < kSH * kSW * 3; i += 256) {
    const int r = i / (kSW * 3), rem = i - r * (kSW * 3), c = rem / 3, ch = rem - c * 3;
    const int sy = reflect101_any(ty0 - kHalo + r, Hs), sx = reflect101_any(tx0 - kHalo + c, Ws);
    tile[i] = s[(sy * Ws + sx) * 3 + ch];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSH * kTW * 3; i += 256) {  // horizontal [1 4 6 4 1]
    const int r = i / (kTW * 3), rem = i - r * (kTW * 3);
    const unsigned char *t = tile + r * kSW * 3 + rem;
    hrow[i] = blur5_row(t);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTH * kTW * 3; i += 256) {  // vertical [1 4 6 4 1]
    const int r = i / (kTW * 3), rem = i - r * (kTW * 3), c = rem / 3;
    const int y = ty0 + r, x = tx0 + c;
    if (y >= Hs || x >= Ws) continue;
    o[(y * Ws + tx0) * 3 + rem] = (unsigned char)blur5_col(hrow + r * kTW * 3 + rem, kTW * 3);
  }
}

// present[b][8]: bit v set when label value v occurs in the source map of image b (np.unique(label), utils.py:317);
// int32 values outside 0..255 set nothing.  A map starts anywhere in the pool: bytes up to the first 16-byte boundary,
// 16-byte loads, then the tail.
template <typename TL>
__global__ __launch_bounds__(256) void present_ragged_kernel(const TL *__restrict__ lpool, const int *__restrict__ desc,
                                                             int *__restrict__ present) {
  __shared__ int bits[8];
  const int b = blockIdx.y;
  const int *d = desc + kDesc * b;
  const int n = d[2] * d[3];
  const TL *l = lpool + d[1];
  if (threadIdx.x < 8) bits[threadIdx.x] = 0;
  __syncthreads();
  unsigned m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  if constexpr (sizeof(TL) == 1) {
    const int head = min(n, (int)((16 - ((uintptr_t)l & 15)) & 15)), n16 = (n - head) / 16;
    for (int i = t0; i < head; i += stride) present_add(m, l[i]);
    const uint4 *l16 = reinterpret_cast<const uint4 *>(l + head);
    for (int i = t0; i < n16; i += stride) {
      const uint4 q = l16[i];
      const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) present_add(m, (w4[j] >> (8 * k)) & 255u);
    }
    for (int i = head + 16 * n16 + t0; i < n; i += stride) present_add(m, l[i]);
  } else {
    for (int i = t0; i < n; i += stride) {
      const unsigned v = (unsigned)l[i];
      if (v < 256u) present_add(m, v);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    unsigned v = m[k];
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicOr(&bits[k], (int)v);
  }
  __syncthreads();
  if (threadIdx.x < 8 && bits[threadIdx.x]) atomicOr(&present[b * 8 + threadIdx.x], bits[threadIdx.x]);
}

// tables of one source size at tab + desc[8]: xs[W], xa0[W], xa1[W], xn[W], ys[H], yb0[H], yb1[H], yn[H] —
// xs already clamped to [0, Ws-1] (cv2 clamps columns and zeroes their fraction), ys as floor() left it (rows keep their
// coefficients and clamp the two taps), xn / yn the INTER_NEAREST source index.
// 4 consecutive output pixels per thread: 12 image bytes = 3 dword stores when `vec` (planes and bases 4-byte aligned).
template <typename TL>
__global__ __launch_bounds__(256) void resize_ragged_kernel(const unsigned char *__restrict__ pool,
                                                            const unsigned char *__restrict__ blurred,
                                                            const TL *__restrict__ lpool, const int *__restrict__ desc,
                                                            const int *__restrict__ tab, int H, int W,
                                                            unsigned char *__restrict__ out, TL *__restrict__ lout,
                                                            int vec) {
  const int b = blockIdx.y, HW = H * W;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  const int *d = desc + kDesc * b;
  const int Hs = d[2], Ws = d[3], mode = d[5], cx = d[6], cy = d[7];
  const unsigned char *s = (d[4] ? blurred : pool) + d[0];
  const TL *ls = lpool + d[1];
  const int *t = tab + d[8];
  const int n = min(4, HW - p0);
  unsigned v[12];
  TL l[4];
  for (int k = 0; k < 4; k++) {
    const int p = p0 + (k < n ? k : 0), y = p / W, x = p - y * W;
    if (mode) {
      const int so = (cy + y) * Ws + cx + x;
      if (out)
        for (int ch = 0; ch < 3; ch++) v[3 * k + ch] = s[so * 3 + ch];
      if (lout) l[k] = ls[so];
    } else {
      if (out) {
        const int xs = t[x], a0 = t[W + x], a1 = t[2 * W + x];
        const int ys = t[4 * W + y], b0 = t[4 * W + H + y], b1 = t[4 * W + 2 * H + y];
        const int x1 = min(xs + 1, Ws - 1);
        const int y0 = min(max(ys, 0), Hs - 1), y1 = min(max(ys + 1, 0), Hs - 1);
        const unsigned char *r0 = s + y0 * Ws * 3, *r1 = s + y1 * Ws * 3;
        for (int ch = 0; ch < 3; ch++) {
          const int S0 = r0[xs * 3 + ch] * a0 + r0[x1 * 3 + ch] * a1;
          const int S1 = r1[xs * 3 + ch] * a0 + r1[x1 * 3 + ch] * a1;
          v[3 * k + ch] = (unsigned)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2) & 255u;
        }
      }
      if (lout) l[k] = ls[t[4 * W + 3 * H + y] * Ws + t[3 * W + x]];
    }
  }
  if (out) {
    unsigned char *o = out + ((size_t)b * HW + p0) * 3;
    if (vec && n == 4) {
      unsigned *o4 = reinterpret_cast<unsigned *>(o);
      o4[0] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
      o4[1] = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
      o4[2] = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
    } else {
      for (int k = 0; k < 3 * n; k++) o[k] = (unsigned char)v[k];
    }
  }
  if (lout) {
    TL *lo = lout + (size_t)b * HW + p0;
    for (int k = 0; k < n; k++) lo[k] = l[k];
  }
}

template <typename TL>
void launch_all(const unsigned char *pool, const TL *lpool, int B, int max_hs, int max_ws, int H, int W, int blur,
                const int *desc, const int *tab, unsigned char *out, TL *lout, int *present, unsigned char *ws,
                hipStream_t st) {
  if (blur)
    hipLaunchKernelGGL(blur_ragged_kernel, dim3(dl3_cdiv(max_ws, kTW), dl3_cdiv(max_hs, kTH), B), dim3(256), 0, st, pool,
                       desc, ws);
  if (present) {
    (void)hipMemsetAsync(present, 0, (size_t)B * 8 * sizeof(int), st);
    const int chunks = min(max(dl3_cdiv(max_hs * max_ws, 256 * 64), 1), 64);
    hipLaunchKernelGGL(present_ragged_kernel<TL>, dim3(chunks, B), dim3(256), 0, st, lpool, desc, present);
  }
  if (out || lout) {
    const int vec = (H * W) % 4 == 0 && ((uintptr_t)out & 3) == 0;
    hipLaunchKernelGGL(resize_ragged_kernel<TL>, dim3(dl3_cdiv(H * W, 1024), B), dim3(256), 0, st, pool, blur ? ws : pool, lpool,
                       desc, tab, H, W, out, lout, vec);
  }
}

}  // namespace

extern "C" size_t dl3_cv_resize_workspace_bytes(size_t image_pool_bytes, int blur_any) {
  return blur_any ? (image_pool_bytes + 255) & ~(size_t)255 : 0;
}

extern "C" int dl3_cv_resize(const unsigned char *image_pool, size_t image_pool_bytes, const void *label_pool,
                             int label_dtype, int B, int max_hs, int max_ws, int H, int W, int blur_any, const int *desc,
                             const int *tab, void *images_out, void *labels_out, int *present, void *workspace,
                             size_t workspace_bytes, void *stream) {
  DL3_CHECK_ARG(desc && tab && B > 0, "cv_resize: bad argument");
  DL3_CHECK_ARG(H >= 1 && W >= 1 && max_hs >= 1 && max_ws >= 1, "cv_resize: sizes must be positive, got %dx%d from at most "
                "%dx%d", H, W, max_hs, max_ws);
  DL3_CHECK_ARG((size_t)max_hs * max_ws < ((size_t)1 << 29) && (size_t)H * W < ((size_t)1 << 29) &&
                image_pool_bytes < ((size_t)1 << 31), "cv_resize: image of more than 2^29 pixels or pool of more than 2^31 bytes");
  DL3_CHECK_ARG((image_pool != nullptr) == (images_out != nullptr) && (label_pool != nullptr) == (labels_out != nullptr) &&
                (image_pool || label_pool), "cv_resize: an image pool needs images_out, a label pool labels_out");
  DL3_CHECK_ARG(!present || label_pool, "cv_resize: present is taken from the label pool");
  DL3_UNSUPPORTED(label_pool && label_dtype != DL3_LABEL_U8 && label_dtype != DL3_LABEL_I32,
                  "cv_resize: label maps are uint8 or int32, got dtype code %d", label_dtype);
  const bool blur = blur_any && image_pool;
  const size_t need = dl3_cv_resize_workspace_bytes(image_pool_bytes, blur);
  DL3_CHECK_ARG(!need || (workspace && workspace_bytes >= need), "cv_resize: workspace of %zu bytes, needs %zu",
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (label_pool && label_dtype == DL3_LABEL_I32)
    launch_all<int>(image_pool, (const int *)label_pool, B, max_hs, max_ws, H, W, blur, desc, tab,
                    (unsigned char *)images_out, (int *)labels_out, present, (unsigned char *)workspace, st);
  else
    launch_all<unsigned char>(image_pool, (const unsigned char *)label_pool, B, max_hs, max_ws, H, W, blur, desc, tab,
                              (unsigned char *)images_out, (unsigned char *)labels_out, present,
                              (unsigned char *)workspace, st);
  DL3_LAUNCH_CHECK("cv_resize");
  return DL3_OK;
}
