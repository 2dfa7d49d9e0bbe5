// misc.hip — the tail of the DeepLabV3+ path: TF1-legacy bilinear resize (deeplabv3p.py:382,:418,
// :439; utils.py:190), Subpixel phase shift (subpixel.py:77-88), softmax (deeplabv3p.py:441,:444), argmax and the
// count of non-zero sample weights (the training loss itself: losstail.hip).
// All HBM-bound, one pass each; backward kernels are gather-form (no atomics, deterministic).
#include "tailmath.h"

namespace {

// (the TF1-legacy bilinear weights and lerps: tailmath.h; the resize kernels take the fused weight .w)
__global__ __launch_bounds__(256) void resize_fwd_kernel(const float *__restrict__ x, int ldx,
                                                         const float *__restrict__ sc,
                                                         const float *__restrict__ sh, int act,
                                                         float *__restrict__ y, int ldy, int N, int Hi, int Wi,
                                                         int Ho, int Wo, int C, float sy, float sx) {
  // grid.y = output row (n, oy); threads cover (ox, c) of that row: no 64-bit divisions per element
  const int n = blockIdx.y / Ho, oy = blockIdx.y - n * Ho;
  const Lerp ly = tf1_lerp(oy, sy, Hi);
  const float *b = x + (size_t)n * Hi * Wi * ldx;
  const float *r0 = b + (size_t)ly.lo * Wi * ldx, *r1 = b + (size_t)ly.hi * Wi * ldx;
  float *yo = y + (size_t)blockIdx.y * Wo * ldy;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < Wo * C; i += gridDim.x * 256) {
    const int ox = i / C, c = i - ox * C;
    const Lerp lx = tf1_lerp(ox, sx, Wi);
    float es = 1.f, et = 0.f;
    if (sc) { es = sc[c]; et = sh[c]; }
    const float tl = dl3_act(es * r0[(size_t)lx.lo * ldx + c] + et, act);
    const float tr = dl3_act(es * r0[(size_t)lx.hi * ldx + c] + et, act);
    const float bl = dl3_act(es * r1[(size_t)lx.lo * ldx + c] + et, act);
    const float br = dl3_act(es * r1[(size_t)lx.hi * ldx + c] + et, act);
    yo[(size_t)ox * ldy + c] = bilerp(tl, tr, bl, br, lx.w, ly.w);
  }
}

// gather form of the transpose: input pixel (iy,ix) collects from every output pixel whose
// lower/upper source index hits it; weights are recomputed with the forward formula.
__global__ __launch_bounds__(256) void resize_bwd_kernel(const float *__restrict__ dy, int lddy,
                                                         float *__restrict__ dx, int lddx, int N, int Hi, int Wi,
                                                         int Ho, int Wo, int C, float sy, float sx, int accumulate) {
  // grid.y = input row (n, iy); threads cover (ix, c)
  const int n = blockIdx.y / Hi, iy = blockIdx.y - n * Hi;
  // candidate output rows: those with floor(oy*sy) in {iy-1, iy} (+1 slack each side for rounding)
  int oy0 = (int)floorf((float)(iy - 1) / sy) - 1, oy1 = (int)ceilf((float)(iy + 1) / sy) + 1;
  oy0 = max(oy0, 0);
  oy1 = min(oy1, Ho - 1);
  const float *dyn = dy + (size_t)n * Ho * Wo * lddy;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < Wi * C; i += gridDim.x * 256) {
    const int ix = i / C, c = i - ix * C;
    int ox0 = (int)floorf((float)(ix - 1) / sx) - 1, ox1 = (int)ceilf((float)(ix + 1) / sx) + 1;
    ox0 = max(ox0, 0);
    ox1 = min(ox1, Wo - 1);
    float acc = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy) {
      const Lerp ly = tf1_lerp(oy, sy, Hi);
      const float wy = (ly.lo == iy ? 1.f - ly.w : 0.f) + (ly.hi == iy ? ly.w : 0.f);
      if (wy == 0.f) continue;
      float racc = 0.f;
      const float *row = dyn + (size_t)oy * Wo * lddy + c;
      for (int ox = ox0; ox <= ox1; ++ox) {
        const Lerp lx = tf1_lerp(ox, sx, Wi);
        const float wx = (lx.lo == ix ? 1.f - lx.w : 0.f) + (lx.hi == ix ? lx.w : 0.f);
        racc += wx * row[(size_t)ox * lddy];
      }
      acc += wy * racc;
    }
    float *o = dx + ((size_t)blockIdx.y * Wi + ix) * lddx + c;
    *o = accumulate ? (*o + acc) : acc;
  }
}

// separable form of the same transpose: pass X folds the output columns of every output row onto the input columns
// (tmp [N,Ho,Wi,C]), pass Y folds the output rows onto the input rows.  Each dy element is read once instead of four
// times and the per-element loop is 2f+3 long instead of (2f+3)^2.
__global__ __launch_bounds__(256) void resize_bwd_x_kernel(const float *__restrict__ dy, int lddy,
                                                           float *__restrict__ tmp, int Wi, int Wo, int C, float sx) {
  // grid.y = output row (n, oy); threads cover (ix, c)
  const float *row = dy + (size_t)blockIdx.y * Wo * lddy;
  float *trow = tmp + (size_t)blockIdx.y * Wi * C;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < Wi * C; i += gridDim.x * 256) {
    const int ix = i / C, c = i - ix * C;
    int ox0 = (int)floorf((float)(ix - 1) / sx) - 1, ox1 = (int)ceilf((float)(ix + 1) / sx) + 1;
    ox0 = max(ox0, 0);
    ox1 = min(ox1, Wo - 1);
    float acc = 0.f;
    for (int ox = ox0; ox <= ox1; ++ox) {
      const Lerp lx = tf1_lerp(ox, sx, Wi);
      const float wx = (lx.lo == ix ? 1.f - lx.w : 0.f) + (lx.hi == ix ? lx.w : 0.f);
      acc += wx * row[(size_t)ox * lddy + c];
    }
    trow[i] = acc;
  }
}
__global__ __launch_bounds__(256) void resize_bwd_y_kernel(const float *__restrict__ tmp, float *__restrict__ dx,
                                                           int lddx, int Hi, int Wi, int Ho, int C, float sy,
                                                           int accumulate) {
  // grid.y = input row (n, iy); threads cover (ix, c)
  const int n = blockIdx.y / Hi, iy = blockIdx.y - n * Hi;
  int oy0 = (int)floorf((float)(iy - 1) / sy) - 1, oy1 = (int)ceilf((float)(iy + 1) / sy) + 1;
  oy0 = max(oy0, 0);
  oy1 = min(oy1, Ho - 1);
  const float *tn = tmp + (size_t)n * Ho * Wi * C;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < Wi * C; i += gridDim.x * 256) {
    const int ix = i / C, c = i - ix * C;
    float acc = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy) {
      const Lerp ly = tf1_lerp(oy, sy, Hi);
      const float wy = (ly.lo == iy ? 1.f - ly.w : 0.f) + (ly.hi == iy ? ly.w : 0.f);
      acc += wy * tn[(size_t)oy * Wi * C + i];
    }
    float *o = dx + ((size_t)blockIdx.y * Wi + ix) * lddx + c;
    *o = accumulate ? (*o + acc) : acc;
  }
}

// out[n, ia*r+q, ib*r+p, ch] = in[n, ia, ib, ch*r*r + p*r + q]   (subpixel.py:81-87)
// Generic fallback: one thread per element of the shuffled tensor (its reads are r*r floats apart: ~1 TB/s).
__global__ __launch_bounds__(256) void phase_shift_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                          int N, int H, int W, int Cout, int r, int inverse) {
  const long total = (long)N * H * W * Cout * r * r;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    // i indexes the shuffled tensor [N, H*r, W*r, Cout]
    const int ch = (int)(i % Cout);
    long p = i / Cout;
    const int X = (int)(p % ((long)W * r));
    p /= (long)W * r;
    const int Y = (int)(p % ((long)H * r));
    const int n = (int)(p / ((long)H * r));
    const int ia = Y / r, q = Y % r, ib = X / r, pp = X % r;
    const size_t j = (((size_t)n * H + ia) * W + ib) * ((size_t)Cout * r * r) + (size_t)ch * r * r + pp * r + q;
    if (inverse) out[j] = in[i];
    else out[i] = in[j];
  }
}

// The same permutation with both sides coalesced (round 3; the Subpixel head moved 2.8 GB each way at 0.98 TB/s: 12 ms of
// a 135 ms step).  A workgroup owns PB consecutive pixels (ib0 .. ib0+PB-1) of one row (n, ia) of the UNshuffled
// tensor: PB * Cout*r*r contiguous floats on that side; on the shuffled side they are r runs (q = 0..r-1, image row
// ia*r+q) of PB*r*Cout contiguous floats.  The tile goes through LDS, element (pixel, ch, pq) at
// pixel*Cout*(r*r+1) + ch*(r*r+1) + pq: the channel stride is odd, so the transposing access (consecutive lanes =
// consecutive ch) touches distinct banks.
__global__ __launch_bounds__(256) void phase_shift_lds_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                              int H, int W, int Cout, int r, int PB, int inverse) {
  extern __shared__ float tile[];
  const int rr = r * r, P = Cout * rr, LP = Cout * (rr + 1);
  const int wblocks = (W + PB - 1) / PB;
  const int ib0 = (blockIdx.x % wblocks) * PB;
  const long row = blockIdx.x / wblocks;  // n * H + ia
  const int ia = (int)(row % H);
  const long n = row / H;
  const int pb = min(PB, W - ib0);
  const float *flat_src = inverse ? nullptr : in + ((size_t)row * W + ib0) * P;    // unshuffled side, contiguous
  float *flat_dst = inverse ? out + ((size_t)row * W + ib0) * P : nullptr;
  const int run = pb * r * Cout;                                                    // one shuffled-side run
  const size_t run0 = (((size_t)n * H * r + (size_t)ia * r) * ((size_t)W * r) + (size_t)ib0 * r) * Cout;  // q = 0
  const size_t run_stride = (size_t)W * r * Cout;                                   // next image row (q + 1)
  if (!inverse) {
    for (int t = threadIdx.x; t < pb * P; t += 256) {
      const int px = t / P, e = t % P;
      tile[px * LP + (e / rr) * (rr + 1) + e % rr] = flat_src[t];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < r * run; t += 256) {
      const int q = t / run, u = t % run;
      const int ch = u % Cout, xx = u / Cout;  // xx = ib_local * r + p
      out[run0 + (size_t)q * run_stride + u] = tile[(xx / r) * LP + ch * (rr + 1) + (xx % r) * r + q];
    }
  } else {
    for (int t = threadIdx.x; t < r * run; t += 256) {
      const int q = t / run, u = t % run;
      const int ch = u % Cout, xx = u / Cout;
      tile[(xx / r) * LP + ch * (rr + 1) + (xx % r) * r + q] = in[run0 + (size_t)q * run_stride + u];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < pb * P; t += 256) {
      const int px = t / P, e = t % P;
      flat_dst[t] = tile[px * LP + (e / rr) * (rr + 1) + e % rr];
    }
  }
}

// k x k taps of T(x) side by side (Subpixel with kernel_size > 1): one thread per (output pixel, tap, channel)
__global__ __launch_bounds__(256) void conv_taps_fwd_kernel(const float *__restrict__ x, int ldx,
                                                            const float *__restrict__ sc, const float *__restrict__ sh,
                                                            int act, float *__restrict__ cols, int N, int H, int W, int C,
                                                            int k, int pt, int pl, int Ho, int Wo) {
  const long total = (long)N * Ho * Wo * k * k * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long p = i / C;
    const int t = (int)(p % (k * k));
    p /= k * k;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho), n = (int)(p / Ho);
    const int iy = oy - pt + t / k, ix = ox - pl + t % k;
    float v = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      v = x[(((size_t)n * H + iy) * W + ix) * ldx + c];
      if (sc) v = sc[c] * v + sh[c];
      v = dl3_act(v, act);
    }
    cols[i] = v;
  }
}

__global__ __launch_bounds__(256) void conv_taps_bwd_kernel(const float *__restrict__ dcols, float *__restrict__ dx,
                                                            int N, int H, int W, int C, int k, int pt, int pl, int Ho,
                                                            int Wo) {
  const long total = (long)N * H * W * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long p = i / C;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H), n = (int)(p / H);
    float s = 0.f;
    for (int t = 0; t < k * k; t++) {  // fixed tap order: deterministic
      const int oy = iy + pt - t / k, ox = ix + pl - t % k;
      if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo)
        s += dcols[((((size_t)n * Ho + oy) * Wo + ox) * (k * k) + t) * C + c];
    }
    dx[i] = s;
  }
}

__global__ __launch_bounds__(256) void softmax_kernel(const float *__restrict__ x, float *__restrict__ p, long M,
                                                      int C) {
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const float *r = x + (size_t)m * C;
    float mx = r[0];
    for (int c = 1; c < C; c++) mx = fmaxf(mx, r[c]);
    float s = 0.f;
    for (int c = 0; c < C; c++) s += expf(r[c] - mx);
    const float inv = 1.f / s;
    for (int c = 0; c < C; c++) p[(size_t)m * C + c] = expf(r[c] - mx) * inv;
  }
}

__global__ __launch_bounds__(256) void argmax_kernel(const float *__restrict__ x, int *__restrict__ out, long M,
                                                     int C) {
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const float *r = x + (size_t)m * C;
    float mx = r[0];
    int am = 0;
    for (int c = 1; c < C; c++)
      if (r[c] > mx) { mx = r[c]; am = c; }
    out[m] = am;
  }
}

__global__ __launch_bounds__(256) void count_nz_kernel(const float *__restrict__ w, long M, unsigned int *cnt) {
  __shared__ unsigned int red[4];
  unsigned int c = 0;
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) c += (w[m] != 0.f);
  // integer adds commute: the atomic result is order-independent (deterministic)
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(cnt, red[0] + red[1] + red[2] + red[3]);
}
__global__ void count_to_float_kernel(unsigned int *cnt) {
  const unsigned int v = *cnt;
  *reinterpret_cast<float *>(cnt) = (float)v;
}

inline int ew_blocks(size_t n) { return dl3_blocks((long)n, 256, 8192); }

}  // namespace

extern "C" int dl3_resize_bilinear_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift,
                                       int in_act, float *y, int ldy, int N, int Hi, int Wi, int Ho, int Wo, int C,
                                       void *stream) {
  DL3_CHECK_ARG(x && y && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0, "resize_fwd: bad argument");
  DL3_CHECK_ARG(ldx >= C && ldy >= C, "resize_fwd: leading dimension too small");
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "resize_fwd: scale/shift must come together");
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  DL3_UNSUPPORTED((long)N * Ho > 2147483647L, "resize_fwd: too many rows");
  int gx = dl3_cdiv(Wo * C, 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(resize_fwd_kernel, dim3(gx, N * Ho), dim3(256), 0, (hipStream_t)stream, x, ldx, in_scale,
                     in_shift, in_act, y, ldy, N, Hi, Wi, Ho, Wo, C, sy, sx);
  DL3_LAUNCH_CHECK("resize_fwd");
  return DL3_OK;
}

extern "C" size_t dl3_resize_bilinear_bwd_workspace(int N, int Hi, int Wi, int Ho, int Wo, int C) {
  (void)Hi; (void)Wo;
  return (size_t)N * Ho * Wi * C * sizeof(float);
}

extern "C" int dl3_resize_bilinear_bwd(const float *dy, int lddy, float *dx, int lddx, int N, int Hi, int Wi,
                                       int Ho, int Wo, int C, int accumulate, void *workspace,
                                       size_t workspace_bytes, void *stream) {
  DL3_CHECK_ARG(dy && dx && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0, "resize_bwd: bad argument");
  DL3_CHECK_ARG(lddy >= C && lddx >= C, "resize_bwd: leading dimension too small");
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  if (workspace && workspace_bytes >= dl3_resize_bilinear_bwd_workspace(N, Hi, Wi, Ho, Wo, C)) {
    int gx = dl3_cdiv(Wi * C, 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(resize_bwd_x_kernel, dim3(gx, N * Ho), dim3(256), 0, (hipStream_t)stream, dy, lddy,
                       (float *)workspace, Wi, Wo, C, sx);
    hipLaunchKernelGGL(resize_bwd_y_kernel, dim3(gx, N * Hi), dim3(256), 0, (hipStream_t)stream,
                       (const float *)workspace, dx, lddx, Hi, Wi, Ho, C, sy, accumulate);
    DL3_LAUNCH_CHECK("resize_bwd(separable)");
    return DL3_OK;
  }
  int gx = dl3_cdiv(Wi * C, 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(resize_bwd_kernel, dim3(gx, N * Hi), dim3(256), 0, (hipStream_t)stream, dy, lddy, dx, lddx, N,
                     Hi, Wi, Ho, Wo, C, sy, sx, accumulate);
  DL3_LAUNCH_CHECK("resize_bwd");
  return DL3_OK;
}

extern "C" int dl3_resize_bilinear_bwd_rows(const float *xfold, float *dx, int lddx, int N, int Hi, int Wi, int Ho,
                                            int C, int accumulate, void *stream) {
  DL3_CHECK_ARG(xfold && dx && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && C > 0, "resize_bwd_rows: bad argument");
  DL3_CHECK_ARG(lddx >= C, "resize_bwd_rows: leading dimension too small");
  const float sy = (float)Hi / (float)Ho;
  int gx = dl3_cdiv(Wi * C, 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(resize_bwd_y_kernel, dim3(gx, N * Hi), dim3(256), 0, (hipStream_t)stream, xfold, dx, lddx, Hi, Wi,
                     Ho, C, sy, accumulate);
  DL3_LAUNCH_CHECK("resize_bwd_rows");
  return DL3_OK;
}

extern "C" int dl3_phase_shift(const float *in, float *out, int N, int H, int W, int Cout, int r, int inverse,
                               void *stream) {
  DL3_CHECK_ARG(in && out && N > 0 && H > 0 && W > 0 && Cout > 0 && r > 0, "phase_shift: bad argument");
  const size_t per_px = (size_t)Cout * (r * r + 1) * sizeof(float);
  const int PB = subpixel_tile_pixels(W, Cout, r, 8);
  const long blocks = (long)N * H * dl3_cdiv(W, PB > 0 ? PB : 1);
  if (PB >= 1 && blocks < (1L << 31)) {
    hipLaunchKernelGGL(phase_shift_lds_kernel, dim3((unsigned)blocks), dim3(256), PB * per_px, (hipStream_t)stream, in,
                       out, H, W, Cout, r, PB, inverse);
  } else {
    hipLaunchKernelGGL(phase_shift_kernel, dim3(ew_blocks((size_t)N * H * W * Cout * r * r)), dim3(256), 0,
                       (hipStream_t)stream, in, out, N, H, W, Cout, r, inverse);
  }
  DL3_LAUNCH_CHECK("phase_shift");
  return DL3_OK;
}

extern "C" int dl3_conv_taps_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                                 float *cols, int N, int H, int W, int C, int k, int pad_t, int pad_l, int Ho, int Wo,
                                 void *stream) {
  DL3_CHECK_ARG(x && cols && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && Ho > 0 && Wo > 0 && ldx >= C,
                "conv_taps_fwd: bad argument");
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "conv_taps_fwd: scale/shift must come together");
  DL3_CHECK_ARG(pad_t >= 0 && pad_l >= 0 && Ho - 1 - pad_t + k - 1 < H + k && Wo - 1 - pad_l + k - 1 < W + k,
                "conv_taps_fwd: geometry out of range");
  hipLaunchKernelGGL(conv_taps_fwd_kernel, dim3(ew_blocks((size_t)N * Ho * Wo * k * k * C)), dim3(256), 0,
                     (hipStream_t)stream, x, ldx, in_scale, in_shift, in_act, cols, N, H, W, C, k, pad_t, pad_l, Ho, Wo);
  DL3_LAUNCH_CHECK("conv_taps_fwd");
  return DL3_OK;
}

extern "C" int dl3_conv_taps_bwd(const float *dcols, float *dx, int N, int H, int W, int C, int k, int pad_t, int pad_l,
                                 int Ho, int Wo, void *stream) {
  DL3_CHECK_ARG(dcols && dx && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && Ho > 0 && Wo > 0 && pad_t >= 0 && pad_l >= 0,
                "conv_taps_bwd: bad argument");
  hipLaunchKernelGGL(conv_taps_bwd_kernel, dim3(ew_blocks((size_t)N * H * W * C)), dim3(256), 0, (hipStream_t)stream,
                     dcols, dx, N, H, W, C, k, pad_t, pad_l, Ho, Wo);
  DL3_LAUNCH_CHECK("conv_taps_bwd");
  return DL3_OK;
}

extern "C" int dl3_softmax_fwd(const float *logits, float *probs, int M, int C, void *stream) {
  DL3_CHECK_ARG(logits && probs && M > 0 && C > 0, "softmax_fwd: bad argument");
  hipLaunchKernelGGL(softmax_kernel, dim3(ew_blocks((size_t)M)), dim3(256), 0, (hipStream_t)stream, logits, probs,
                     (long)M, C);
  DL3_LAUNCH_CHECK("softmax_fwd");
  return DL3_OK;
}

extern "C" int dl3_argmax(const float *x, int *out, int M, int C, void *stream) {
  DL3_CHECK_ARG(x && out && M > 0 && C > 0, "argmax: bad argument");
  hipLaunchKernelGGL(argmax_kernel, dim3(ew_blocks((size_t)M)), dim3(256), 0, (hipStream_t)stream, x, out, (long)M,
                     C);
  DL3_LAUNCH_CHECK("argmax");
  return DL3_OK;
}

extern "C" int dl3_count_nonzero(const float *w, int M, float *out, void *stream) {
  DL3_CHECK_ARG(w && out && M > 0, "count_nonzero: bad argument");
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(out, 0, sizeof(float), st);
  int blocks = ew_blocks((size_t)M);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(count_nz_kernel, dim3(blocks), dim3(256), 0, st, w, (long)M, (unsigned int *)out);
  hipLaunchKernelGGL(count_to_float_kernel, dim3(1), dim3(1), 0, st, (unsigned int *)out);
  DL3_LAUNCH_CHECK("count_nonzero");
  return DL3_OK;
}
