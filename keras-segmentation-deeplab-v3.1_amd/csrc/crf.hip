// crf.hip — exact mean-field inference of the fully connected CRF that the reference's do_crf configures (reference
// utils.py:74-91; semantics: DESIGN.md §9 [pydensecrf-semantics]).  Three pieces:
//   crf_pair_kernel    one message pass out_i = sum_j exp(-|f_i - f_j|^2 / 2) * q_j over ALL pairs, K never materialised:
//                      row tiles of i per wave, a streamed loop over column tiles of j staged through LDS, the kernel
//                      values on the VALU (differences, packed squares, v_exp_f32), P . Q on v_mfma_f32_32x32x2_f32.
//   crf_gauss_kernel   the sigma = 3 px position kernel, separable: two 1-D passes over the full fp32 support.
//   crf_update_kernel  -U + w_g n_g G + w_b n_b B -> softmax -> Q, the pre-scaled operands n.Q of the next pass, and on
//                      the last iteration Q / energy / argmax.
// fp32 throughout, fixed summation order, no float atomics: two runs are bit-identical.
#include "common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kLP = 32;     // labels are padded to one 32-wide MFMA column block
constexpr int kMaxD = 6;    // feature dimensions (three packed pairs)
constexpr int kRI = 2;      // 32-row blocks per wave: a wave owns 64 rows i, a workgroup 256
constexpr int kRows = 64 * 4;
constexpr int kJS = 128;    // columns j per LDS stage
constexpr int kFlush = 2;   // stages per accumulation chunk (256 columns), see below

// ---------------------------------------------------------------------------------------------------------------------
// The pairwise pass.  grid (ceil(N / 256), B), 256 threads.
//
// Lane l of a wave stands for row i = l & 31 of each of its kRI row blocks and for the column parity h = l >> 5: in step r
// of a 32-column tile it evaluates p = exp(-|f_i - f_j|^2 / 2) for j = 2r + h, which is exactly the A operand of
// v_mfma_f32_32x32x2_f32 (A[i][k = h]); the B operand B[k = h][c = l & 31] is q[j = 2r + h][c], read from the staged
// [j][32] tile at consecutive addresses.  So P goes from the VALU into the matrix pipe without a shuffle or an LDS trip.
// The feature reads of a step are two LDS broadcasts (one address per half-wave).
//
// The kernel value is formed from DIFFERENCES, not from f_i.f_j - |f_i|^2/2 - |f_j|^2/2 on the matrix pipe: with the
// model's scales |f|^2 reaches several hundred, the three-term form cancels to an absolute exponent error of |f|^2 * 2^-24
// — 1e-5 relative on the dominant near-diagonal terms — where the difference form is exact for close features
// (DESIGN.md §9).  Packed fp32 math keeps the squared distance at 7 VALU issues per pair and lane; the exponential
// (crf_exp_neg_half) is 5 more and one v_exp_f32.
//
// Summation: the MFMA accumulator runs over 256 columns, then is folded into a master sum with a compensated (two-sum)
// add and cleared — the rounding error of a 262 144-term fp32 sum stays at that of a 256-term one.
// Columns past N carry q = 0 (and finite features), rows past N are clamped for the loads and not stored.
// ---------------------------------------------------------------------------------------------------------------------
// exp(-s / 2) = 2^(s c), c = -log2(e) / 2 = c_hi + c_lo: the rounding error of the product s c_hi (up to |s c| 2^-24
// relative in the result — several ulp for the pairs that matter, which a lone near neighbour does not average out) is
// recovered with one fma and applied as the first-order factor 1 + ln2 pl; v_exp_f32 itself is good to an ulp.
__device__ __forceinline__ float crf_exp_neg_half(float s) {
  const float c_hi = -0x1.715476p-1f, c_lo = -0x1.4ae0cp-27f;
  const float ph = s * c_hi;
  const float pl = fmaf(s, c_lo, fmaf(s, c_hi, -ph));
  const float e = __builtin_amdgcn_exp2f(ph);
  return fmaf(e, pl * 0.6931471824645996f, e);
}

template <int DP2>
__global__ __launch_bounds__(256) void crf_pair_kernel(const float *__restrict__ feat, int D,
                                                       const float *__restrict__ opnd, float *__restrict__ out, int ldo,
                                                       int Lout, int N) {
  constexpr int FD = 2 * DP2;
  __shared__ __attribute__((aligned(16))) float Fs[2][kJS * FD];
  __shared__ __attribute__((aligned(16))) float Qs[2][kJS * kLP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int b = blockIdx.y;
  const float *fb = feat + (size_t)b * N * D;
  const float *qb = opnd + (size_t)b * N * kLP;
  const int i0 = blockIdx.x * kRows + wave * 64;

  f32x2 fi[kRI][DP2];
#pragma unroll
  for (int rb = 0; rb < kRI; rb++) {
    const int row = min(i0 + rb * 32 + l31, N - 1);
#pragma unroll
    for (int k = 0; k < DP2; k++) {
      fi[rb][k].x = (2 * k < D) ? fb[(size_t)row * D + 2 * k] : 0.f;
      fi[rb][k].y = (2 * k + 1 < D) ? fb[(size_t)row * D + 2 * k + 1] : 0.f;
    }
  }

  constexpr int NF = (kJS * FD + 255) / 256;  // feature elements per thread and stage
  f32x4 qreg[4];
  float freg[NF];
  auto load = [&](int j0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = tid + 256 * u;  // f32x4 index in the [128][32] tile
      const int j = j0 + (e >> 3);
      qreg[u] = j < N ? ld4(qb + (size_t)j * kLP + (e & 7) * 4) : splat4(0.f);
    }
#pragma unroll
    for (int u = 0; u < NF; u++) {
      const int e = tid + 256 * u;
      const int j = j0 + e / FD, d = e % FD;
      freg[u] = (e < kJS * FD && d < D && j < N) ? fb[(size_t)j * D + d] : 0.f;
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; u++) st4(&Qs[buf][(tid + 256 * u) * 4], qreg[u]);
#pragma unroll
    for (int u = 0; u < NF; u++) {
      const int e = tid + 256 * u;
      if (e < kJS * FD) Fs[buf][e] = freg[u];
    }
  };

  f32x16 acc[kRI], sum[kRI], comp[kRI];
#pragma unroll
  for (int rb = 0; rb < kRI; rb++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[rb][r] = sum[rb][r] = comp[rb][r] = 0.f;
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < kRI; rb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float y = acc[rb][r] - comp[rb][r];
        const float t = sum[rb][r] + y;
        comp[rb][r] = (t - sum[rb][r]) - y;
        sum[rb][r] = t;
        acc[rb][r] = 0.f;
      }
  };

  const int S = (N + kJS - 1) / kJS;
  load(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < S; s++) {
    const int buf = s & 1;
    if (s + 1 < S) load((s + 1) * kJS);
    const float *F = Fs[buf], *Q = Qs[buf];
#pragma unroll
    for (int t = 0; t < kJS / 32; t++) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int jj = t * 32 + 2 * r + h;
        f32x2 fj[DP2];
#pragma unroll
        for (int k = 0; k < DP2; k++) fj[k] = *reinterpret_cast<const f32x2 *>(F + jj * FD + 2 * k);
        const float q = Q[jj * kLP + l31];
#pragma unroll
        for (int rb = 0; rb < kRI; rb++) {
          f32x2 d = fi[rb][0] - fj[0];
          f32x2 s2 = d * d;
#pragma unroll
          for (int k = 1; k < DP2; k++) {
            d = fi[rb][k] - fj[k];
            s2 = d * d + s2;
          }
          const float p = crf_exp_neg_half(s2.x + s2.y);
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(p, q, acc[rb], 0, 0, 0);
        }
      }
    }
    if ((s + 1) % kFlush == 0) fold();
    if (s + 1 < S) stash(buf ^ 1);
    __syncthreads();
  }
  fold();

  // C/D register r of lane l: row (r & 3) + 8 (r >> 2) + 4 h of the block, column l & 31
  if (l31 < Lout) {
#pragma unroll
    for (int rb = 0; rb < kRI; rb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = i0 + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < N) out[((size_t)b * N + row) * ldo + l31] = sum[rb][r];
      }
  }
}

// Qin [B][N][L] -> the padded operand [B][N][32] (zeros in columns L..31)
__global__ __launch_bounds__(256) void crf_pack_kernel(const float *__restrict__ q, int L, float *__restrict__ opnd,
                                                       size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int l = (int)(e & (kLP - 1));
  opnd[e] = l < L ? q[(e >> 5) * L + l] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// The position kernel exp(-(dx/sx)^2/2 - (dy/sy)^2/2) = kx(dx) ky(dy): one 1-D pass per axis over src [B][H][W][ld],
// channels 0..C-1, taps -R..R in ascending order (R: the offset beyond which the tap is zero in fp32).
// grid (ceil(H*W*C / 256), B).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kMaxTaps = 2048;
__global__ __launch_bounds__(256) void crf_gauss_kernel(const float *__restrict__ src, float *__restrict__ dst, int H,
                                                        int W, int C, int ld, float sigma, int R, int vertical) {
  __shared__ float wt[kMaxTaps + 1];
  for (int d = threadIdx.x; d <= R; d += 256) {
    const float u = (float)d / sigma;
    wt[d] = expf(-0.5f * (u * u));
  }
  __syncthreads();
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= H * W * C) return;
  const int c = e % C, pix = e / C, x = pix % W, y = pix / W;
  const size_t base = (size_t)blockIdx.y * H * W * ld;
  float a = 0.f;
  if (vertical) {
    const int lo = max(y - R, 0), hi = min(y + R, H - 1);
    for (int yy = lo; yy <= hi; yy++) a += wt[abs(yy - y)] * src[base + ((size_t)yy * W + x) * ld + c];
  } else {
    const int lo = max(x - R, 0), hi = min(x + R, W - 1);
    for (int xx = lo; xx <= hi; xx++) a += wt[abs(xx - x)] * src[base + ((size_t)y * W + xx) * ld + c];
  }
  dst[base + (size_t)pix * ld + c] = a;
}

// features of the appearance kernel (x / sxy, y / sxy, c0 / srgb, c1 / srgb, c2 / srgb), taken about the image centre
// and mid-grey (the kernel only sees differences; smaller magnitudes round finer), and the ones operands of the two
// normaliser passes (column 0 of opb / opg)
__global__ __launch_bounds__(256) void crf_setup_kernel(const unsigned char *__restrict__ im, int H, int W, float sxy,
                                                        float srgb, float *__restrict__ feat, float *__restrict__ opb,
                                                        float *__restrict__ opg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const size_t g = (size_t)blockIdx.y * H * W + i;
  const int x = i % W, y = i / W;
  float *f = feat + g * kMaxD;
  f[0] = ((float)x - (float)(W / 2)) / sxy;
  f[1] = ((float)y - (float)(H / 2)) / sxy;
  f[2] = ((float)im[g * 3 + 0] - 128.f) / srgb;
  f[3] = ((float)im[g * 3 + 1] - 128.f) / srgb;
  f[4] = ((float)im[g * 3 + 2] - 128.f) / srgb;
  f[5] = 0.f;
  const f32x4 one = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < kLP / 4; k++) {
    st4(opb + g * kLP + 4 * k, k ? splat4(0.f) : one);
    st4(opg + g * kLP + 4 * k, k ? splat4(0.f) : one);
  }
}

// n_i = 1 / sqrt(sum_j k_ij + 1e-20) from column 0 of the two ones passes
__global__ __launch_bounds__(256) void crf_norm_kernel(const float *__restrict__ sb, const float *__restrict__ sg,
                                                       float *__restrict__ nb, float *__restrict__ ng, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  nb[i] = 1.f / sqrtf(sb[i * kLP] + 1e-20f);
  ng[i] = 1.f / sqrtf(sg[i * kLP] + 1e-20f);
}

// one pixel per thread: e_l = -U_l (+ wg n_g G_l + wb n_b B_l when msg), Q = softmax(e); writes the operands of the next
// pass and, where asked, Q / e ([B][L][N]) and the argmax (first maximum).  grid (ceil(N / 256), B)
__global__ __launch_bounds__(256) void crf_update_kernel(const float *__restrict__ U, const float *__restrict__ Gm,
                                                         const float *__restrict__ Bm, const float *__restrict__ nb,
                                                         const float *__restrict__ ng, float wg, float wb, int msg,
                                                         int N, int L, float *__restrict__ opb,
                                                         float *__restrict__ opg, float *__restrict__ Qout,
                                                         float *__restrict__ Eout, int *__restrict__ map) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t g = (size_t)blockIdx.y * N + i;
  const float *Ub = U + (size_t)blockIdx.y * L * N + i;
  const float nbi = nb[g], ngi = ng[g];
  float e[kLP];
#pragma unroll
  for (int k = 0; k < kLP / 4; k++) {
    f32x4 gv = splat4(0.f), bv = splat4(0.f);
    if (msg) {
      gv = ld4(Gm + g * kLP + 4 * k);
      bv = ld4(Bm + g * kLP + 4 * k);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int l = 4 * k + c;
      const float u = l < L ? Ub[(size_t)l * N] : 0.f;
      e[l] = msg ? (-u + wg * (ngi * gv[c])) + wb * (nbi * bv[c]) : -u;
    }
  }
  float m = e[0];
  int am = 0;
#pragma unroll
  for (int l = 1; l < kLP; l++)
    if (l < L && e[l] > m) {
      m = e[l];
      am = l;
    }
  float p[kLP], z = 0.f;
#pragma unroll
  for (int l = 0; l < kLP; l++) {
    p[l] = l < L ? expf(e[l] - m) : 0.f;
    z += p[l];
  }
  const float iz = 1.f / z;
#pragma unroll
  for (int l = 0; l < kLP; l++) p[l] *= iz;
  if (opb) {
#pragma unroll
    for (int k = 0; k < kLP / 4; k++) {
      const f32x4 q = {p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]};
      st4(opb + g * kLP + 4 * k, q * nbi);
      st4(opg + g * kLP + 4 * k, q * ngi);
    }
  }
  float *Qb = Qout ? Qout + (size_t)blockIdx.y * L * N + i : nullptr;
  float *Eb = Eout ? Eout + (size_t)blockIdx.y * L * N + i : nullptr;
#pragma unroll
  for (int l = 0; l < kLP; l++)
    if (l < L) {
      if (Qb) Qb[(size_t)l * N] = p[l];
      if (Eb) Eb[(size_t)l * N] = e[l];
    }
  if (map) map[g] = am;
}

// workspace of dl3_crf_inference, in floats per pixel: features, two normalisers, five [32]-wide planes
struct CrfLayout {
  size_t feat, nb, ng, opb, opg, bm, gt, gm, total;
};
CrfLayout crf_layout(size_t BN) {
  CrfLayout l;
  size_t o = 0;
  l.feat = o, o += BN * kMaxD;
  l.nb = o, o += BN;
  l.ng = o, o += BN;
  o = (o + 3) & ~(size_t)3;  // the planes are read with 16-byte loads
  l.opb = o, o += BN * kLP;
  l.opg = o, o += BN * kLP;
  l.bm = o, o += BN * kLP;
  l.gt = o, o += BN * kLP;
  l.gm = o, o += BN * kLP;
  l.total = o * sizeof(float);
  return l;
}

// sizes every index of the kernels above fits in: N * 32 in an int, B * N * 32 elements in the grid of the pack kernel
bool crf_size_ok(long long B, long long N) { return N <= (1ll << 25) && B * N <= (1ll << 30); }

int crf_pair(const float *feat, int D, const float *opnd, float *out, int ldo, int Lout, int B, int N, hipStream_t st) {
  const dim3 grid(dl3_cdiv(N, kRows), B), block(256);
  if (D <= 2)
    hipLaunchKernelGGL(crf_pair_kernel<1>, grid, block, 0, st, feat, D, opnd, out, ldo, Lout, N);
  else if (D <= 4)
    hipLaunchKernelGGL(crf_pair_kernel<2>, grid, block, 0, st, feat, D, opnd, out, ldo, Lout, N);
  else
    hipLaunchKernelGGL(crf_pair_kernel<3>, grid, block, 0, st, feat, D, opnd, out, ldo, Lout, N);
  DL3_LAUNCH_CHECK("crf_pair_kernel");
  return DL3_OK;
}

// offset beyond which exp(-(d / sigma)^2 / 2) is below the smallest normal float (2^-126): d > sigma sqrt(2 * 126 ln 2)
int crf_gauss_radius(float sigma) { return (int)ceilf(sigma * 13.22f); }

}  // namespace

extern "C" size_t dl3_crf_workspace_bytes(int B, int H, int W, int L) {
  if (B <= 0 || H <= 0 || W <= 0 || L <= 0 || L > kLP) return 0;
  return crf_layout((size_t)B * H * W).total;
}

extern "C" int dl3_crf_message(const float *feat, int D, const float *Qin, int B, int N, int L, float *out, void *ws,
                               size_t ws_bytes, void *stream) {
  DL3_CHECK_ARG(feat && Qin && out, "crf_message: null pointer");
  DL3_CHECK_ARG(B > 0 && N > 0 && L > 0 && D > 0, "crf_message: B, N, L, D must be positive, got %d, %d, %d, %d", B, N,
                L, D);
  DL3_CHECK_ARG(crf_size_ok(B, N), "crf_message: B = %d, N = %d is too large", B, N);
  DL3_UNSUPPORTED(L > kLP, "crf_message: at most %d labels, got %d", kLP, L);
  DL3_UNSUPPORTED(D > kMaxD, "crf_message: at most %d feature dimensions, got %d", kMaxD, D);
  const size_t need = (size_t)B * N * kLP * sizeof(float);
  if (!ws || ws_bytes < need) {
    dl3_set_error("crf_message: workspace of %zu bytes, needs %zu", ws ? ws_bytes : (size_t)0, need);
    return DL3_EWORKSPACE;
  }
  DL3_CHECK_ARG(((uintptr_t)ws & 15) == 0, "crf_message: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float *opnd = (float *)ws;
  const size_t total = (size_t)B * N * kLP;
  hipLaunchKernelGGL(crf_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Qin, L, opnd, total);
  DL3_LAUNCH_CHECK("crf_pack_kernel");
  return crf_pair(feat, D, opnd, out, L, L, B, N, st);
}

extern "C" int dl3_crf_inference(const unsigned char *im, const float *U, int B, int H, int W, int L,
                                 const float *params, int iters, float *Q, float *energy, int *map, void *ws,
                                 size_t ws_bytes, void *stream) {
  DL3_CHECK_ARG(im && U && params, "crf_inference: null pointer (image, unary or parameters)");
  DL3_CHECK_ARG(B > 0 && H > 0 && W > 0 && L > 0 && iters >= 0,
                "crf_inference: B, H, W, L must be positive and iters >= 0, got %d, %d, %d, %d, %d", B, H, W, L, iters);
  DL3_CHECK_ARG(crf_size_ok(B, (long long)H * W), "crf_inference: B = %d, H * W = %lld is too large", B,
                (long long)H * W);
  DL3_UNSUPPORTED(L > kLP, "crf_inference: at most %d labels, got %d", kLP, L);
  const float sx = params[0], sy = params[1], wg = params[2], sxy = params[3], srgb = params[4], wb = params[5];
  DL3_CHECK_ARG(sx > 0.f && sy > 0.f && sxy > 0.f && srgb > 0.f, "crf_inference: kernel widths must be positive");
  const int Rx = min(crf_gauss_radius(sx), W - 1), Ry = min(crf_gauss_radius(sy), H - 1);
  DL3_UNSUPPORTED(Rx > kMaxTaps || Ry > kMaxTaps, "crf_inference: position kernel wider than %d taps", kMaxTaps);
  const int N = H * W;
  const CrfLayout lay = crf_layout((size_t)B * N);
  if (!ws || ws_bytes < lay.total) {
    dl3_set_error("crf_inference: workspace of %zu bytes, needs %zu", ws ? ws_bytes : (size_t)0, lay.total);
    return DL3_EWORKSPACE;
  }
  DL3_CHECK_ARG(((uintptr_t)ws & 15) == 0, "crf_inference: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float *w = (float *)ws;
  float *feat = w + lay.feat, *nb = w + lay.nb, *ng = w + lay.ng, *opb = w + lay.opb, *opg = w + lay.opg;
  float *bm = w + lay.bm, *gt = w + lay.gt, *gm = w + lay.gm;
  const dim3 gpix(dl3_cdiv(N, 256), B), block(256);

  auto gauss = [&](int C) -> int {
    const dim3 g(dl3_cdiv(N * C, 256), B);
    hipLaunchKernelGGL(crf_gauss_kernel, g, block, 0, st, (const float *)opg, gt, H, W, C, kLP, sx, Rx, 0);
    hipLaunchKernelGGL(crf_gauss_kernel, g, block, 0, st, (const float *)gt, gm, H, W, C, kLP, sy, Ry, 1);
    DL3_LAUNCH_CHECK("crf_gauss_kernel");
    return DL3_OK;
  };

  // normalisers: both kernels applied to ones
  hipLaunchKernelGGL(crf_setup_kernel, gpix, block, 0, st, im, H, W, sxy, srgb, feat, opb, opg);
  DL3_LAUNCH_CHECK("crf_setup_kernel");
  int rc = crf_pair(feat, kMaxD, opb, bm, kLP, 1, B, N, st);
  if (rc) return rc;
  if ((rc = gauss(1))) return rc;
  const size_t BN = (size_t)B * N;
  hipLaunchKernelGGL(crf_norm_kernel, dim3((unsigned)((BN + 255) / 256)), block, 0, st, (const float *)bm,
                     (const float *)gm, nb, ng, BN);
  DL3_LAUNCH_CHECK("crf_norm_kernel");

  // Q0 = softmax(-U), then iters parallel updates
  const bool last0 = iters == 0;
  hipLaunchKernelGGL(crf_update_kernel, gpix, block, 0, st, U, (const float *)gm, (const float *)bm, (const float *)nb,
                     (const float *)ng, wg, wb, 0, N, L, opb, opg, last0 ? Q : nullptr, last0 ? energy : nullptr,
                     last0 ? map : nullptr);
  DL3_LAUNCH_CHECK("crf_update_kernel");
  for (int it = 0; it < iters; it++) {
    if ((rc = crf_pair(feat, kMaxD, opb, bm, kLP, L, B, N, st))) return rc;
    if ((rc = gauss(L))) return rc;
    const bool last = it + 1 == iters;
    hipLaunchKernelGGL(crf_update_kernel, gpix, block, 0, st, U, (const float *)gm, (const float *)bm,
                       (const float *)nb, (const float *)ng, wg, wb, 1, N, L, last ? (float *)nullptr : opb,
                       last ? (float *)nullptr : opg, last ? Q : nullptr, last ? energy : nullptr,
                       last ? map : nullptr);
    DL3_LAUNCH_CHECK("crf_update_kernel");
  }
  return DL3_OK;
}
