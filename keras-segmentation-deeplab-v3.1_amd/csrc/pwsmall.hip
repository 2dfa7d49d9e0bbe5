// pwsmall.hip — the 1x1 GEMMs over few rows: the K-split kernel (PW_KSPLIT), the per-image rows kernel in double (pwgemm.hip)
#include "common.h"
#include "pwargs.h"
namespace {
using pw::GemmArgs;

// ---- small batches (round 5): 32 rows x all N <= 160 columns per workgroup, the REDUCTION split over the four
// waves.  At B = 2 - 4 the 64x64 maps are 8 192 - 16 384 rows: the 32-row stream kernels put their four waves side by side
// along N (64 columns each), which pads a 160-wide output to 256 columns (1.6x the MFMAs) and a 96-wide one to 128, on a
// launch that is one workgroup per CU walking K/16 barrier-separated K-tiles.  Here every wave owns whole 32 x (32 TN)
// accumulators and walks every fourth K-tile on its own — weights through a wave-private double buffer in LDS, no barrier
// in the loop —, the four partial accumulators meet in LDS once ((w0 + w1) + (w2 + w3), fixed order) and column block j is
// finished (bias, mask, addend, store, BatchNorm sums) by wave j % 4.  One partial-sum row per workgroup (= 32-row tile).
template <int TN, bool TWO>
__global__ __launch_bounds__(256) void pw_ksplit32_kernel(GemmArgs P) {
  constexpr int KT = 16, BN = 32 * TN, BQ = KT * BN;
  constexpr int NB = (BQ / 4 + 63) / 64;             // float4 weight loads per LANE: one wave loads a whole K-tile
  constexpr int KCS = DL3_STREAM_KMAX + KT;
  __shared__ float cf[(TWO ? 3 : 2) * KCS];
  __shared__ __attribute__((aligned(16))) float wbuf[4][2 * BQ];  // per wave: two weight tiles; later its TN accumulators
  static_assert(2 * BQ == 1024 * TN, "the reduction reuses the weight buffers");
  // gfx950 only: TN = 5 holds 80 KB of weight tiles + up to 24 KB of coefficients in static LDS — inside the 160 KB of a
  // CDNA4 CU, beyond the 64 KB of gfx90a / gfx942 (this library is built for gfx950 alone: csrc/Makefile)
  static_assert(sizeof(float) * ((TWO ? 3 : 2) * KCS + 4 * 2 * BQ) <= 160 * 1024, "K-split kernel: static LDS exceeds a gfx950 CU's 160 KB");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int ktiles = (P.K + KT - 1) / KT;
  const bool xform = (P.ka != nullptr);
  for (int i = tid; i < ktiles * KT; i += 256) {
    const bool in = i < P.K;
    const int k = min(i, P.K - 1);
    cf[i] = in ? (xform ? P.ka[k] : 1.f) : 0.f;
    cf[KCS + i] = (in && xform) ? P.kc[k] : 0.f;
    if (TWO) cf[2 * KCS + i] = in ? P.kb[k] : 0.f;
  }
  __syncthreads();
  const int m0 = blockIdx.x * 32;
  const int row = min(m0 + l31, P.M - 1);
  const float *ar = P.a + (size_t)row * P.lda;
  const float *ar2 = TWO ? P.a2 + (size_t)row * P.lda2 : nullptr;
  float *wb = wbuf[wave];
  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
  f32x4 an[2], an2[2], rb[NB];
  float ac[8];
  auto request = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int kc = min(kt * KT + 8 * lhi + 4 * j, P.K - 4);
      an[j] = ld4(ar + kc);
      if (TWO) an2[j] = ld4(ar2 + kc);
    }
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int idx = lane + 64 * i;
      if (NB * 64 == BQ / 4 || idx < BQ / 4) {
        const int kk = idx / (BN / 4), nq = idx % (BN / 4);
        const int krow = min(kt * KT + kk, P.K - 1), col = min(nq * 4, P.N - 4);
        rb[i] = ld4(P.b + (size_t)krow * P.ldb + col);
      }
    }
  };
  auto stash = [&](int kt, float *Bs) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int idx = lane + 64 * i;
      if (NB * 64 == BQ / 4 || idx < BQ / 4) st4(&Bs[(idx / (BN / 4)) * BN + (idx % (BN / 4)) * 4], rb[i]);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int k = kt * KT + 8 * lhi + 4 * j;
      f32x4 v = ld4(cf + k) * an[j] + ld4(cf + KCS + k);
      if (TWO) v += ld4(cf + 2 * KCS + k) * an2[j];
      v = dl3_act4(v, P.a_act);
      ac[4 * j + 0] = v.x; ac[4 * j + 1] = v.y; ac[4 * j + 2] = v.z; ac[4 * j + 3] = v.w;
    }
  };
  int kt = wave, buf = 0;
  if (kt < ktiles) {
    request(kt);
    stash(kt, wb);
  }
  for (; kt < ktiles; kt += 4) {
    const bool more = kt + 4 < ktiles;
    if (more) request(kt + 4);
    __builtin_amdgcn_wave_barrier();   // (a wave's LDS operations complete in order: the tile it stashed is there)
    const float *Bs = wb + buf * BQ;
    float av[8];
#pragma unroll
    for (int s_ = 0; s_ < 8; s_++) av[s_] = ac[s_];
#pragma unroll
    for (int s_ = 0; s_ < 8; s_++) {
#pragma unroll
      for (int j = 0; j < TN; j++)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s_], Bs[(8 * lhi + s_) * BN + j * 32 + l31], acc[j], 0, 0, 0);
    }
    if (more) stash(kt + 4, wb + (buf ^ 1) * BQ);
    buf ^= 1;
  }
  // the four partial accumulators meet: wave w parks its TN blocks in its own buffer, block j is summed by wave j % 4
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TN; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) wb[(j * 16 + r) * 64 + lane] = acc[j][r];
  __syncthreads();
  const bool mode2 = P.stat_mode == 2;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    if ((j & 3) != wave) continue;     // (wave-uniform)
    float v16[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int o = (j * 16 + r) * 64 + lane;
      v16[r] = (wbuf[0][o] + wbuf[1][o]) + (wbuf[2][o] + wbuf[3][o]);
    }
    const int col = j * 32 + l31;
    const bool cok = col < P.N;
    const int colc = min(col, P.N - 1);
    float bias = 0.f, es = 1.f, et = 0.f, mu = 0.f, is = 0.f;
    if (P.bias) bias = P.bias[colc];
    if (P.ep_x && P.ep_scale) { es = P.ep_scale[colc]; et = P.ep_shift[colc]; }
    if (mode2) { mu = P.ep_mean[colc]; is = P.ep_invstd[colc]; }
    const int rbase = m0 + 4 * lhi;
    float xr_[16], ad[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int rw = min(rbase + (r & 3) + 8 * (r >> 2), P.M - 1);
      xr_[r] = P.ep_x ? P.ep_x[(size_t)rw * P.ld_epx + colc] : 0.f;
      const int arow_ = (P.add_div > 1) ? rw / P.add_div : rw;
      ad[r] = P.ep_add ? P.add_scale * P.ep_add[(size_t)arow_ * P.ld_add + colc] : 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int rw = rbase + (r & 3) + 8 * (r >> 2);
      float v = v16[r] + bias;
      if (P.ep_x) v *= dl3_act_mask(es * xr_[r] + et, P.ep_act);
      v += ad[r];
      if (cok && rw < P.M) {
        __builtin_nontemporal_store(v, &P.c[(size_t)rw * P.ldc + col]);
        s1 += v;
        s2 += mode2 ? v * ((xr_[r] - mu) * is) : v * v;
      }
    }
    if (P.stat_mode != 0) {
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (lhi == 0 && cok) {
        P.part[((size_t)blockIdx.x * P.N + col) * 2 + 0] = s1;
        P.part[((size_t)blockIdx.x * P.N + col) * 2 + 1] = s2;
        for (int rr = blockIdx.x + (int)gridDim.x; rr < P.part_rows; rr += (int)gridDim.x) {
          P.part[((size_t)rr * P.N + col) * 2 + 0] = 0.f;
          P.part[((size_t)rr * P.N + col) * 2 + 1] = 0.f;
        }
      }
    }
  }
}

// ---- dl3_pwconv_fwd_rows: a handful of rows (the ASPP image-pooling branch: ONE row per image, deeplabv3p.py:375-382,
// and its share of concat_projection, :402-406): Y[m][n] = act(ka*x + kc)[m][:] . W[:][n] + bias + addend, in DOUBLE.  The
// result is a per-image constant the network adds to every pixel of the 64x64 map: its rounding error does not average
// out over pixels, and a reduction of 2 048 on the f32 MFMA was where the HIP path's distance to float64 left torch-fp32's
// (tools/r5/xception_layer_distance.py: ratio 1.00 up to the exit flow, 1.08 behind image_pooling, 1.15 at the logits).
// 16 columns x 16 slices of the reduction per workgroup (a lane's chain is K/16 long: at M = 2 rows the launch is eight to
// thirty-two workgroups and its time is that chain), four independent partial sums per lane, slices folded in slice order.
constexpr int ROWS_CL = 16, ROWS_SL = 16;
__global__ __launch_bounds__(256) void pw_rows_f64_kernel(GemmArgs P) {
  __shared__ double red[ROWS_SL][ROWS_CL];
  const int cl = threadIdx.x % ROWS_CL, sl = threadIdx.x / ROWS_CL;
  const int n = blockIdx.x * ROWS_CL + cl, m = blockIdx.y;
  const int kper = (P.K + ROWS_SL - 1) / ROWS_SL, k0 = sl * kper, k1 = min(P.K, k0 + kper);
  const float *xr = P.a + (size_t)m * P.lda;
  const bool xform = P.ka != nullptr;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (n < P.N) {
    auto term = [&](int k) -> double {
      float v = xr[k];
      if (xform) v = P.ka[k] * v + P.kc[k];
      v = dl3_act(v, P.a_act);
      return (double)v * (double)P.b[(size_t)k * P.ldb + n];
    };
    int k = k0;
    for (; k + 4 <= k1; k += 4) {
      a0 += term(k);
      a1 += term(k + 1);
      a2 += term(k + 2);
      a3 += term(k + 3);
    }
    for (; k < k1; k++) a0 += term(k);
  }
  red[sl][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (sl == 0 && n < P.N) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < ROWS_SL; i++) t += red[i][cl];
    if (P.bias) t += (double)P.bias[n];
    if (P.ep_add) t += (double)(P.add_scale * P.ep_add[(size_t)(m / P.add_div) * P.ld_add + n]);
    P.c[(size_t)m * P.ldc + n] = (float)t;
  }
}
}  // namespace

// (tests/test_pwconv_cases_host.py::test_universe_restates_the_launchers reads this switch as text and tests/pwconv_cases.py universe()
// lists its instantiations: an instantiation added, dropped or renamed here is added there, with a case that reaches it)
void pw::launch_ksplit(const GemmArgs &A, const GemmPlan &P, void *stream) {
  const dim3 grid(P.grid[0], P.grid[1], P.grid[2]), blk(256);
#define DL3_GO(KERNEL_) hipLaunchKernelGGL((KERNEL_), grid, blk, P.lds, (hipStream_t)stream, A)
  switch (P.tn * 2 + (P.two ? 1 : 0)) {
    case 4: DL3_GO((pw_ksplit32_kernel<2, false>)); break;
    case 5: DL3_GO((pw_ksplit32_kernel<2, true>)); break;
    case 6: DL3_GO((pw_ksplit32_kernel<3, false>)); break;
    case 7: DL3_GO((pw_ksplit32_kernel<3, true>)); break;
    case 10: DL3_GO((pw_ksplit32_kernel<5, false>)); break;
    default: DL3_GO((pw_ksplit32_kernel<5, true>)); break;
  }
#undef DL3_GO
}

void pw::launch_rows(const GemmArgs &A, void *stream) {
  hipLaunchKernelGGL(pw_rows_f64_kernel, dim3(dl3_cdiv(A.N, ROWS_CL), A.M), dim3(256), 0, (hipStream_t)stream, A);
}
