// pwlds.hip — the tiled LDS kernel of the 1x1 GEMMs (PW_LDS): unaligned operands, reductions beyond DL3_STREAM_KMAX (pwgemm.hip)
#include "common.h"
#include "pwargs.h"
namespace {
using pw::GemmArgs;

constexpr int BK = 16;

// Main loop structure (both kernels): global -> registers -> LDS, double-buffered LDS (ONE barrier per
// K-tile), MFMA operand fragments prefetched one k-step ahead.  Out-of-range rows / columns are handled by
// clamping the ADDRESS (always in bounds, so loads are unconditional and branch-free) and zeroing the VALUE
// when it is written to LDS.
// VEC: 1 = 16-byte loads on both operands, 0 = scalar loads on both, 2 (round 5) = 16-byte loads on the activation operand
// only — the logits layer (K = 256, N = classes = 21): the big operand is the aligned one
template <int TM, int TN, int WM, int WN, int VEC>
__global__ __launch_bounds__(256, 2) void pw_gemm_kernel(GemmArgs P) {
  static_assert(WM * WN == 4, "4 waves per workgroup");
  constexpr bool AVEC = VEC != 0, BVEC = VEC == 1;
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int LDA = BM + 2;  // 4*LDA == 8 (mod 32): transposed 4-float stores hit distinct banks
  constexpr int LDB = BN + 4;
  constexpr int NA = BM / 64;               // float4 A loads per thread per K-tile
  constexpr int NB = (4 * BN + 255) / 256;  // float4 B loads per thread per K-tile
  constexpr int STAGE = BK * LDA + BK * LDB;
  __shared__ float lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, lhi = lane >> 5;
  // XCD-aware remap (workgroup b runs on XCD b % 8): give each XCD a contiguous run of logical ids so that the
  // column tiles of one row tile — which re-read the same A rows — share one XCD's L2.  Speed only.
  const int nwg = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = b & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (b >> 3);
  const int bx = lid % gridDim.x, by = lid / gridDim.x;
  const int n0 = bx * BN;
  const int akq = tid & 3, amr = tid >> 2;
  const int ktiles = (P.K + BK - 1) / BK;
  const bool xform = (P.ka != nullptr);
  const bool two = (P.a2 != nullptr);

  float st1[TN], st2[TN];
#pragma unroll
  for (int i = 0; i < TN; i++) st1[i] = st2[i] = 0.f;

  for (int mt = by; mt < P.mtiles; mt += gridDim.y) {
    const int m0 = mt * BM;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    f32x4 ra[NA], ra2[NA], rb[NB];

    auto load_tiles = [&](int kt) {
      const int k = kt * BK + akq * 4;
      if (AVEC) {
        const int kc = min(k, P.K - 4);
#pragma unroll
        for (int i = 0; i < NA; i++) {
          const int row = min(m0 + amr + 64 * i, P.M - 1);
          ra[i] = ld4(P.a + (size_t)row * P.lda + kc);
          if (two) ra2[i] = ld4(P.a2 + (size_t)row * P.lda2 + kc);
        }
      } else {
#pragma unroll
        for (int i = 0; i < NA; i++) {
          const int row = min(m0 + amr + 64 * i, P.M - 1);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int kc = min(k + j, P.K - 1);
            ra[i][j] = P.a[(size_t)row * P.lda + kc];
            if (two) ra2[i][j] = P.a2[(size_t)row * P.lda2 + kc];
          }
        }
      }
      if (BVEC) {
#pragma unroll
        for (int i = 0; i < NB; i++) {
          const int idx = tid + 256 * i;
          if (NB * 256 == 4 * BN || idx < 4 * BN) {
            const int kk = idx / (BN / 4), nq = idx % (BN / 4);
            const int krow = min(kt * BK + kk, P.K - 1), col = min(n0 + nq * 4, P.N - 4);
            rb[i] = ld4(P.b + (size_t)krow * P.ldb + col);
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < NB; i++) {
          const int idx = tid + 256 * i;
          if (NB * 256 == 4 * BN || idx < 4 * BN) {
            const int kk = idx / (BN / 4), nq = idx % (BN / 4);
            const int krow = min(kt * BK + kk, P.K - 1);
#pragma unroll
            for (int j = 0; j < 4; j++) rb[i][j] = P.b[(size_t)krow * P.ldb + min(n0 + nq * 4 + j, P.N - 1)];
          }
        }
      }
    };

    auto store_tiles = [&](int kt, float *As, float *Bs) {
      const int k = kt * BK + akq * 4;
      f32x4 fa = splat4(1.f), fb = splat4(0.f), fc = splat4(0.f);
      if (xform) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int kc = min(k + j, P.K - 1);
          fa[j] = P.ka[kc];
          fc[j] = P.kc[kc];
          if (two) fb[j] = P.kb[kc];
        }
      }
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const bool rok = (m0 + amr + 64 * i) < P.M;
        f32x4 v = ra[i];
        if (xform) {
          v = fa * v + fc;
          if (two) v += fb * ra2[i];
        }
        v = dl3_act4(v, P.a_act);
#pragma unroll
        for (int j = 0; j < 4; j++) As[(akq * 4 + j) * LDA + amr + 64 * i] = (rok && (k + j < P.K)) ? v[j] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (NB * 256 == 4 * BN || idx < 4 * BN) {
          const int kk = idx / (BN / 4), nq = idx % (BN / 4);
          const bool kok = (kt * BK + kk) < P.K;
          f32x4 v = rb[i];
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (!(kok && (n0 + nq * 4 + j < P.N))) v[j] = 0.f;
          st4(&Bs[kk * LDB + nq * 4], v);
        }
      }
    };

    load_tiles(0);
    __syncthreads();  // the previous m-tile's LDS reads (and the stat fold) are done
    store_tiles(0, lds, lds + BK * LDA);
    __syncthreads();
    for (int kt = 0; kt < ktiles; ++kt) {
      const float *As = lds + (kt & 1) * STAGE;
      const float *Bs = As + BK * LDA;
      const bool more = kt + 1 < ktiles;
      if (more) load_tiles(kt + 1);
      float af[2][TM], bf[2][TN];
#pragma unroll
      for (int i = 0; i < TM; i++) af[0][i] = As[lhi * LDA + (wm * TM + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < TN; j++) bf[0][j] = Bs[lhi * LDB + (wn * TN + j) * 32 + l31];
#pragma unroll
      for (int ks = 0; ks < BK / 2; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < BK / 2) {
#pragma unroll
          for (int i = 0; i < TM; i++) af[nxt][i] = As[(2 * ks + 2 + lhi) * LDA + (wm * TM + i) * 32 + l31];
#pragma unroll
          for (int j = 0; j < TN; j++) bf[nxt][j] = Bs[(2 * ks + 2 + lhi) * LDB + (wn * TN + j) * 32 + l31];
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
      }
      if (more) {
        float *An = lds + ((kt + 1) & 1) * STAGE;
        store_tiles(kt + 1, An, An + BK * LDA);
      }
      __syncthreads();
    }

    // ---------------- epilogue: all global reads of a 32x32 sub-tile are issued up front (clamped addresses,
    // no branches) so 16-32 loads per lane are in flight; values outside the matrix are dropped at the store
    const bool full = (m0 + BM <= P.M) && (n0 + BN <= P.N);
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col = n0 + (wn * TN + j) * 32 + l31;
      const bool cok = col < P.N;
      const int colc = min(col, P.N - 1);
      float bias = 0.f, es = 1.f, et = 0.f, mu = 0.f, is = 0.f;
      if (P.bias) bias = P.bias[colc];
      if (P.ep_scale) { es = P.ep_scale[colc]; et = P.ep_shift[colc]; }
      if (P.stat_mode == 2) { mu = P.ep_mean[colc]; is = P.ep_invstd[colc]; }
#pragma unroll
      for (int i = 0; i < TM; i++) {
        const int rbase = m0 + (wm * TM + i) * 32 + 4 * lhi;
        float xr[16], ad[16];
        if (P.ep_x) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = min(rbase + (r & 3) + 8 * (r >> 2), P.M - 1);
            xr[r] = P.ep_x[(size_t)row * P.ld_epx + colc];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) xr[r] = 0.f;
        }
        if (P.ep_add) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = min(rbase + (r & 3) + 8 * (r >> 2), P.M - 1);
            const int arow = (P.add_div > 1) ? row / P.add_div : row;
            ad[r] = P.add_scale * P.ep_add[(size_t)arow * P.ld_add + colc];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) ad[r] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = rbase + (r & 3) + 8 * (r >> 2);
          const bool ok = full || (cok && row < P.M);
          float v = acc[i][j][r] + bias;
          if (P.ep_x) v *= dl3_act_mask(es * xr[r] + et, P.ep_act);
          v += ad[r];
          if (ok) {
            __builtin_nontemporal_store(v, &P.c[(size_t)row * P.ldc + col]);
            st1[j] += v;
            st2[j] += (P.stat_mode == 2) ? v * ((xr[r] - mu) * is) : v * v;
          }
        }
      }
    }
  }

  if (P.stat_mode != 0) {
    // fold the two half-waves (same column), then the WM waves that share columns
    float *sred = lds;  // [WM][BN][2]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; j++) {
      float a1 = st1[j] + __shfl_xor(st1[j], 32, 64);
      float a2 = st2[j] + __shfl_xor(st2[j], 32, 64);
      if (lhi == 0) {
        const int cl = (wn * TN + j) * 32 + l31;
        sred[(wm * BN + cl) * 2 + 0] = a1;
        sred[(wm * BN + cl) * 2 + 1] = a2;
      }
    }
    __syncthreads();
    for (int cl = tid; cl < BN; cl += 256) {
      const int col = n0 + cl;
      if (col < P.N) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int w = 0; w < WM; w++) {
          a1 += sred[(w * BN + cl) * 2 + 0];
          a2 += sred[(w * BN + cl) * 2 + 1];
        }
        const int pld = P.part_ld ? P.part_ld : P.N;
        P.part[((size_t)by * pld + col) * 2 + 0] = a1;
        P.part[((size_t)by * pld + col) * 2 + 1] = a2;
        // rows of the buffer no workgroup owns (it is sized for the largest grid any tile choice uses): zeroed here, by
        // the row groups in turn, instead of by a memset node behind every launch
        for (int r = by + (int)gridDim.y; r < P.part_rows; r += (int)gridDim.y) {
          P.part[((size_t)r * pld + col) * 2 + 0] = 0.f;
          P.part[((size_t)r * pld + col) * 2 + 1] = 0.f;
        }
      }
    }
  }
}
}  // namespace

// (tests/test_pwconv_cases_host.py::test_universe_restates_the_launchers reads this switch as text and tests/pwconv_cases.py universe()
// lists its instantiations: an instantiation added, dropped or renamed here is added there, with a case that reaches it)
void pw::launch_lds(const GemmArgs &A, const GemmPlan &P, void *stream) {
  const dim3 grid(P.grid[0], P.grid[1], P.grid[2]), blk(256);
#define DL3_GO(KERNEL_) hipLaunchKernelGGL((KERNEL_), grid, blk, P.lds, (hipStream_t)stream, A)
#define DL3_LDS(TM_, TN_, WM_, WN_)                                                \
  do {                                                                             \
    if (P.vmode == 1) DL3_GO((pw_gemm_kernel<TM_, TN_, WM_, WN_, 1>));             \
    else if (P.vmode == 2) DL3_GO((pw_gemm_kernel<TM_, TN_, WM_, WN_, 2>));        \
    else DL3_GO((pw_gemm_kernel<TM_, TN_, WM_, WN_, 0>));                          \
  } while (0)
  switch (P.cfg) {
    case 0: DL3_LDS(2, 2, 2, 2); break;
    case 1: DL3_LDS(2, 2, 4, 1); break;
    case 2: DL3_LDS(2, 1, 4, 1); break;
    case 3: DL3_LDS(1, 5, 4, 1); break;
    default: DL3_LDS(1, 3, 4, 1); break;
  }
#undef DL3_LDS
#undef DL3_GO
}
