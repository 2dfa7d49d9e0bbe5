// pwstream.hip — the stream kernel of the 1x1-convolution GEMMs (PW_STREAM), the default route: the A operand goes global ->
// registers -> MFMA, the weight tile is double-buffered in LDS.  f32 MFMA and split math (three bf16 pieces per fp32 operand,
// pwdev.h), the weight packing of split math (pack_b_kernel) and its per-process scratch.  Fragment layouts: pwgemm.hip.
#include <mutex>
#include <vector>
#include "common.h"
#include "pwargs.h"
#include "pwdev.h"
namespace {
using pw::GemmArgs;

#ifndef DL3_STREAM_KT_FWD
#define DL3_STREAM_KT_FWD 16  // K-tile depth of the forward instantiation (32 measured in round 2: see DESIGN.md)
#endif
#ifndef DL3_STREAM_KT_BWD1
#define DL3_STREAM_KT_BWD1 16  // K-tile depth of the single-tensor bwd-data instantiation (dY materialised, round 4)
#endif
#ifndef DL3_STREAM_PD_SMALL
#define DL3_STREAM_PD_SMALL 2  // 32-row (small-M) stream kernels: K-tiles of operands in flight (register ring); 1 = the plain loop
#endif

// W[K][N] (row stride ldb) -> out[K-tile of 32][k-step s][plane][sub-tile][lane] (16 B each): lane l of sub-tile j holds
// column 32 j + (l & 31) and k = 32 kt + 16 (l >> 5) + 8 s + 0..7 — the B fragment of v_mfma_f32_32x32x16_bf16 under the
// stream kernel's k map.  Zero beyond K / N.
__global__ __launch_bounds__(256) void pack_b_kernel(const float *__restrict__ b, int ldb, int K, int N,
                                                     u32x4 *__restrict__ out, int ktiles, int nsub) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ktiles * 2 * nsub * 64) return;
  const int lane = t & 63, j = (t >> 6) % nsub, ks = ((t >> 6) / nsub) & 1, kt = (t >> 6) / nsub / 2;
  const int col = j * 32 + (lane & 31), k0 = kt * 32 + 16 * (lane >> 5) + 8 * ks;
  f32x4 v0, v1;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int k = k0 + e;
    const float x = (k < K && col < N) ? b[(size_t)k * ldb + col] : 0.f;
    if (e < 4) v0[e] = x; else v1[e - 4] = x;
  }
  u32x4 h, m, l;
  split3(v0, v1, h, m, l);
  const size_t base = ((size_t)(kt * 2 + ks) * 3 * nsub + j) * 64 + lane;
  out[base] = h;
  out[base + (size_t)nsub * 64] = m;
  out[base + (size_t)2 * nsub * 64] = l;
}

// Epilogue of the stream kernel for a tile that lies inside the matrix, specialised at compile time on what it has to
// do.  (The generic version below tests its run-time flags and the bounds on every element; its exec-mask branches and
// waits cost ~28k cycles per 128x160 tile — two thirds of the main loop of a K=160 GEMM.)  EPX: activation mask from
// the forward input (bwd-data); ADD: residual gradient; MODE2: second statistic is sum(c * xhat) instead of sum(c^2).
// All 16 (32 with ADD) global reads of a 32x32 sub-tile are issued before the first use.
template <int TM, int TN, bool EPX, bool ADD, bool MODE2>
__device__ __forceinline__ void stream_epilogue_full(const GemmArgs &P, const f32x16 (&acc)[TM][TN], int m0, int n0,
                                                     int wm, int l31, int lhi, float (&st1)[TN], float (&st2)[TN]) {
  // addresses = wave-uniform base (scalar registers) + ONE 32-bit lane offset per tensor: the rows of a sub-tile differ
  // by uniform multiples of the leading dimension, only (lane >> 5, lane & 31) is lane-specific
  const int wmu = __builtin_amdgcn_readfirstlane(wm);
  const unsigned lo_c = (unsigned)(4 * lhi * P.ldc + l31);
  const unsigned lo_x = EPX ? (unsigned)(4 * lhi * P.ld_epx + l31) : 0u;
  const unsigned lo_a = ADD ? (unsigned)(4 * lhi * P.ld_add + l31) : 0u;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int col = n0 + j * 32 + l31;
    float bias = 0.f, es = 1.f, et = 0.f, mu = 0.f, is = 0.f;
    if (P.bias) bias = P.bias[col];
    if (EPX && P.ep_scale) { es = P.ep_scale[col]; et = P.ep_shift[col]; }
    if (MODE2) { mu = P.ep_mean[col]; is = P.ep_invstd[col]; }
#pragma unroll
    for (int i = 0; i < TM; i++) {
      const size_t urow = (size_t)(m0 + (wmu * TM + i) * 32);
      const int ucol = n0 + j * 32;
      float *pc = P.c + urow * P.ldc + ucol;
      const float *px = EPX ? P.ep_x + urow * P.ld_epx + ucol : nullptr;
      const float *pa = ADD ? P.ep_add + urow * P.ld_add + ucol : nullptr;
      float xr_[16], ad[16];
      if (EPX) {
#pragma unroll
        for (int r = 0; r < 16; r++) xr_[r] = (px + (size_t)((r & 3) + 8 * (r >> 2)) * P.ld_epx)[lo_x];
      }
      if (ADD) {
        if (P.add_div > 1) {
          // one addend row per image (run_gemm only sends a launch here when 32-row blocks never straddle two images)
          const float a0 = P.add_scale * P.ep_add[(urow / (size_t)P.add_div) * P.ld_add + ucol + l31];
#pragma unroll
          for (int r = 0; r < 16; r++) ad[r] = a0;
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) ad[r] = P.add_scale * (pa + (size_t)((r & 3) + 8 * (r >> 2)) * P.ld_add)[lo_a];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = acc[i][j][r] + bias;
        if (EPX) v *= dl3_act_mask(es * xr_[r] + et, P.ep_act);
        if (ADD) v += ad[r];
#ifndef DL3_DBG_NOSTORE
        __builtin_nontemporal_store(v, &(pc + (size_t)((r & 3) + 8 * (r >> 2)) * P.ldc)[lo_c]);
#else
        if (v == 1.2345e30f) __builtin_nontemporal_store(v, &(pc + (size_t)((r & 3) + 8 * (r >> 2)) * P.ldc)[lo_c]);
#endif
#ifndef DL3_DBG_NOSTAT
        st1[j] += v;
        st2[j] += MODE2 ? v * ((xr_[r] - mu) * is) : v * v;
#endif
      }
      // keep the sub-tiles apart: interleaving them would hold several sub-tiles' operands live on top of the
      // accumulators (spills)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// FWD: the launch has no masked epilogue (no ep_x, stat_mode != 2, no per-image broadcast residual) — the forward
// GEMMs; their interior tiles take the straight-line epilogue and the masked code is not compiled in at all.
// WN: waves side by side along N (4/WN stacked along M).  WN = 4 gives 32-row tiles for small M (batch 1-4: a
// 128-row tile leaves most CUs idle and every workgroup a long serial K loop).
template <int TM, int TN, bool TWO, int KT, int EPI, int WN = 1, int MATH = 0>
__global__ __launch_bounds__(256, 2) void pw_gemm_stream_kernel(GemmArgs P) {
  // MATH 1: split math (see split3) — the A registers are split after the operand transform, the weight tile comes
  // pre-split from pack_b_kernel, six bf16 MFMAs per 16-deep K-tile and 32x32 sub-tile
  constexpr bool SPL = (MATH == 1);
  static_assert(!SPL || KT == 32, "split math: two bf16 MFMA k-steps per K-tile");
  // EPI: 0 generic epilogue only, 1 forward (see above).  A straight-line MASKED bwd-data variant was measured too:
  // on top of 80 accumulators its operand registers push long-lived values into scratch and it came out slower.
  constexpr bool FWD = (EPI == 1);
  // EPI 2 (bwd-data without residual, TM = 1, TN <= 3): the masked epilogue's operand — the forward input x of the
  // tile — is requested BEFORE the main loop and consumed after it.  The generic epilogue
  // fetches them sub-tile by sub-tile after the last MFMA, one exposed HBM round trip each (~4 us per sub-tile; for a
  // reduction of 96-320 that is as long as the main loop itself, and the in-situ table shows exactly these launches
  // running at mfma-time + hbm-time).  48 accumulators + 48 operand registers fit two waves per SIMD next to the main
  // loop's own; 80 + 80 do not (nor 48 + 96 with a residual operand: measured, spills between the loads).
  constexpr bool PRE = (EPI == 2);
  static_assert(!PRE || (TM == 1 && WN == 1 && TN <= 3), "prefetched epilogue: narrow single-row-block tiles only");
  // (round 4, single-tensor operand: the same at 128x160 — 80 accumulators + 80 prefetched operands — still does not fit:
  // 200 B of scratch, 30-40 of the operands are parked there as they arrive, which puts their HBM round trip in front of
  // the K loop again: bwd-data GEMMs 23.1 -> 25.0 ms per step, profiles/r04_ab_calls.txt call 13)
  // (EPI 3 / 4, round 4: a straight-line MASKED epilogue for the single-tensor bwd-data launches — forward input for the
  // mask and x_hat, optional residual, BatchNorm-backward sums; 0-260 B of scratch once the epilogue addresses were
  // fenced — measured no faster than the generic epilogue below: bwd-data GEMMs 25.95 ms per step with it, 25.81 without
  // (B=128, same call, profiles/r04_ab_dy_epilogue.txt); removed again)
  // KT = depth of one K-tile: each half-wave walks KT/2 consecutive k (KT/8 float4 loads per lane and tensor)
  constexpr int WM = 4 / WN;
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, KH = KT / 2, NJ = KT / 8;
  constexpr int LDB = BN;
  constexpr int NS = KT / 16;                    // split math: bf16 MFMA k-steps per K-tile
  constexpr int BQ = SPL ? NS * 3 * (BN / 32) * 64 : KT * BN / 4;  // 16-byte pieces of one K-tile's weight tile
  constexpr int NB = SPL ? 1 : (KT * BN / 4 + 255) / 256;  // float4 B loads per thread per K-tile (f32 path)
  constexpr int KCS = DL3_STREAM_KMAX + KT;      // per-k operand-transform coefficients live in LDS
  __shared__ float lds[2 * BQ * 4];
  // split math: the coefficient vectors are sized by the launch (dynamic LDS, 4 * (2 or 3) * ktiles * KT bytes) so that
  // two workgroups of the 160-wide tile still fit a CU next to the 60 KB of split weight tiles
  __shared__ float cf_static[SPL ? 1 : (TWO ? 3 : 2) * KCS];
  extern __shared__ float cf_dyn[];
  float *const cf = SPL ? cf_dyn : cf_static;
  __shared__ float eco[PRE ? 4 * BN : 1];  // prefetched epilogue: per-column scale, shift, mean, invstd (n0 is fixed)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int nwg = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = b & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (b >> 3);
  const int bx = lid % gridDim.x, by = lid / gridDim.x;
  const int n0 = bx * BN;
  const int ktiles = (P.K + KT - 1) / KT;
  const int KC = SPL ? ktiles * KT : KCS;
  const bool xform = (P.ka != nullptr);
  const int wm = wave / WN, wn = wave % WN;
  const int nw0 = n0 + wn * TN * 32;  // first column of this wave's sub-tile

  float st1[TN], st2[TN];
#pragma unroll
  for (int i = 0; i < TN; i++) st1[i] = st2[i] = 0.f;

  // T(a)[k] = act(ka[k]*a + kb[k]*a2 + kc[k]); k >= K gets all-zero coefficients, so the clamped (in-bounds) loads
  // beyond K contribute act(0) = 0
  for (int i = tid; i < ktiles * KT; i += 256) {
    const bool in = i < P.K;
    const int k = min(i, P.K - 1);
    cf[i] = in ? (xform ? P.ka[k] : 1.f) : 0.f;
    cf[KC + i] = (in && xform) ? P.kc[k] : 0.f;
    if (TWO) cf[2 * KC + i] = in ? P.kb[k] : 0.f;
  }
  if constexpr (PRE) {
    for (int i = tid; i < BN; i += 256) {
      const int col = min(n0 + i, P.N - 1);
      eco[i] = P.ep_scale ? P.ep_scale[col] : 1.f;
      eco[BN + i] = P.ep_scale ? P.ep_shift[col] : 0.f;
      eco[2 * BN + i] = P.stat_mode == 2 ? P.ep_mean[col] : 0.f;
      eco[3 * BN + i] = P.stat_mode == 2 ? P.ep_invstd[col] : 0.f;
    }
  }
  __syncthreads();

  for (int mt = by; mt < P.mtiles; mt += gridDim.y) {
    const int m0 = mt * BM;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const bool full = (m0 + BM <= P.M) && (n0 + BN <= P.N);
    float pxv[PRE ? TN : 1][16];
    if constexpr (PRE) {
      if (full) {
        const size_t urow = (size_t)(m0 + __builtin_amdgcn_readfirstlane(wm) * 32);
        const float *px = P.ep_x + urow * P.ld_epx + nw0;
        const unsigned lo_x = (unsigned)(4 * lhi * P.ld_epx + l31);
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) pxv[j][r] = (px + (size_t)((r & 3) + 8 * (r >> 2)) * P.ld_epx + j * 32)[lo_x];
      }
    }

    const float *arow[TM], *arow2[TM];
#pragma unroll
    for (int i = 0; i < TM; i++) {
      const int row = min(m0 + (wm * TM + i) * 32 + l31, P.M - 1);
      arow[i] = P.a + (size_t)row * P.lda;
      arow2[i] = TWO ? P.a2 + (size_t)row * P.lda2 : nullptr;
    }
    f32x4 an[TM][NJ], an2[TM][NJ], ac[TM][NJ], rb[NB];

    // (the `_to` / `_from` forms name the register set: the ring loop of the 32-row kernels keeps several K-tiles in flight)
    auto load_A_to = [&](int kt, f32x4 (&da)[TM][NJ], f32x4 (&da2)[TM][NJ]) {
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int kc = min(kt * KT + KH * lhi + 4 * j, P.K - 4);
#pragma unroll
        for (int i = 0; i < TM; i++) {
          da[i][j] = ld4(arow[i] + kc);
          if (TWO) da2[i][j] = ld4(arow2[i] + kc);
        }
      }
    };
    auto load_B_to = [&](int kt, f32x4 (&db)[NB]) {
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (NB * 256 == KT * BN / 4 || idx < KT * BN / 4) {
          const int kk = idx / (BN / 4), nq = idx % (BN / 4);
          const int krow = min(kt * KT + kk, P.K - 1), col = min(n0 + nq * 4, P.N - 4);
          db[i] = ld4(P.b + (size_t)krow * P.ldb + col);
        }
      }
    };
    auto store_B_from = [&](float *Bs, const f32x4 (&db)[NB]) {
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int idx = tid + 256 * i;
        if (NB * 256 == KT * BN / 4 || idx < KT * BN / 4) st4(&Bs[(idx / (BN / 4)) * LDB + (idx % (BN / 4)) * 4], db[i]);
      }
    };
    auto load_A = [&](int kt) { load_A_to(kt, an, an2); };
    auto load_B = [&](int kt) { load_B_to(kt, rb); };
    auto store_B = [&](float *Bs) { store_B_from(Bs, rb); };
    // loaded registers of K-tile kt -> MFMA operand values.  f32 path: straight into the operand registers ac, AFTER the
    // last MFMA of the running K-tile has been issued (round 3: a wave's own VALU work does not overlap its own MFMAs, so
    // there is nothing to gain from placing it earlier, and the separate copy an -> ac cost 8 v_mov per K-tile);
    // split path: in place (an <- T(an)), split3 reads it
    auto transform_from = [&](int kt, f32x4 (&sa)[TM][NJ], const f32x4 (&sa2)[TM][NJ]) {
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int k = kt * KT + KH * lhi + 4 * j;
        const f32x4 fa = ld4(cf + k), fc = ld4(cf + KC + k);
#pragma unroll
        for (int i = 0; i < TM; i++) {
          f32x4 v = fa * sa[i][j] + fc;
          if (TWO) v += ld4(cf + 2 * KC + k) * sa2[i][j];
          if constexpr (SPL) sa[i][j] = dl3_act4(v, P.a_act);
          else ac[i][j] = dl3_act4(v, P.a_act);
        }
      }
    };
    auto transform = [&](int kt) { transform_from(kt, an, an2); };

    if constexpr (SPL) {
      // K-tile kt: [weights of kt+1 -> LDS by DMA] [MFMAs of k-step 0] [A of kt+1: wait, transform, split; request A of
      // kt+2] [MFMAs of k-step 1] [barrier].  The A loads have a whole K-tile of MFMAs (x2 waves per SIMD) to arrive.
      // Slot (k-step s, half h, element e) of a K-tile holds k = 16 h + 8 s + e — each lane's 16 k are consecutive in
      // memory; pack_b_kernel lays the weights out with the same map.
      u32x4 ch[NS][TM], cm[NS][TM], cl[NS][TM], nh[NS][TM], nm[NS][TM], nl[NS][TM];
      auto dma_B = [&](int kt, int buf) {
        constexpr int PIECES = NS * 3 * (BN / 32);  // 1 KB each: 64 lanes x 16 B, lane-linear in LDS
        const char *src0 = (const char *)P.bp + (size_t)lane * 16;
        for (int pc = __builtin_amdgcn_readfirstlane(wave); pc < PIECES; pc += 4) {
          const int sub = pc % (BN / 32), pl = (pc / (BN / 32)) % 3, ks = pc / (3 * (BN / 32));
          const int gsub = min(n0 / 32 + sub, P.nsub - 1);
          const size_t off = (((size_t)(kt * NS + ks) * 3 + pl) * P.nsub + gsub) * 1024;  // wave-uniform
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src0 + off),
                                           (__attribute__((address_space(3))) void *)(lds + (buf * BQ + pc * 64) * 4), 16, 0, 0);
        }
      };
      auto split_next = [&]() {
#pragma unroll
        for (int ks = 0; ks < NS; ks++)
#pragma unroll
          for (int i = 0; i < TM; i++) split3(an[i][2 * ks], an[i][2 * ks + 1], nh[ks][i], nm[ks][i], nl[ks][i]);
      };
      auto take_next = [&]() {
#pragma unroll
        for (int ks = 0; ks < NS; ks++)
#pragma unroll
          for (int i = 0; i < TM; i++) { ch[ks][i] = nh[ks][i]; cm[ks][i] = nm[ks][i]; cl[ks][i] = nl[ks][i]; }
      };
      auto mfma_step = [&](const float *Bs, int ks) {
        const u32x4 *Bq = (const u32x4 *)Bs + (ks * 3 * (BN / 32) + wn * TN) * 64 + lane;
#pragma unroll
        for (int j = 0; j < TN; j++) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, Bq[j * 64]);
          const bf16x8 bm = __builtin_bit_cast(bf16x8, Bq[((BN / 32) + j) * 64]);
          const bf16x8 bl = __builtin_bit_cast(bf16x8, Bq[(2 * (BN / 32) + j) * 64]);
#pragma unroll
          for (int i = 0; i < TM; i++) {
            const bf16x8 ah = __builtin_bit_cast(bf16x8, ch[ks][i]), am = __builtin_bit_cast(bf16x8, cm[ks][i]),
                         al = __builtin_bit_cast(bf16x8, cl[ks][i]);
            f32x16 c = acc[i][j];  // small terms first
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
          }
        }
      };
      // Every wave DMAs only its own pieces of a weight tile and, after the barrier, reads ALL of them: a wave must not
      // reach the barrier with its DMA still in flight.  s_barrier does not imply it on gfx950 (back-off barriers), so
      // the vmcnt(0) is spelled out (0x0F70 = vmcnt 0, expcnt / lgkmcnt untouched) instead of left to the fence the
      // compiler happens to emit for __syncthreads today.  (Waiting for LESS — a counted vmcnt that keeps the operand
      // request of K-tile kt+2 in flight across a raw s_barrier — was measured in round 3: split math 1 235-1 245 img/s
      // either way.)
      load_A(0);
      __syncthreads();  // the previous row tile is done with the LDS
      dma_B(0, 0);
      transform(0);
      split_next();
      take_next();
      if (ktiles > 1) load_A(1);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      for (int kt = 0; kt < ktiles; ++kt) {
        const float *Bs = lds + (kt & 1) * BQ * 4;
        const bool more = kt + 1 < ktiles;
        if (more) dma_B(kt + 1, (kt + 1) & 1);
        mfma_step(Bs, 0);
        if (more) {
          transform(kt + 1);
          split_next();
          if (kt + 2 < ktiles) load_A(kt + 2);
        }
        mfma_step(Bs, 1);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (more) take_next();
      }
    } else if constexpr (WN == 4 && DL3_STREAM_PD_SMALL > 1) {
    // 32-row tiles (small M: a few hundred workgroups, each a long serial chain of short K-tiles — 8-16 MFMAs per wave):
    // a ring of PD register sets keeps PD K-tiles of both operands in flight; __syncthreads only waits for the LDS
    // (lgkmcnt) on gfx950, so the requests survive the barriers.  The loop is unrolled by PD so that the set index is a
    // constant.  Measured (round 4, call 14, same box): B=2 478.5 / 477.7 img/s with PD = 1, 486.2 / 486.1 with 2, 480.2 /
    // 480.3 with 3 (251-254 VGPRs: two workgroups per CU instead of three); B=4 683 / 690 / 687; B=16 unchanged.  The exposed
    // round trip was a small part of these K-tiles after all — their 8-16 MFMAs on a 160-wide output padded to 256 columns
    // are most of the 0.7 us each takes.
    constexpr int PD = (TWO && DL3_STREAM_PD_SMALL > 2) ? 2 : DL3_STREAM_PD_SMALL;  // (two-tensor operand: a third set spills)
    f32x4 ra[PD][TM][NJ], ra2[PD][TM][NJ], rbb[PD][NB];
#pragma unroll
    for (int d = 0; d < PD; d++)
      if (d < ktiles) {
        load_B_to(d, rbb[d]);
        load_A_to(d, ra[d], ra2[d]);
      }
    __syncthreads();  // the previous row tile is done with the LDS
    store_B_from(lds, rbb[0]);
    transform_from(0, ra[0], ra2[0]);
    __syncthreads();
    for (int kt0 = 0; kt0 < ktiles; kt0 += PD) {
#pragma unroll
      for (int d = 0; d < PD; d++) {
        const int kt = kt0 + d;
        if (kt < ktiles) {  // (the same for every wave of the workgroup: the barrier below is safe)
          const float *Bs = lds + (kt & 1) * KT * LDB;
          // set d (K-tile kt) went to the LDS / the operand registers at the end of the previous K-tile: refill it
          if (kt + PD < ktiles) {
            load_B_to(kt + PD, rbb[d]);
            load_A_to(kt + PD, ra[d], ra2[d]);
          }
          float bf[2][TN];
#pragma unroll
          for (int j = 0; j < TN; j++) bf[0][j] = Bs[(KH * lhi) * LDB + (wn * TN + j) * 32 + l31];
#pragma unroll
          for (int s_ = 0; s_ < KH; ++s_) {
            const int cur = s_ & 1, nxt = cur ^ 1;
            if (s_ + 1 < KH) {
#pragma unroll
              for (int j = 0; j < TN; j++) bf[nxt][j] = Bs[(KH * lhi + s_ + 1) * LDB + (wn * TN + j) * 32 + l31];
            }
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
              for (int j = 0; j < TN; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i][s_ >> 2][s_ & 3], bf[cur][j], acc[i][j], 0, 0, 0);
          }
          if (kt + 1 < ktiles) {
            const int dn = (d + 1) % PD;  // (a constant once the loop is unrolled)
            store_B_from(lds + ((kt + 1) & 1) * KT * LDB, rbb[dn]);
            transform_from(kt + 1, ra[dn], ra2[dn]);
          }
          __syncthreads();
        }
      }
    }
    } else {
    load_A(0);
    load_B(0);
    __syncthreads();  // the previous row tile is done with the LDS
    store_B(lds);
    transform(0);
    __syncthreads();
    for (int kt = 0; kt < ktiles; ++kt) {
      const float *Bs = lds + (kt & 1) * KT * LDB;
      const bool more = kt + 1 < ktiles;
      if (more) {
        load_A(kt + 1);
        load_B(kt + 1);
      }
      float bf[2][TN];
#pragma unroll
      for (int j = 0; j < TN; j++) bf[0][j] = Bs[(KH * lhi) * LDB + (wn * TN + j) * 32 + l31];
#pragma unroll
      for (int s_ = 0; s_ < KH; ++s_) {
        const int cur = s_ & 1, nxt = cur ^ 1;
        if (s_ + 1 < KH) {
#pragma unroll
          for (int j = 0; j < TN; j++) bf[nxt][j] = Bs[(KH * lhi + s_ + 1) * LDB + (wn * TN + j) * 32 + l31];
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i][s_ >> 2][s_ & 3], bf[cur][j], acc[i][j], 0, 0, 0);
      }
      // next tile's weight tile -> LDS and operand transform, behind the last MFMA of this K-tile
      if (more) {
        store_B(lds + ((kt + 1) & 1) * KT * LDB);
        transform(kt + 1);
      }
      __syncthreads();
    }

    }

    // ---------------- epilogue (same C/D layout as the LDS-staged kernel)
#ifndef DL3_EPI_NOFENCE
    // The epilogue's addresses depend only on the tile coordinates: left alone, the scheduler computes them BEFORE the
    // K loop and spills them across it (round 4, kernel-resource-usage: 75 scratch stores per row tile in front of the
    // loop, ~100 reloads behind it in the 128x160 masked kernel).  Laundering the coordinates through an empty asm behind
    // the last MFMA pins that arithmetic where it is used.
    int m0e = __builtin_amdgcn_readfirstlane(m0), nw0e = __builtin_amdgcn_readfirstlane(nw0);  // (wave-uniform both)
    asm volatile("" : "+s"(m0e), "+s"(nw0e));
#else
    const int m0e = m0, nw0e = nw0;
#endif
    if (FWD && full) {
      if (!P.ep_add) stream_epilogue_full<TM, TN, false, false, false>(P, acc, m0e, nw0e, wm, l31, lhi, st1, st2);
      else stream_epilogue_full<TM, TN, false, true, false>(P, acc, m0e, nw0e, wm, l31, lhi, st1, st2);
      continue;
    }
    if constexpr (PRE) {
      if (full) {
        float *pc = P.c + (size_t)(m0e + __builtin_amdgcn_readfirstlane(wm) * 32) * P.ldc + nw0e;
        const unsigned lo_c = (unsigned)(4 * lhi * P.ldc + l31);
        const bool mode2 = P.stat_mode == 2;
#pragma unroll
        for (int j = 0; j < TN; j++) {
          const int cl = j * 32 + l31;
          const float es = eco[cl], et = eco[BN + cl], mu = eco[2 * BN + cl], is = eco[3 * BN + cl];
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const float xv = pxv[j][r];
            float v = acc[0][j][r] * dl3_act_mask(es * xv + et, P.ep_act);
            __builtin_nontemporal_store(v, &(pc + (size_t)((r & 3) + 8 * (r >> 2)) * P.ldc + j * 32)[lo_c]);
            st1[j] += v;
            st2[j] += mode2 ? v * ((xv - mu) * is) : v * v;
          }
        }
        continue;
      }
    }
    // everything else: generic path, every element predicated
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col = nw0e + j * 32 + l31;
      const bool cok = col < P.N;
      const int colc = min(col, P.N - 1);
      float bias = 0.f, es = 1.f, et = 0.f, mu = 0.f, is = 0.f;
      if (P.bias) bias = P.bias[colc];
      if (!FWD && P.ep_scale) { es = P.ep_scale[colc]; et = P.ep_shift[colc]; }
      if (!FWD && P.stat_mode == 2) { mu = P.ep_mean[colc]; is = P.ep_invstd[colc]; }
#pragma unroll
      for (int i = 0; i < TM; i++) {
        const int rbase = m0e + (wm * TM + i) * 32 + 4 * lhi;
        float xr_[16], ad[16];
        if (!FWD && P.ep_x) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = min(rbase + (r & 3) + 8 * (r >> 2), P.M - 1);
            xr_[r] = P.ep_x[(size_t)row * P.ld_epx + colc];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) xr_[r] = 0.f;
        }
        if (P.ep_add) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = min(rbase + (r & 3) + 8 * (r >> 2), P.M - 1);
            const int arow_ = (P.add_div > 1) ? row / P.add_div : row;
            ad[r] = P.add_scale * P.ep_add[(size_t)arow_ * P.ld_add + colc];
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
          if (!FWD && P.ep_x) v *= dl3_act_mask(es * xr_[r] + et, P.ep_act);
          v += ad[r];
          if (ok) {
            __builtin_nontemporal_store(v, &P.c[(size_t)row * P.ldc + col]);
            st1[j] += v;
            st2[j] += (!FWD && P.stat_mode == 2) ? v * ((xr_[r] - mu) * is) : v * v;
          }
        }
      }
    }
  }

  if (P.stat_mode != 0) {
    float *sred = lds;  // [WM][BN][2]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; j++) {
      float a1 = st1[j] + __shfl_xor(st1[j], 32, 64);
      float a2 = st2[j] + __shfl_xor(st2[j], 32, 64);
      if (lhi == 0) {
        sred[(wm * BN + (wn * TN + j) * 32 + l31) * 2 + 0] = a1;
        sred[(wm * BN + (wn * TN + j) * 32 + l31) * 2 + 1] = a2;
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

// split math (opt-in): device scratch for the packed weights of the launch in flight, one buffer per DEVICE.  Launches on
// one stream are ordered, so one buffer serves them all — split-math launches of a device must not be issued from two
// streams at once (the engine issues them on one stream, eagerly or under capture; the weight-gradient kernels, the
// only launches that may run on a second stream, split in registers and do not use it).  Keying by stream as well
// (tried in round 3) breaks hipGraph capture: the capture stream is not the stream the eager warm-up step grew the
// buffer on, and nothing can be allocated while capturing.  A buffer only ever grows, and a superseded one stays
// allocated (a captured hipGraph may still point at it).
void *pack_scratch(size_t bytes, hipStream_t st) {
  struct Slot { int dev; void *buf; size_t cap; };
  static std::mutex mu;
  static std::vector<Slot> slots;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  Slot *s = nullptr;
  for (Slot &q : slots)
    if (q.dev == dev) { s = &q; break; }
  if (s && bytes <= s->cap) return s->buf;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cs);
  if (cs != hipStreamCaptureStatusNone) return nullptr;
  size_t want = bytes < (32u << 20) ? (32u << 20) : bytes * 2;
  void *nb = nullptr;
  if (hipMalloc(&nb, want) != hipSuccess) return nullptr;
  if (!s) {
    slots.push_back(Slot{dev, nullptr, 0});
    s = &slots.back();
  }
  s->buf = nb;
  s->cap = want;
  return nb;
}
}  // namespace

// (tests/test_pwconv_cases_host.py::test_universe_restates_the_launchers reads this switch as text and tests/pwconv_cases.py universe()
// lists its instantiations: an instantiation added, dropped or renamed here is added there, with a case that reaches it)
int pw::launch_stream(GemmArgs A, const GemmPlan &P, void *stream) {
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(P.grid[0], P.grid[1], P.grid[2]), blk(256);
  if (P.split) {
    const int ktiles = dl3_cdiv(A.K, 32);
    A.nsub = dl3_cdiv(A.N, 32);
    const size_t pieces = (size_t)ktiles * 2 * 3 * A.nsub * 64;
    void *ws = pack_scratch(pieces * 16, st);
    if (!ws) return -1;
    A.bp = ws;
    hipLaunchKernelGGL(pack_b_kernel, dim3(dl3_cdiv(ktiles * 2 * A.nsub * 64, 256)), blk, 0, st, A.b, A.ldb, A.K, A.N,
                       (u32x4 *)ws, ktiles, A.nsub);
  }
#define DL3_GO(KERNEL_) hipLaunchKernelGGL((KERNEL_), grid, blk, P.lds, st, A)
  // KT: 32-deep K-tiles in split math; the two-tensor bwd-data operand uses 16-deep ones so that its register budget does not spill
#define DL3_STREAM(TM_, TN_, WN_, KT2_, KTF_, KTB_, MATH_)                                          \
  do {                                                                                             \
    if (P.two) DL3_GO((pw_gemm_stream_kernel<TM_, TN_, true, KT2_, 0, WN_, MATH_>));               \
    else if (P.fwd) DL3_GO((pw_gemm_stream_kernel<TM_, TN_, false, KTF_, 1, WN_, MATH_>));         \
    else DL3_GO((pw_gemm_stream_kernel<TM_, TN_, false, KTB_, 0, WN_, MATH_>));                    \
  } while (0)
#define DL3_F32(TM_, TN_, WN_) DL3_STREAM(TM_, TN_, WN_, 16, DL3_STREAM_KT_FWD, DL3_STREAM_KT_BWD1, 0)
#define DL3_SPLIT(TM_, TN_, WN_) DL3_STREAM(TM_, TN_, WN_, 32, 32, 32, 1)
  if (P.pre) {   // (cfg 4: the 128x96 tile with the prefetched mask operand)
    if (P.split) {
      if (P.two) DL3_GO((pw_gemm_stream_kernel<1, 3, true, 32, 2, 1, 1>));
      else DL3_GO((pw_gemm_stream_kernel<1, 3, false, 32, 2, 1, 1>));
    } else {
      if (P.two) DL3_GO((pw_gemm_stream_kernel<1, 3, true, 16, 2, 1>));
      else DL3_GO((pw_gemm_stream_kernel<1, 3, false, 16, 2, 1>));
    }
  } else if (P.split) {
    switch (P.cfg) {
      case 0: DL3_SPLIT(1, 4, 1); break;
      case 1: DL3_SPLIT(2, 2, 1); break;
      case 2: DL3_SPLIT(2, 1, 1); break;
      case 3: DL3_SPLIT(1, 5, 1); break;
      default: DL3_SPLIT(1, 3, 1); break;
    }
  } else {
    switch (P.cfg) {
      case 0: DL3_F32(1, 4, 1); break;
      case 1: DL3_F32(2, 2, 1); break;
      case 2: DL3_F32(2, 1, 1); break;
      case 3: DL3_F32(1, 5, 1); break;
      case 5: DL3_F32(1, 2, 4); break;
      case 6: DL3_F32(1, 1, 4); break;
      default: DL3_F32(1, 3, 1); break;
    }
  }
#undef DL3_SPLIT
#undef DL3_F32
#undef DL3_STREAM
#undef DL3_GO
  return 0;
}
