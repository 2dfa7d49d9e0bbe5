// pwwgrad.hip — the weight gradient of the 1x1 convolutions: dW[K,N] (+)= sum_m T(X)[m][k] * dY[m][n]; grid (ntn, ntk, S), the
// reduction over M in S slabs [S][K][N] the caller folds.  The tiled kernel (f32 and split math), the one-tile-row kernel of the
// expand convolutions, the logits layer's narrow kernel, the bias gradient's column sums.  Fragment layouts: pwgemm.hip.
#include <type_traits>
#include "common.h"
#include "pwargs.h"
#include "pwdev.h"
namespace {
using pw::WgradArgs;

// VEC: 1 = 16-byte loads of x and of g / y, 0 = scalar loads of both, 2 (round 5) = 16-byte loads of x only (N = classes)
template <int TA, int TB, int WA, int WB, int VEC, bool SPL = false>
__global__ __launch_bounds__(256, 2) void pw_wgrad_kernel(WgradArgs P) {
  constexpr bool XVEC = VEC != 0, DVEC = VEC == 1;
  static_assert(WA * WB == 4, "4 waves per workgroup");
  // SPL: split math (see split3).  The reduction index is the pixel row, and a bf16 MFMA wants 8 CONSECUTIVE reduction
  // elements per lane: lane (column c, half h) gathers rows 8h..8h+7 of its column from the fp32 stage in LDS (the same
  // number of ds_read_b32 per pixel as the f32 MFMA's one-per-k-step), splits them in registers, and one 16-row stage is
  // one k-step of six bf16 MFMAs per 32x32 sub-tile.
  static_assert(!SPL || DL3_WGRAD_MS == 16, "split math: a stage is one 16-deep bf16 MFMA k-step");
  constexpr int BKT = 32 * TA * WA, BNT = 32 * TB * WB, MS = DL3_WGRAD_MS;
  constexpr int LDX = BKT + 4, LDD = BNT + 4;
  constexpr int XQ = MS * BKT / 4, DQ = MS * BNT / 4;  // float4s per stage
  constexpr int NX = (XQ + 255) / 256, ND = (DQ + 255) / 256;
  constexpr int STAGE = MS * LDX + MS * LDD;
  __shared__ float lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wa = wave / WB, wb = wave % WB;
  const int l31 = lane & 31, lhi = lane >> 5;
  // XCD-aware decode: the tiles of ONE row slab (same activations / gradients, different weight tiles) get consecutive
  // virtual ids and therefore one XCD and its L2.  With the plain (x, y, z) order consecutive tiles land on different
  // XCDs and every tile re-reads its slab from HBM (TCC hit rate 0-3 % measured; the 160x960 layer moved 2.5 GB instead
  // of 1.1 GB per launch and ran at HBM speed, not MFMA speed).
  const int nwg = gridDim.x * gridDim.y * gridDim.z;
  const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  const int vid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int bx = vid % gridDim.x, by_ = (vid / gridDim.x) % gridDim.y, bz = vid / (gridDim.x * gridDim.y);
  const int kbase = by_ * BKT, nbase = bx * BNT;
  const int mbeg = bz * P.Mper;
  const int mend = min(P.M, mbeg + P.Mper);
  const bool xform = (P.xs != nullptr);
  const bool two = (P.cA != nullptr);
  // the workgroups of the first K-tile row also write the gradient operand they assemble anyway, dY = cA*g + cB*y + cC,
  // to HBM (every (row, column) is staged by exactly one (bx, by_ = 0, bz)): the bwd-data GEMM of the layer then reads ONE
  // tensor instead of two and has no operand transform (round 4)
  // ... and they take turns: the gridDim.y workgroups that share a row slab (same bx, bz: they all assemble the same dY
  // stages) each write every gridDim.y-th stage, so that no workgroup carries the whole store stream (first version, all
  // stores on by_ == 0: the launch waited for those workgroups, +4.5 ms per step for 25 GB of stores)
  const bool dy_on = (P.dyout != nullptr);

  f32x16 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // per-thread column positions are the same for every M stage: hoist coefficients and validity
  f32x4 xs4[NX], xt4[NX], kA4[ND], kB4[ND], kC4[ND];
  bool xok[NX][4], dok[ND][4];
#pragma unroll
  for (int i = 0; i < NX; i++) {
    const int idx = tid + 256 * i;
    const int k = kbase + (idx % (BKT / 4)) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      xok[i][j] = (k + j) < P.K;
      const int kc = min(k + j, P.K - 1);
      xs4[i][j] = xform ? P.xs[kc] : 1.f;
      xt4[i][j] = xform ? P.xt[kc] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < ND; i++) {
    const int idx = tid + 256 * i;
    const int col = nbase + (idx % (BNT / 4)) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      dok[i][j] = (col + j) < P.N;
      const int cc = min(col + j, P.N - 1);
      kA4[i][j] = two ? P.cA[cc] : 1.f;
      kB4[i][j] = two ? P.cB[cc] : 0.f;
      kC4[i][j] = two ? P.cC[cc] : 0.f;
    }
  }

  f32x4 rx[NX], rg[ND], ry[ND];

  auto load_tiles = [&](int m0) {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i;
      if (NX * 256 == XQ || idx < XQ) {
        const int mr = idx / (BKT / 4), kq = idx % (BKT / 4);
        const int row = min(m0 + mr, P.M - 1), k = kbase + kq * 4;
        if (XVEC) {
          rx[i] = ld4(P.x + (size_t)row * P.ldx + min(k, P.K - 4));
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) rx[i][j] = P.x[(size_t)row * P.ldx + min(k + j, P.K - 1)];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i;
      if (ND * 256 == DQ || idx < DQ) {
        const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
        const int row = min(m0 + mr, P.M - 1), col = nbase + nq * 4;
        if (DVEC) {
          const int cc = min(col, P.N - 4);
          rg[i] = ld4(P.g + (size_t)row * P.ldg + cc);
          if (two) ry[i] = ld4(P.y + (size_t)row * P.ldy + cc);
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int cc = min(col + j, P.N - 1);
            rg[i][j] = P.g[(size_t)row * P.ldg + cc];
            if (two) ry[i][j] = P.y[(size_t)row * P.ldy + cc];
          }
        }
      }
    }
  };

  auto store_tiles = [&](int m0, float *Xs, float *Ds) {
    const bool dy_owner = dy_on && (((m0 - mbeg) / MS) % (int)gridDim.y == by_);
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i;
      if (NX * 256 == XQ || idx < XQ) {
        const int mr = idx / (BKT / 4), kq = idx % (BKT / 4);
        const bool rok = (m0 + mr) < mend;
        f32x4 v = dl3_act4(xs4[i] * rx[i] + xt4[i], P.x_act);
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (!(rok && xok[i][j])) v[j] = 0.f;
        st4(&Xs[mr * LDX + kq * 4], v);
      }
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i;
      if (ND * 256 == DQ || idx < DQ) {
        const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
        const bool rok = (m0 + mr) < mend;
        f32x4 v = kA4[i] * rg[i] + kC4[i];
        if (two) v += kB4[i] * ry[i];
        if (dy_owner && rok) {
          float *dp = P.dyout + (size_t)(m0 + mr) * P.lddy + nbase + nq * 4;
          if (DVEC) {
            if (dok[i][0]) st4_nt(dp, v);
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (dok[i][j]) dp[j] = v[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (!(rok && dok[i][j])) v[j] = 0.f;
        st4(&Ds[mr * LDD + nq * 4], v);
      }
    }
  };

  if (mbeg < mend) {
    load_tiles(mbeg);
    store_tiles(mbeg, lds, lds + MS * LDX);
    __syncthreads();
    int stage = 0;
    for (int m0 = mbeg; m0 < mend; m0 += MS, stage ^= 1) {
      const float *Xs = lds + stage * STAGE;
      const float *Ds = Xs + MS * LDX;
      const bool more = (m0 + MS < mend);
      if (more) load_tiles(m0 + MS);
      if constexpr (SPL) {
        u32x4 ah[TA], am[TA], al[TA];
#pragma unroll
        for (int i = 0; i < TA; i++) {
          f32x4 v0, v1;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            v0[e] = Xs[(8 * lhi + e) * LDX + (wa * TA + i) * 32 + l31];
            v1[e] = Xs[(8 * lhi + 4 + e) * LDX + (wa * TA + i) * 32 + l31];
          }
          split3(v0, v1, ah[i], am[i], al[i]);
        }
#pragma unroll
        for (int j = 0; j < TB; j++) {
          f32x4 v0, v1;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            v0[e] = Ds[(8 * lhi + e) * LDD + (wb * TB + j) * 32 + l31];
            v1[e] = Ds[(8 * lhi + 4 + e) * LDD + (wb * TB + j) * 32 + l31];
          }
          u32x4 bh_, bm_, bl_;
          split3(v0, v1, bh_, bm_, bl_);
          const bf16x8 bh = __builtin_bit_cast(bf16x8, bh_), bm = __builtin_bit_cast(bf16x8, bm_),
                       bl = __builtin_bit_cast(bf16x8, bl_);
#pragma unroll
          for (int i = 0; i < TA; i++) {
            const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[i]), xm = __builtin_bit_cast(bf16x8, am[i]),
                         xl = __builtin_bit_cast(bf16x8, al[i]);
            f32x16 c = acc[i][j];  // small terms first
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm, bm, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bm, c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bh, c, 0, 0, 0);
          }
        }
        if (more) {
          float *Xn = lds + (stage ^ 1) * STAGE;
          store_tiles(m0 + MS, Xn, Xn + MS * LDX);
        }
        __syncthreads();
        continue;
      }
      float af[2][TA], bf[2][TB];
#pragma unroll
      for (int i = 0; i < TA; i++) af[0][i] = Xs[lhi * LDX + (wa * TA + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < TB; j++) bf[0][j] = Ds[lhi * LDD + (wb * TB + j) * 32 + l31];
#pragma unroll
      for (int ks = 0; ks < MS / 2; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < MS / 2) {
#pragma unroll
          for (int i = 0; i < TA; i++) af[nxt][i] = Xs[(2 * ks + 2 + lhi) * LDX + (wa * TA + i) * 32 + l31];
#pragma unroll
          for (int j = 0; j < TB; j++) bf[nxt][j] = Ds[(2 * ks + 2 + lhi) * LDD + (wb * TB + j) * 32 + l31];
        }
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
          for (int j = 0; j < TB; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
      }
      if (more) {
        float *Xn = lds + (stage ^ 1) * STAGE;
        store_tiles(m0 + MS, Xn, Xn + MS * LDX);
      }
      __syncthreads();
    }
  }
  float *out = P.ws + (size_t)bz * P.K * P.N;
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++) {
      const int col = nbase + (wb * TB + j) * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int krow = kbase + (wa * TA + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (krow < P.K && col < P.N) out[(size_t)krow * P.N + col] = acc[i][j][r];
      }
    }
}

// ---- round 6: the weight gradient of a layer whose whole reduction-side width fits ONE tile row (K <= 32 TA WA: the expand
// convolutions 96 -> 576 and 160 -> 960, deeplabv3p.py:175-178) — the HBM-heavy half of the family (a narrow x, a wide g / y,
// and the dY store on top: 3.4 - 3.9 TB/s in the tiled kernel).  One workgroup per row slab stages every dY stage exactly
// once, so the dY store needs no ownership at all and the stage loop is straight-line:
//   * the dY store (DYS) is a template parameter: every lane stores every piece (rows beyond M and column groups beyond N are clamped onto
//     valid ones: same address, same bits) — no store sits in a branch;
//   * the NEXT stage's operands are requested BEFORE this stage's stores: vmcnt retires in order and counts stores, so a
//     request issued behind a store cannot be waited for without waiting for the store; this way the wait is a counted
//     vmcnt(#stores) that leaves them in flight for a whole further stage (ISA: s_waitcnt vmcnt(2) in the loop);
//   * the per-column coefficient vectors live in LDS instead of 40-52 hoisted registers;
//   * waves whose 32-column blocks lie wholly beyond N (the half-empty last column tile of N = 960 / 576 on 128-wide
//     tiles) skip their MFMAs and leave the SIMD's matrix pipe to the co-resident workgroup.
// Same-box microbenchmark against pw_wgrad_kernel (profiles/r06_ab_calls.txt call 3): 96 -> 576 0.941 -> 0.860 ms, 160 -> 960
// 1.945 -> 1.841 ms.  With several workgroups per row slab (K > one tile row) the same structure LOST 2-9 % — whichever
// way the stores were shared out, the slab's workgroups fell out of step and re-read g / y from HBM instead of the XCD's
// L2 — so those launches stay on pw_wgrad_kernel.
template <int TA, int TB, int WA, int WB, bool DYS>
__global__ __launch_bounds__(256, 2) void pw_wgrad_row_kernel(WgradArgs P) {
  constexpr int VEC = 1;
  constexpr bool SPL = false;
  constexpr bool XVEC = VEC != 0, DVEC = VEC == 1;
  static_assert(WA * WB == 4, "4 waves per workgroup");
  // SPL: split math (see split3).  The reduction index is the pixel row, and a bf16 MFMA wants 8 CONSECUTIVE reduction
  // elements per lane: lane (column c, half h) gathers rows 8h..8h+7 of its column from the fp32 stage in LDS (the same
  // number of ds_read_b32 per pixel as the f32 MFMA's one-per-k-step), splits them in registers, and one 16-row stage is
  // one k-step of six bf16 MFMAs per 32x32 sub-tile.
  static_assert(!SPL || DL3_WGRAD_MS == 16, "split math: a stage is one 16-deep bf16 MFMA k-step");
  constexpr int BKT = 32 * TA * WA, BNT = 32 * TB * WB, MS = DL3_WGRAD_MS;
  constexpr int LDX = BKT + 4, LDD = BNT + 4;
  constexpr int XQ = MS * BKT / 4, DQ = MS * BNT / 4;  // float4s per stage
  constexpr int NX = (XQ + 255) / 256, ND = (DQ + 255) / 256;
  constexpr int STAGE = MS * LDX + MS * LDD;
  __shared__ float lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wa = wave / WB, wb = wave % WB;
  const int l31 = lane & 31, lhi = lane >> 5;
  // XCD-aware decode: the tiles of ONE row slab (same activations / gradients, different weight tiles) get consecutive
  // virtual ids and therefore one XCD and its L2.  With the plain (x, y, z) order consecutive tiles land on different
  // XCDs and every tile re-reads its slab from HBM (TCC hit rate 0-3 % measured; the 160x960 layer moved 2.5 GB instead
  // of 1.1 GB per launch and ran at HBM speed, not MFMA speed).
  const int nwg = gridDim.x * gridDim.y * gridDim.z;
  const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  const int vid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int bx = vid % gridDim.x, by_ = (vid / gridDim.x) % gridDim.y, bz = vid / (gridDim.x * gridDim.y);
  const int kbase = by_ * BKT, nbase = bx * BNT;
  const int mbeg = bz * P.Mper;
  const int mend = min(P.M, mbeg + P.Mper);
  const bool xform = (P.xs != nullptr);
  const bool two = (P.cA != nullptr);
  // 32 x 32 blocks of this wave's sub-tile that lie inside the K x N matrix (wave-uniform)
  const int ia = max(0, min(TA, (P.K - kbase - wa * TA * 32 + 31) >> 5));
  const int jb = max(0, min(TB, (P.N - nbase - wb * TB * 32 + 31) >> 5));
  const bool wfull = (ia == TA) && (jb == TB);

  f32x16 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // per-column coefficient vectors of the tile (input transform of x; BatchNorm-backward affine of g, y) live in LDS — as
  // hoisted registers they were 40-52 VGPRs of every instantiation (an occupancy step for the 128 x 96 / 128 x 128 tiles).
  // Columns beyond K / N carry the LAST valid column group's values shifted in: a lane whose 16-byte piece lies beyond N
  // works on a duplicate of the last valid group (load_tiles clamps it there) and must assemble the same bits for it.
  __shared__ __attribute__((aligned(16))) float cfx[2][BKT];
  __shared__ __attribute__((aligned(16))) float cfd[3][BNT];
  for (int c = tid; c < BKT; c += 256) {
    const int kc = min(kbase + c, P.K - 1);
    cfx[0][c] = xform ? P.xs[kc] : 1.f;
    cfx[1][c] = xform ? P.xt[kc] : 0.f;
  }
  for (int c = tid; c < BNT; c += 256) {
    const int cc = min(nbase + c, P.N - 1);
    cfd[0][c] = two ? P.cA[cc] : 1.f;
    cfd[1][c] = two ? P.cB[cc] : 0.f;
    cfd[2][c] = two ? P.cC[cc] : 0.f;
  }
  __syncthreads();

  f32x4 rx[NX], rg[ND], ry[ND];

  // requests of the stage that starts at row m0 (all unconditional: clamped rows / columns / piece indices)
  auto load_tiles = [&](int m0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = min(tid + 256 * i, XQ - 1);
      const int mr = idx / (BKT / 4), kq = idx % (BKT / 4);
      const int row = min(m0 + mr, P.M - 1), k = kbase + kq * 4;
      if (XVEC) {
        rx[i] = ld4(P.x + (size_t)row * P.ldx + min(k, P.K - 4));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) rx[i][j] = P.x[(size_t)row * P.ldx + min(k + j, P.K - 1)];
      }
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = min(tid + 256 * i, DQ - 1);
      const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
      const int row = min(m0 + mr, P.M - 1), col = nbase + nq * 4;
      if (DVEC) {
        const int cc = min(col, P.N - 4);
        rg[i] = ld4(P.g + (size_t)row * P.ldg + cc);
        if (two) ry[i] = ld4(P.y + (size_t)row * P.ldy + cc);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int cc = min(col + j, P.N - 1);
          rg[i][j] = P.g[(size_t)row * P.ldg + cc];
          if (two) ry[i][j] = P.y[(size_t)row * P.ldy + cc];
        }
      }
    }
  };

  // the loaded stage (rows m0 ..) -> MFMA operands in LDS [+ dY to HBM]; the requests of the stage at mnext are issued in
  // between: behind the last use of the registers they land in, in front of this stage's stores
  auto load_x = [&](int m0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = min(tid + 256 * i, XQ - 1);
      const int mr = idx / (BKT / 4), kq = idx % (BKT / 4);
      const int row = min(m0 + mr, P.M - 1), k = kbase + kq * 4;
      if (XVEC) {
        rx[i] = ld4(P.x + (size_t)row * P.ldx + min(k, P.K - 4));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) rx[i][j] = P.x[(size_t)row * P.ldx + min(k + j, P.K - 1)];
      }
    }
  };
  auto load_d = [&](int m0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = min(tid + 256 * i, DQ - 1);
      const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
      const int row = min(m0 + mr, P.M - 1), col = nbase + nq * 4;
      if (DVEC) {
        const int cc = min(col, P.N - 4);
        rg[i] = ld4(P.g + (size_t)row * P.ldg + cc);
        if (two) ry[i] = ld4(P.y + (size_t)row * P.ldy + cc);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int cc = min(col + j, P.N - 1);
          rg[i][j] = P.g[(size_t)row * P.ldg + cc];
          if (two) ry[i][j] = P.y[(size_t)row * P.ldy + cc];
        }
      }
    }
  };
  auto prepare = [&](int m0, int mnext, float *Xs, float *Ds, auto store_tag) __attribute__((always_inline)) {
    constexpr bool STORE = decltype(store_tag)::value;
    // x: transform -> LDS (not a vector-memory operation: it may sit anywhere), then its registers take the next stage's
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int idx = tid + 256 * i;
      const int mr = min(idx, XQ - 1) / (BKT / 4), kq = min(idx, XQ - 1) % (BKT / 4);
      const bool rok = (m0 + mr) < mend;
      const int kl = XVEC ? min(kbase + kq * 4, P.K - 4) - kbase : kq * 4;   // (the column group the load was clamped to)
      f32x4 v = dl3_act4(ld4(&cfx[0][kl]) * rx[i] + ld4(&cfx[1][kl]), P.x_act);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (!(rok && (kbase + kq * 4 + j) < P.K)) v[j] = 0.f;
      if (NX * 256 == XQ || idx < XQ) st4(&Xs[mr * LDX + kq * 4], v);
    }
    f32x4 td[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int nq_ = min(tid + 256 * i, DQ - 1) % (BNT / 4);
      const int nl = DVEC ? min(nbase + nq_ * 4, P.N - 4) - nbase : nq_ * 4;
      td[i] = ld4(&cfd[0][nl]) * rg[i] + ld4(&cfd[2][nl]);
      if (two) td[i] += ld4(&cfd[1][nl]) * ry[i];
    }
    __builtin_amdgcn_sched_barrier(0);
    load_x(mnext);
    load_d(mnext);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STORE) {
#pragma unroll
      for (int i = 0; i < ND; i++) {
        const int idx = min(tid + 256 * i, DQ - 1);
        const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
        if constexpr (DVEC) {
          float *dp = P.dyout + (size_t)min(m0 + mr, P.M - 1) * P.lddy + min(nbase + nq * 4, P.N - 4);
          st4_nt(dp, td[i]);
        } else {
          if (m0 + mr < mend) {
            float *dp = P.dyout + (size_t)(m0 + mr) * P.lddy + nbase + nq * 4;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if ((nbase + nq * 4 + j) < P.N) dp[j] = td[i][j];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int idx = tid + 256 * i;
      if (ND * 256 == DQ || idx < DQ) {
        const int mr = idx / (BNT / 4), nq = idx % (BNT / 4);
        const bool rok = (m0 + mr) < mend;
        f32x4 v = td[i];
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (!(rok && (nbase + nq * 4 + j) < P.N)) v[j] = 0.f;
        st4(&Ds[mr * LDD + nq * 4], v);
      }
    }
  };

  // the MFMAs of one staged 16-row slice
  auto mfma_stage = [&](const float *Xs, const float *Ds) __attribute__((always_inline)) {
    if constexpr (SPL) {
      u32x4 ah[TA], am[TA], al[TA];
#pragma unroll
      for (int i = 0; i < TA; i++) {
        f32x4 v0, v1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          v0[e] = Xs[(8 * lhi + e) * LDX + (wa * TA + i) * 32 + l31];
          v1[e] = Xs[(8 * lhi + 4 + e) * LDX + (wa * TA + i) * 32 + l31];
        }
        split3(v0, v1, ah[i], am[i], al[i]);
      }
#pragma unroll
      for (int j = 0; j < TB; j++) {
        f32x4 v0, v1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          v0[e] = Ds[(8 * lhi + e) * LDD + (wb * TB + j) * 32 + l31];
          v1[e] = Ds[(8 * lhi + 4 + e) * LDD + (wb * TB + j) * 32 + l31];
        }
        u32x4 bh_, bm_, bl_;
        split3(v0, v1, bh_, bm_, bl_);
        const bf16x8 bh = __builtin_bit_cast(bf16x8, bh_), bm = __builtin_bit_cast(bf16x8, bm_),
                     bl = __builtin_bit_cast(bf16x8, bl_);
#pragma unroll
        for (int i = 0; i < TA; i++) {
          const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[i]), xm = __builtin_bit_cast(bf16x8, am[i]),
                       xl = __builtin_bit_cast(bf16x8, al[i]);
          f32x16 c = acc[i][j];  // small terms first
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm, bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm, bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bm, c, 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, bh, c, 0, 0, 0);
        }
      }
    } else if (ia > 0 && jb > 0) {
      float af[2][TA], bf[2][TB];
#pragma unroll
      for (int i = 0; i < TA; i++) af[0][i] = Xs[lhi * LDX + (wa * TA + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < TB; j++) bf[0][j] = Ds[lhi * LDD + (wb * TB + j) * 32 + l31];
#pragma unroll
      for (int ks = 0; ks < MS / 2; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < MS / 2) {
#pragma unroll
          for (int i = 0; i < TA; i++) af[nxt][i] = Xs[(2 * ks + 2 + lhi) * LDX + (wa * TA + i) * 32 + l31];
#pragma unroll
          for (int j = 0; j < TB; j++) bf[nxt][j] = Ds[(2 * ks + 2 + lhi) * LDD + (wb * TB + j) * 32 + l31];
        }
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
          for (int j = 0; j < TB; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
      }
    }
  };

    if (mbeg < mend) {
    const int ns = (mend - mbeg + MS - 1) / MS;          // stages of this workgroup
    const int mlast = mbeg + (ns - 1) * MS;              // (the last stage asks for itself again instead of for nothing)
    auto stage_x = [&](int t) { return lds + (t & 1) * STAGE; };
    load_x(mbeg);
    load_d(mbeg);
    prepare(mbeg, min(mbeg + MS, mlast), stage_x(0), stage_x(0) + MS * LDX, std::integral_constant<bool, DYS>{});
    __syncthreads();
    // (requests in flight at the loop's entry would make its header the pessimistic merge of entry and back edge — every
    // wait inside vmcnt(0): wait once here)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int t = 1; t < ns; ++t) {
      mfma_stage(stage_x(t - 1), stage_x(t - 1) + MS * LDX);
      prepare(mbeg + t * MS, min(mbeg + (t + 1) * MS, mlast), stage_x(t), stage_x(t) + MS * LDX, std::integral_constant<bool, DYS>{});
      __syncthreads();
    }
    mfma_stage(stage_x(ns - 1), stage_x(ns - 1) + MS * LDX);
  }
  float *out = P.ws + (size_t)bz * P.K * P.N;
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++) {
      const int col = nbase + (wb * TB + j) * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int krow = kbase + (wa * TA + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (krow < P.K && col < P.N) out[(size_t)krow * P.N + col] = acc[i][j][r];
      }
    }
}

// column sums of dY over row ranges: partial [PR][N]; block = 64 columns x 4 row lanes
__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ g, int ldg, int M, int N,
                                                     float *__restrict__ part) {
  __shared__ float red[256];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  float s = 0.f;
  if (col < N)
    for (long m = (long)blockIdx.y * 4 + rl; m < M; m += (long)gridDim.y * 4) s += g[(size_t)m * ldg + col];
  red[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && col < N)
    part[(size_t)blockIdx.y * N + col] = ((red[cl] + red[64 + cl]) + red[128 + cl]) + red[192 + cl];
}

// bwd-weight: dW[K][N] = T(x)^T[K, M] . dY[M, N] (+ db[N] = column sums of dY) with N = classes <= 32 and K = 128 HB.  No LDS
// stage, no barrier in the loop: the reduction index of the MFMA is the pixel row, so a lane's A operand is x[row + lhi][its
// channel] — and WHICH channel an accumulator row stands for is ours to choose.  Lane (l31, lhi) requests 16 bytes at channel
// 128 h + 4 l31 of row r + lhi (a half-wave reads 512 contiguous bytes): element e of that piece is the A operand of block
// (h, e), whose accumulator row i is channel 128 h + 4 i + e.  Every 2-row k-step is HB 16-byte loads + one 4-byte load of dY
// and 4 HB MFMAs; a wave keeps all 4 HB accumulators (the whole K x 32 gradient), walks 4-row chunks chunk = gw, gw + GW, ...
// through a ring of D register slots (three chunks in flight while one is multiplied), and the NW waves of a workgroup meet
// in LDS once at the end, in wave order: one [K][N] slab (and one row of column sums) per workgroup.
template <int HB, int NW>
__global__ __launch_bounds__(64 * NW) void pw_wgrad_narrow_kernel(WgradArgs P, float *cpart) {
  constexpr int NB = 4 * HB, K = 128 * HB, D = 4;
  __shared__ __attribute__((aligned(16))) float red[NB * 16 * 64];   // the workgroup's sum, accumulator layout
  __shared__ __attribute__((aligned(16))) float cfx[2 * K];
  __shared__ float dbs[NW * 32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const bool xform = P.xs != nullptr;
  for (int i = tid; i < K; i += 64 * NW) {
    cfx[i] = xform ? P.xs[i] : 1.f;
    cfx[K + i] = xform ? P.xt[i] : 0.f;
  }
  __syncthreads();
  const int nchunks = (P.M + 3) >> 2;
  const int gw = blockIdx.x * NW + wave, GW = gridDim.x * NW;
  const int gcol = min(l31, P.N - 1);
  const float colmask = l31 < P.N ? 1.f : 0.f;
  f32x16 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[b][r] = 0.f;
  float gsum = 0.f;
  f32x4 xr[D][2][HB];
  float gr[D][2];
  auto req = [&](int c, int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const int row = min(4 * c + 2 * ks + lhi, P.M - 1);   // (rows beyond M: a valid row, masked when it is multiplied)
      const float *xp = P.x + (size_t)row * P.ldx + 4 * l31;
#pragma unroll
      for (int h = 0; h < HB; h++) xr[sl][ks][h] = ld4(xp + 128 * h);
      gr[sl][ks] = P.g[(size_t)row * P.ldg + gcol];
    }
  };
  auto multiply = [&](int c, int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const float gv = (4 * c + 2 * ks + lhi < P.M) ? gr[sl][ks] * colmask : 0.f;
      gsum += gv;
#pragma unroll
      for (int h = 0; h < HB; h++) {
        // (scale 1, shift 0 without a BatchNorm: an activation-only view is still rectified)
        const f32x4 v = dl3_act4(ld4(cfx + 128 * h + 4 * l31) * xr[sl][ks][h] + ld4(cfx + K + 128 * h + 4 * l31), P.x_act);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[4 * h + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], gv, acc[4 * h + e], 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int d = 0; d < D; d++) req(gw + d * GW, d);
  for (int c = gw; c < nchunks; c += D * GW) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      multiply(c + d * GW, d);
      __builtin_amdgcn_sched_barrier(0);
      req(c + (d + D) * GW, d);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the NW waves' accumulators, in wave order
  for (int w = 0; w < NW; w++) {
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int i = (b * 16 + r) * 64 + lane;
          red[i] = (w == 0 ? 0.f : red[i]) + acc[b][r];
        }
    }
    __syncthreads();
  }
  gsum += __shfl_xor(gsum, 32, 64);
  if (lhi == 0) dbs[wave * 32 + l31] = gsum;
  float *slab = P.ws + (size_t)blockIdx.x * K * P.N;
  for (int i = tid; i < K * P.N; i += 64 * NW) {
    const int ch = i / P.N, n = i - ch * P.N;
    const int h = ch >> 7, ii = (ch & 127) >> 2, e = ch & 3;
    const int r = (ii & 3) + 4 * (ii >> 3), hi = (ii >> 2) & 1;
    slab[i] = red[((4 * h + e) * 16 + r) * 64 + hi * 32 + n];
  }
  __syncthreads();
  if (cpart && tid < P.N) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w++) a += dbs[w * 32 + tid];
    cpart[(size_t)blockIdx.x * P.N + tid] = a;
  }
}
}  // namespace

// (tests/test_pwconv_cases_host.py::test_universe_restates_the_launchers reads this switch as text and tests/pwconv_cases.py universe()
// lists its instantiations: an instantiation added, dropped or renamed here is added there, with a case that reaches it)
void pw::launch_wgrad(const WgradArgs &A, const WgradPlan &P, float *cpart, void *stream) {
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(P.grid[0], P.grid[1], P.grid[2]), blk(256);
  if (P.narrow) {
    hipLaunchKernelGGL((pw_wgrad_narrow_kernel<2, DL3_WS2_NW>), grid, dim3(64 * DL3_WS2_NW), 0, st, A, cpart);
    return;
  }
#define DL3_GO(KERNEL_) hipLaunchKernelGGL((KERNEL_), grid, blk, 0, st, A)
  if (P.row) {   // (cfg 2 or 8, 16-byte loads on both operands: wgrad_row_ok)
    if (P.cfg == 2) {
      if (A.dyout) DL3_GO((pw_wgrad_row_kernel<5, 1, 1, 4, true>));
      else DL3_GO((pw_wgrad_row_kernel<5, 1, 1, 4, false>));
    } else {
      if (A.dyout) DL3_GO((pw_wgrad_row_kernel<3, 1, 1, 4, true>));
      else DL3_GO((pw_wgrad_row_kernel<3, 1, 1, 4, false>));
    }
    return;
  }
#define DL3_WG(TA_, TB_, WA_, WB_)                                                            \
  do {                                                                                        \
    if (P.vec == 1 && P.split) DL3_GO((pw_wgrad_kernel<TA_, TB_, WA_, WB_, 1, true>));        \
    else if (P.vec == 1) DL3_GO((pw_wgrad_kernel<TA_, TB_, WA_, WB_, 1>));                    \
    else if (P.vec == 2) DL3_GO((pw_wgrad_kernel<TA_, TB_, WA_, WB_, 2>));                    \
    else DL3_GO((pw_wgrad_kernel<TA_, TB_, WA_, WB_, 0>));                                    \
  } while (0)
  switch (P.cfg) {
    case 0: DL3_WG(1, 1, 2, 2); break;
    case 1: DL3_WG(2, 2, 2, 2); break;
    case 2: DL3_WG(5, 1, 1, 4); break;
    case 3: DL3_WG(1, 5, 4, 1); break;
    case 4: DL3_WG(2, 1, 1, 4); break;
    case 5: DL3_WG(1, 2, 4, 1); break;
    case 6: DL3_WG(1, 1, 1, 4); break;
    case 7: DL3_WG(1, 1, 4, 1); break;
    case 8: DL3_WG(3, 1, 1, 4); break;
    default: DL3_WG(1, 3, 4, 1); break;
  }
#undef DL3_WG
#undef DL3_GO
}

void pw::launch_colsum(const float *g, int ldg, int M, int N, int rows, float *part, void *stream) {
  hipLaunchKernelGGL(colsum_kernel, dim3(dl3_cdiv(N, 64), rows), dim3(256), 0, (hipStream_t)stream, g, ldg, M, N, part);
}
