// pwws.hip — the weight-stationary kernels of the 1x1-convolution GEMMs: the whole weight slice of a workgroup stays in LDS and
// every wave walks 32-row tiles on its own.  PW_WS (the HBM-bound early layers, forward), PW_WS2 (the MFMA-bound short
// reductions, forward and bwd-data), PW_NARROW_FLAT and PW_NARROWK (the logits layer).  Fragment layouts: pwgemm.hip.
#include "common.h"
#include "pwargs.h"
namespace {
using pw::GemmArgs;

// ---- round 5: weight-stationary streaming forward kernel for the HBM-bound layers ---------------------------------------
// The expand / project convolutions of the first blocks (deeplabv3p.py:175-198: 16..192 channels on 256x256 .. 64x64 maps)
// carry 5-14 FLOP per byte: they are streaming kernels, and the tiled GEMM (pwstream.hip) runs them at 2.3-4.6 TB/s (24 -> 144 at
// 0.29 of the HBM peak) because a 128- or 256-row tile of a reduction of 16..32 is all prologue and epilogue — one or two
// K-tiles, a weight tile re-staged per row tile, 16 four-byte stores per 32x32 sub-tile and lane, three column tiles
// re-reading the rows.  Here the WHOLE weight matrix sits in LDS for the life of the workgroup (K x N <= 6 blocks of
// 32 x 32), and every WAVE walks 32-row tiles on its own — no barrier in the loop:
//   * the lane (row l & 31, half l >> 5) loads its K/2 consecutive floats of the NEXT tile (K/8 16-byte loads) while the
//     current one is in the matrix pipe; with 3-4 workgroups per CU that keeps 12-16 tiles in flight per CU;
//   * the producer's BatchNorm + ReLU6 is applied in registers, coefficient vectors in LDS;
//   * K/2 x TN MFMAs (v_mfma_f32_32x32x2_f32) against B fragments read from LDS (32 consecutive floats per half-wave:
//     conflict-free);
//   * epilogue per 32-column block: bias, BatchNorm partial sums (per lane: its column), then the block goes through a
//     4 KB per-wave LDS tile and leaves as 16-byte non-temporal stores — 4 instead of 16 store instructions per lane and
//     block, 128 contiguous bytes per row and instruction (the epilogue of an HBM-bound kernel is store-ISSUE-bound).
// Tile -> wave assignment is static (tile t belongs to wave t mod 4G): the statistic partial rows are deterministic.
// KQ = K / 8 (16-byte loads per lane and tile), TN = ceil(N / 32).
template <int KQ, int TN, int OC>
__global__ __launch_bounds__(256, OC) void pw_fwd_ws_kernel(GemmArgs P) {
  constexpr int KH = 4 * KQ, K = 8 * KQ, NP = 32 * TN;
  __shared__ float Ws[K * NP];        // W[k][n], zero beyond N
  __shared__ float cf[2 * K];         // scale | shift of the input transform
  __shared__ float bs[NP];            // bias
  __shared__ float Cs[4 * 1024];      // per wave: one 32x32 block on its way out; at the end: the statistic fold
  // gfx950 only: <4,6,3> keeps 41 KB per workgroup at 3 workgroups per CU (160 KB LDS); a 64 KB-LDS part would get one
  static_assert(sizeof(float) * (K * NP + 2 * K + NP + 4 * 1024) * OC <= 160 * 1024, "weight-stationary kernel: OC workgroups do not fit a gfx950 CU's LDS");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const bool xform = (P.ka != nullptr);

  for (int i = tid; i < K * NP; i += 256) {
    const int k = i / NP, n = i % NP;
    Ws[i] = n < P.N ? P.b[(size_t)k * P.ldb + n] : 0.f;
  }
  for (int i = tid; i < K; i += 256) {
    cf[i] = xform ? P.ka[i] : 1.f;
    cf[K + i] = xform ? P.kc[i] : 0.f;
  }
  for (int i = tid; i < NP; i += 256) bs[i] = (P.bias && i < P.N) ? P.bias[i] : 0.f;
  float st1[TN], st2[TN];
#pragma unroll
  for (int j = 0; j < TN; j++) st1[j] = st2[j] = 0.f;
  __syncthreads();

  const int nfull = P.M >> 5;  // whole 32-row tiles: the loop below; a ragged last tile is handled behind it
  const int gw = blockIdx.x * 4 + wave, GW = gridDim.x * 4;
  float *const cw = Cs + wave * 1024;
  const float *const wfrag = Ws + KH * lhi * NP + l31;
  const float *const cfs = cf + KH * lhi, *const cft = cf + K + KH * lhi;
  // 16-byte stores: lane -> (row r0 + 8 p, columns c4 .. c4 + 3) of a 32x32 block.  In the last block only N - 32 (TN - 1)
  // columns exist: the lanes beyond them repeat a valid column group (same address, same data) instead of being
  // predicated off, so that EVERY lane issues every store: with a fixed number of stores per tile the wait for the next
  // tile's rows is a counted s_waitcnt vmcnt(stores) — a branch around a store makes it vmcnt(0), i.e. every wave
  // drains its own stores (microseconds under load) once per tile.
  const int c4 = (lane & 7) * 4, r0 = lane >> 3;
  const int c4l = c4 % (P.N - 32 * (TN - 1));

  f32x4 nx[KQ];
  auto load_tile = [&](int t) {
    const int row = min(t * 32 + l31, P.M - 1);
    const float *p = P.a + (size_t)row * P.lda + KH * lhi;
#pragma unroll
    for (int j = 0; j < KQ; j++) nx[j] = ld4(p + 4 * j);
  };
  // MFMAs of the tile whose rows are in nx; then, the registers being free again, ALL K/8 requests of tile `next` (>= 0) —
  // in front of this tile's stores, so that the wait for them at the next tile's start is a counted one.  (Requested a
  // whole tile ahead through a second register set — measured: no faster for K <= 32, spills from K = 96; left alone the
  // scheduler sinks the requests between the MFMAs one by one to save registers — twelve exposed round trips per tile.)
  auto mfma_tile = [&](f32x16 (&acc)[TN], int next) {
#pragma unroll
    for (int q = 0; q < KQ; q++) {
      const f32x4 v = dl3_act4(ld4(cfs + 4 * q) * nx[q] + ld4(cft + 4 * q), P.a_act);
#pragma unroll
      for (int e = 0; e < 4; e++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], wfrag[(4 * q + e) * NP + j * 32], acc[j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (next >= 0) load_tile(next);
    __builtin_amdgcn_sched_barrier(0);
  };

  if (gw < nfull) load_tile(gw);
  // (the first tile's rows are waited for HERE: entering the loop with requests in flight and no stores behind them, the
  // compiler has to merge that state with the back edge's — requests followed by 4 TN stores — and settles for vmcnt(0))
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int t = gw; t < nfull; t += GW) {
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    mfma_tile(acc, t + GW < nfull ? t + GW : -1);
    float *const cp = P.c + (size_t)(t * 32 + r0) * P.ldc;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const float bj = bs[j * 32 + l31];
      // BatchNorm partial sums of this lane's column; C layout (row (r & 3) + 8 (r >> 2) + 4 lhi, column l31) -> rows of
      // 32 floats in LDS -> 16 bytes per lane
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float v = acc[j][r] + bj;
        st1[j] += v;
        st2[j] += v * v;
        cw[((r & 3) + 8 * (r >> 2) + 4 * lhi) * 32 + l31] = v;
      }
      __builtin_amdgcn_wave_barrier();
      const int cc = (j == TN - 1) ? c4l : c4;
      f32x4 o[4];
#pragma unroll
      for (int p = 0; p < 4; p++) o[p] = ld4(cw + (r0 + 8 * p) * 32 + cc);
#pragma unroll
      for (int p = 0; p < 4; p++) st4_nt(cp + (size_t)(8 * p) * P.ldc + j * 32 + cc, o[p]);
      __builtin_amdgcn_wave_barrier();
    }
  }
  if ((P.M & 31) != 0 && gw == nfull % GW) {
    // the one ragged tile of the launch: every element predicated
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    load_tile(nfull);
    mfma_tile(acc, -1);
    const int m0 = nfull * 32;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col = j * 32 + l31;
      const float bj = bs[col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        const float v = acc[j][r] + bj;
        if (row < P.M && col < P.N) {
          st1[j] += v;
          st2[j] += v * v;
          P.c[(size_t)row * P.ldc + col] = v;
        }
      }
    }
  }

  if (P.stat_mode != 0) {
    // half-waves, then the four waves in wave order: one partial row per workgroup
    __syncthreads();
    float *sred = Cs;  // [4][NP][2] (NP <= 192: 6 KB)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const float a1 = st1[j] + __shfl_xor(st1[j], 32, 64), a2 = st2[j] + __shfl_xor(st2[j], 32, 64);
      if (lhi == 0) {
        sred[(wave * NP + j * 32 + l31) * 2 + 0] = a1;
        sred[(wave * NP + j * 32 + l31) * 2 + 1] = a2;
      }
    }
    __syncthreads();
    for (int cl = tid; cl < NP; cl += 256) {
      if (cl < P.N) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          a1 += sred[(w * NP + cl) * 2 + 0];
          a2 += sred[(w * NP + cl) * 2 + 1];
        }
        P.part[((size_t)blockIdx.x * P.N + cl) * 2 + 0] = a1;
        P.part[((size_t)blockIdx.x * P.N + cl) * 2 + 1] = a2;
        for (int r = blockIdx.x + (int)gridDim.x; r < P.part_rows; r += (int)gridDim.x) {
          P.part[((size_t)r * P.N + cl) * 2 + 0] = 0.f;
          P.part[((size_t)r * P.N + cl) * 2 + 1] = 0.f;
        }
      }
    }
  }
}

// ---- round 6: weight-stationary GEMM for the MFMA-bound short reductions ------------------------------------------------
// The expand convolutions forward / the project convolutions' bwd-data (deeplabv3p.py:175-198: reduction 64 / 96 / 160 into a
// 384 / 576 / 960-wide output at 64 x 64) spend a third of every row tile outside the K loop in the tiled stream kernel: ten
// K-tiles of a reduction of 160 are 25 us of MFMAs between a prologue (first operand round trip, two barriers) and an
// epilogue of 6-8 us during which the wave issues none (DESIGN.md, round 3 phase table: matrix pipe 71 % / 50 % busy).
// Here a workgroup of NW = 8 waves keeps its WHOLE weight slice W[K][32 TN] in LDS for its lifetime (102 KB at K = 160,
// TN = 5: one workgroup per CU, two waves per SIMD) and every wave walks 32-row tiles on its own, like pw_fwd_ws_kernel: all
// K/8 16-byte requests of a tile up front (the lane's half of its row: K/2 registers), K/2 x TN MFMAs against fragments read
// straight from the resident slice — no weight staging, no barrier anywhere in the loop — then the epilogue, block by block
// through a per-wave LDS square (16-byte stores of whole rows).  The two waves of a SIMD drift apart by themselves: while one
// is in its epilogue or waits for its rows, the other one owns the matrix pipe.
// BWD: the bwd-data instantiation (dX = dY . W^T with the single-tensor dY the weight-gradient launch materialised): no operand
// transform; the epilogue multiplies by the activation mask of the forward input x and reduces the BatchNorm-backward sums
// sum(v), sum(v * x_hat).  Both need x element by element — it is requested 16 bytes at a time in the SAME row-piece layout the
// output leaves in (block j + 1's pieces while block j is finished), and the sums are kept per lane for its four columns,
// folded over the eight row lanes once at the end.
// TWO (BWD only): the two-tensor gradient operand dY = cA*g + cB*y + cC assembled on load — the expand convolutions 64 -> 384,
// whose weight-gradient launch writes no dY (a narrow x against a wide dY: the store does not pay, round 4): reduction 384
// into a 64-wide gradient, HBM-bound, 98 KB of W^T resident.  ADD (BWD only): a residual gradient joins in the epilogue
// (requested in the same row-piece layout as the forward input).
// FLAT (forward only, one column block): the logits layer (deeplabv3p.py:438) — N = classes <= 32 columns, rows of N floats
// back to back (ldc == N, N any number): a 32-row tile of the output is ONE contiguous run of 128 N bytes, which starts on a
// 16-byte boundary whatever N is.  The block goes through the wave's LDS square packed N floats per row and leaves as 8 N
// 16-byte pieces — the tiled kernel's scalar stores into 84-byte rows were what held this HBM-bound launch at 0.40 of peak.
#ifndef DL3_WS2_XPRE_TN
#define DL3_WS2_XPRE_TN 4
#endif
template <int KQ, int TN, int NW, bool BWD = false, bool TWO = false, bool ADD = false, bool FLAT = false>
__global__ __launch_bounds__(64 * NW) void pw_ws2_kernel(GemmArgs P) {
  static_assert(BWD || (!TWO && !ADD), "two-tensor operand / residual addend: bwd-data only");
  static_assert(!FLAT || (!BWD && TN == 1), "packed narrow output: forward, one column block");
  constexpr bool XPRE = BWD && !TWO && TN <= DL3_WS2_XPRE_TN;   // the epilogue's forward-input pieces requested two column blocks ahead (below)
  constexpr int KH = 4 * KQ, K = 8 * KQ, NP = 32 * TN;
  __shared__ __attribute__((aligned(16))) float Ws[K * NP];   // W[k][n0 + n], zero beyond N
  __shared__ __attribute__((aligned(16))) float cf[(TWO ? 3 : 2) * K];    // scale | shift of the input transform (TWO: cA | cC | cB)
  __shared__ __attribute__((aligned(16))) float bs[BWD ? 4 * NP : NP];   // bias | BWD: mask scale, mask shift, mean, 1 / sigma of x
  __shared__ __attribute__((aligned(16))) float Cs[NW * 1024];  // per wave: one 32x32 block on its way out; at the end: the statistic fold
  static_assert(sizeof(float) * (K * NP + 3 * K + 4 * NP + NW * 1024) <= 160 * 1024, "gfx950: 160 KB of LDS per CU");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  // XCD-aware decode: the column tiles of one row group walk the same rows at the same time — one XCD, one L2
  const int nwg = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = b & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (b >> 3);
  const int ct = lid % gridDim.x, rg = lid / gridDim.x, nrg = gridDim.y;
  const int n0 = ct * NP;
  const bool xform = (P.ka != nullptr);

  for (int i = tid; i < K * NP; i += 64 * NW) {
    const int k = i / NP, n = n0 + i % NP;
    Ws[i] = n < P.N ? P.b[(size_t)k * P.ldb + n] : 0.f;
  }
  for (int i = tid; i < K; i += 64 * NW) {
    cf[i] = xform ? P.ka[i] : 1.f;
    cf[K + i] = xform ? P.kc[i] : 0.f;
    if constexpr (TWO) cf[2 * K + i] = P.kb[i];
  }
  for (int i = tid; i < NP; i += 64 * NW) {
    const int col = min(n0 + i, P.N - 1);
    if constexpr (BWD) {
      bs[i] = P.ep_scale ? P.ep_scale[col] : 1.f;
      bs[NP + i] = P.ep_scale ? P.ep_shift[col] : 0.f;
      bs[2 * NP + i] = P.stat_mode == 2 ? P.ep_mean[col] : 0.f;
      bs[3 * NP + i] = P.stat_mode == 2 ? P.ep_invstd[col] : 0.f;
    } else {
      bs[i] = (P.bias && n0 + i < P.N) ? P.bias[n0 + i] : 0.f;
    }
  }
  float st1[TN], st2[TN];
#pragma unroll
  for (int j = 0; j < TN; j++) st1[j] = st2[j] = 0.f;
  f32x4 q1[BWD ? TN : 1], q2[BWD ? TN : 1];   // BWD: the lane's sums for the four columns of its pieces, per column block
  if constexpr (BWD) {
#pragma unroll
    for (int j = 0; j < TN; j++) q1[j] = q2[j] = splat4(0.f);
  }
  __syncthreads();

  const int nfull = P.M >> 5;
  const int gw = rg * NW + wave, GW = nrg * NW;
  float *const cw = Cs + wave * 1024;
  const float *const wfrag = Ws + KH * lhi * NP + l31;
  const float *const cfs = cf + KH * lhi, *const cft = cf + K + KH * lhi;
  const int c4 = (lane & 7) * 4, r0 = lane >> 3;
  const int ncol = min(NP, P.N - n0);                   // columns of this tile inside the matrix (a multiple of 4; FLAT: any)
  const int jl = (ncol - 1) >> 5;                        // its last column block
  const int c4l = FLAT ? 0 : c4 % (ncol - 32 * jl);      // lanes beyond the last block's columns repeat a valid column group

  // The lane's K/2 operand values arrive as a stream of NCH chunks per tile through a ring of two register slots: while the
  // MFMAs of chunk c run, chunk c + 1 is in flight and chunk c + 2 — of this tile or, behind its last two chunks, of the wave's
  // NEXT tile — is requested as soon as slot c & 1 has been read.  The stream never drains at a tile boundary: the next tile's
  // first two chunks are requested before this tile's epilogue (and in front of its stores: counted waits).
  // chunks per tile (even: the slot of a chunk is c & 1 in every tile).  BWD: two pieces per chunk — its epilogue needs the
  // registers (the forward-input pieces of two column blocks, the per-column sums)
  constexpr int NCH = BWD ? KQ / 2 : 4;
  static_assert(NCH % 2 == 0, "an even number of chunks per tile");
  constexpr int SQ = KQ / NCH;                       // 16-byte pieces per chunk
  static_assert(KQ % NCH == 0, "the reduction must split into an even number of equal chunks");
  f32x4 nx[2][SQ], ny[2][TWO ? SQ : 1];
  auto req = [&](int t, int c, int sl) __attribute__((always_inline)) {
    const int row = min(t * 32 + l31, P.M - 1);
    const float *p = P.a + (size_t)row * P.lda + KH * lhi + 4 * SQ * c;
#pragma unroll
    for (int j = 0; j < SQ; j++) nx[sl][j] = ld4(p + 4 * j);
    if constexpr (TWO) {
      const float *p2 = P.a2 + (size_t)row * P.lda2 + KH * lhi + 4 * SQ * c;
#pragma unroll
      for (int j = 0; j < SQ; j++) ny[sl][j] = ld4(p2 + 4 * j);
    }
  };
  // tile t: its chunks 0 and 1 are in flight (or landed) on entry; tn = the wave's next tile (itself again at the end:
  // harmless duplicate requests instead of a branch around requests).  The B fragments of k-step s + 1 are read from the
  // resident slice while the TN MFMAs of k-step s run (two register sets, the order pinned with sched_group_barrier: left
  // alone the scheduler sinks every ds_read next to its MFMA — read, s_waitcnt lgkmcnt(0), two MFMAs — and with eight
  // waves on the LDS that round trip is longer than the two MFMAs)
  auto mfma_tile = [&](f32x16 (&acc)[TN], int t, int tn) __attribute__((always_inline)) {
    float bf[2][TN];
#pragma unroll
    for (int j = 0; j < TN; j++) bf[0][j] = wfrag[j * 32];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
#pragma unroll
      for (int q = 0; q < SQ; q++) {
        const int kq = SQ * c + q;
        f32x4 v;
        if constexpr (TWO) {
          v = ld4(cfs + 4 * kq) * nx[c & 1][q] + ld4(cft + 4 * kq);
          v += ld4(cf + 2 * K + KH * lhi + 4 * kq) * ny[c & 1][q];
        } else if constexpr (BWD) {
          v = nx[c & 1][q];
        } else {
          v = dl3_act4(ld4(cfs + 4 * kq) * nx[c & 1][q] + ld4(cft + 4 * kq), P.a_act);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int ks = 4 * kq + e, cur = ks & 1;
          if (ks + 1 < KH) {
#pragma unroll
            for (int j = 0; j < TN; j++) bf[cur ^ 1][j] = wfrag[(ks + 1) * NP + j * 32];
          }
#pragma unroll
          for (int j = 0; j < TN; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], bf[cur][j], acc[j], 0, 0, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, TN, 0);   // TN LDS reads (k-step s + 1) ...
          __builtin_amdgcn_sched_group_barrier(0x008, TN, 0);   // ... then the TN MFMAs of k-step s
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (c + 2 < NCH) req(t, c + 2, c & 1);
      else req(tn, c + 2 - NCH, c & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  if (gw < nfull) {
    req(gw, 0, 0);
    req(gw, 1, 1);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int t = gw; t < nfull; t += GW) {
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    // BWD, XPRE: the forward-input (and addend) pieces of the first TWO column blocks are requested in front of the tile's MFMAs
    // (they retire before the operand ring's requests: in-order vmcnt) and block j + 2's as soon as block j has used its slot —
    // the epilogue runs two blocks ahead of its HBM round trip instead of one, which a block's own ~1 us of work did not cover
    // (same-call A/B, 524 288 rows: 576 <- 96 0.737 -> 0.703 ms, 384 <- 96 0.495 -> 0.471, 384 <- 64 0.392 -> 0.383).  Not at
    // TN = 5 and not for the two-tensor operand: 32 more live registers across the MFMA loop spill there (144 -> 236 B of scratch,
    // 960 <- 160 1.93 -> 1.99 ms; 64 <- 384 0.505 -> 0.516)
    f32x4 xq[BWD ? 2 : 1][BWD ? 4 : 1], aq[BWD ? 2 : 1][ADD ? 4 : 1];
    if constexpr (XPRE) {
      int le = lane, c4le = c4l;   // (laundered like the epilogue's: see there)
      asm volatile("" : "+v"(le), "+v"(c4le));
      const int c4 = (le & 7) * 4, r0 = le >> 3, c4l = c4le;
      const float *const xp0 = P.ep_x + (size_t)(t * 32 + r0) * P.ld_epx + n0;
      const float *const ap0 = ADD ? P.ep_add + (size_t)(t * 32 + r0) * P.ld_add + n0 : nullptr;
#pragma unroll
      for (int jj = 0; jj < (TN < 2 ? TN : 2); jj++) {
        // (a block beyond the tile's last one: block jl's columns again — a valid address, never used)
        const int cc_ = jj < jl ? jj * 32 + c4 : jl * 32 + c4l;
#pragma unroll
        for (int p = 0; p < 4; p++) {
          xq[jj][p] = ld4(xp0 + (size_t)(8 * p) * P.ld_epx + cc_);
          if constexpr (ADD) aq[jj][p] = ld4(ap0 + (size_t)(8 * p) * P.ld_add + cc_);
        }
      }
    }
    mfma_tile(acc, t, t + GW < nfull ? t + GW : t);
    // every block leaves through the wave's LDS square as 16-byte stores of whole rows (4-byte stores straight from the accumulator
    // layout, two 128-byte row segments per instruction and no LDS round trip, measured slower: 160 -> 960 at 524 288 rows 1.51 -> 1.59 ms)
    if constexpr (BWD) {
      // The epilogue's lane-derived addresses depend only on the lane: left alone, the scheduler computes them once in front of
      // the tile loop and — at TN = 5, 256 registers — parks 25 of them in scratch, reloaded here tile after tile.  Laundering
      // the lane id through an empty asm behind the last MFMA makes them a handful of VALU instructions per tile instead.
      int le = lane, c4le = c4l;
      asm volatile("" : "+v"(le), "+v"(c4le));
      const int c4 = (le & 7) * 4, r0 = le >> 3, l31 = le & 31, lhi = le >> 5, c4l = c4le;
      float *const cp = P.c + (size_t)(t * 32 + r0) * P.ldc + n0;
      const float *const xp = P.ep_x + (size_t)(t * 32 + r0) * P.ld_epx + n0;
      const float *const ap = ADD ? P.ep_add + (size_t)(t * 32 + r0) * P.ld_add + n0 : nullptr;
      if constexpr (!XPRE) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
          xq[0][p] = ld4(xp + (size_t)(8 * p) * P.ld_epx + (0 == jl ? c4l : c4));
          if constexpr (ADD) aq[0][p] = ld4(ap + (size_t)(8 * p) * P.ld_add + (0 == jl ? c4l : c4));
        }
      }
#pragma unroll
      for (int j = 0; j < TN; j++) {
        if (j <= jl) {
          if (!XPRE && j + 1 <= jl) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
              xq[(j + 1) & 1][p] = ld4(xp + (size_t)(8 * p) * P.ld_epx + (j + 1) * 32 + (j + 1 == jl ? c4l : c4));
              if constexpr (ADD) aq[(j + 1) & 1][p] = ld4(ap + (size_t)(8 * p) * P.ld_add + (j + 1) * 32 + (j + 1 == jl ? c4l : c4));
            }
          }
#pragma unroll
          for (int r = 0; r < 16; r++) cw[((r & 3) + 8 * (r >> 2) + 4 * lhi) * 32 + l31] = acc[j][r];
          __builtin_amdgcn_wave_barrier();
          const int cc = (j == jl) ? c4l : c4;
          const f32x4 es = ld4(bs + j * 32 + cc), et = ld4(bs + NP + j * 32 + cc);
          const f32x4 mu = ld4(bs + 2 * NP + j * 32 + cc), is = ld4(bs + 3 * NP + j * 32 + cc);
          // (a lane that repeats a column group — cc != c4 in the last block — stores duplicates but must not count them)
          const float own = (cc == c4) ? 1.f : 0.f;
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const f32x4 x = xq[j & 1][p];
            f32x4 o = ld4(cw + (r0 + 8 * p) * 32 + cc) * dl3_mask4(es * x + et, P.ep_act);
            if constexpr (ADD) o += P.add_scale * aq[j & 1][p];
            st4_nt(cp + (size_t)(8 * p) * P.ldc + j * 32 + cc, o);
            q1[j] += own * o;
            q2[j] += own * (o * ((x - mu) * is));
          }
          if (XPRE && j + 2 <= jl) {   // (slot j & 1 is free again: block j + 2)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < 4; p++) {
              xq[j & 1][p] = ld4(xp + (size_t)(8 * p) * P.ld_epx + (j + 2) * 32 + (j + 2 == jl ? c4l : c4));
              if constexpr (ADD) aq[j & 1][p] = ld4(ap + (size_t)(8 * p) * P.ld_add + (j + 2) * 32 + (j + 2 == jl ? c4l : c4));
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    } else if constexpr (FLAT) {
      const float bj = bs[l31];
      float *const cq = cw + 4 * lhi * P.N + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float v = acc[0][r] + bj;
        st1[0] += v;
        st2[0] += v * v;
        if (l31 < P.N) cq[((r & 3) + 8 * (r >> 2)) * P.N] = v;
      }
      __builtin_amdgcn_wave_barrier();
      float *const cp = P.c + (size_t)t * 32 * P.N;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const int piece = lane + 64 * p;
        if (piece < 8 * P.N) st4_nt(cp + 4 * piece, ld4(cw + 4 * piece));
      }
      __builtin_amdgcn_wave_barrier();
    } else {
    float *const cp = P.c + (size_t)(t * 32 + r0) * P.ldc + n0;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      if (j <= jl) {   // (workgroup-uniform: column blocks wholly beyond N — only in the last column tile — are skipped)
        const float bj = bs[j * 32 + l31];
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float v = acc[j][r] + bj;
          st1[j] += v;
          st2[j] += v * v;
          cw[((r & 3) + 8 * (r >> 2) + 4 * lhi) * 32 + l31] = v;
        }
        __builtin_amdgcn_wave_barrier();
        const int cc = (j == jl) ? c4l : c4;
        f32x4 o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) o[p] = ld4(cw + (r0 + 8 * p) * 32 + cc);
#pragma unroll
        for (int p = 0; p < 4; p++) st4_nt(cp + (size_t)(8 * p) * P.ldc + j * 32 + cc, o[p]);
        __builtin_amdgcn_wave_barrier();
      }
    }
    }
  }
  if ((P.M & 31) != 0 && gw == nfull % GW) {
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    __builtin_amdgcn_s_waitcnt(0x0F70);
    req(nfull, 0, 0);
    req(nfull, 1, 1);
    mfma_tile(acc, nfull, nfull);
    const int m0 = nfull * 32;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col = n0 + j * 32 + l31;
      const float bj = BWD ? 0.f : bs[j * 32 + l31];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        float v = acc[j][r] + bj;
        if (row < P.M && col < P.N) {
          if constexpr (BWD) {
            const float x = P.ep_x[(size_t)row * P.ld_epx + col];
            v *= dl3_act_mask(bs[j * 32 + l31] * x + bs[NP + j * 32 + l31], P.ep_act);
            if constexpr (ADD) v += P.add_scale * P.ep_add[(size_t)row * P.ld_add + col];
            st1[j] += v;
            st2[j] += v * ((x - bs[2 * NP + j * 32 + l31]) * bs[3 * NP + j * 32 + l31]);
          } else {
            st1[j] += v;
            st2[j] += v * v;
          }
          P.c[(size_t)row * P.ldc + col] = v;
        }
      }
    }
  }

  if (P.stat_mode != 0) {
    // half-waves, then the NW waves in wave order: one partial row per row group
    __syncthreads();
    float *sred = Cs;  // [NW][NP][2]
    if constexpr (BWD) {
      // the lane's sums for its four columns: over the eight row lanes (lane bits 3-5), then lanes 0-7 own 4 columns each
#pragma unroll
      for (int j = 0; j < TN; j++) {
#pragma unroll
        for (int o = 8; o <= 32; o <<= 1) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            q1[j][e] += __shfl_xor(q1[j][e], o, 64);
            q2[j][e] += __shfl_xor(q2[j][e], o, 64);
          }
        }
        if (lane < 8) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            sred[(wave * NP + j * 32 + c4 + e) * 2 + 0] = q1[j][e];
            sred[(wave * NP + j * 32 + c4 + e) * 2 + 1] = q2[j][e];
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const float a1 = st1[j] + __shfl_xor(st1[j], 32, 64), a2 = st2[j] + __shfl_xor(st2[j], 32, 64);
      if (lhi == 0) {
        // (BWD: st1 / st2 only hold the ragged last tile's share, on top of the row-piece sums written above)
        sred[(wave * NP + j * 32 + l31) * 2 + 0] = (BWD ? sred[(wave * NP + j * 32 + l31) * 2 + 0] : 0.f) + a1;
        sred[(wave * NP + j * 32 + l31) * 2 + 1] = (BWD ? sred[(wave * NP + j * 32 + l31) * 2 + 1] : 0.f) + a2;
      }
    }
    __syncthreads();
    for (int cl = tid; cl < NP; cl += 64 * NW) {
      const int col = n0 + cl;
      if (col < P.N) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; w++) {
          a1 += sred[(w * NP + cl) * 2 + 0];
          a2 += sred[(w * NP + cl) * 2 + 1];
        }
        P.part[((size_t)rg * P.N + col) * 2 + 0] = a1;
        P.part[((size_t)rg * P.N + col) * 2 + 1] = a2;
        for (int r = rg + nrg; r < P.part_rows; r += nrg) {
          P.part[((size_t)r * P.N + col) * 2 + 0] = 0.f;
          P.part[((size_t)r * P.N + col) * 2 + 1] = 0.f;
        }
      }
    }
  }
}

// ---- round 6: the logits layer's backward (deeplabv3p.py:438: Conv2D(classes, (1, 1)) on the 256-wide decoder output) --------
// Both are HBM-bound streams whose narrow side is `classes` = 21 floats per row — 84-byte rows that no 16-byte access lines up
// with, which is why the tiled kernels ran them at 0.35 / 0.21 of the HBM peak (scalar loads of the narrow operand, 16-row
// stages with eight MFMAs per barrier).  The narrow operand is handled as what it is in memory: one contiguous run.
//
// bwd-data: dX[M, 32 TN] = dY[M, K] . W^T[K, 32 TN] with K = classes <= 32 and dY rows back to back (lda == K): a wave takes the
// 32 K floats of its row tile as 8 K 16-byte pieces of one contiguous, 16-byte-aligned run (three loads per lane at K = 21,
// requested one tile ahead), parks them in a wave-private LDS strip and reads its MFMA A-fragments from there (row l31, k =
// lhi ceil(K/2) + s: stride K, conflict-free for odd K); W^T sits in LDS for the workgroup's lifetime, zero rows up to 2 ceil(K/2).
// No transform, mask, addend or BatchNorm sums: the layer's input is the Dropout output (a materialised buffer).
template <int TN, int NW>
__global__ __launch_bounds__(64 * NW) void pw_narrowk_kernel(GemmArgs P) {
  constexpr int NP = 32 * TN;
  __shared__ __attribute__((aligned(16))) float Bs[32 * NP];     // W^T[k][n], zero for k >= K
  __shared__ __attribute__((aligned(16))) float As[NW * 1024];   // per wave: its tile of dY, 32 rows of K floats, packed
  __shared__ __attribute__((aligned(16))) float Cs[NW * 1024];   // per wave: one 32x32 block on its way out
  static_assert(sizeof(float) * (32 * NP + 2 * NW * 1024) <= 160 * 1024, "gfx950: 160 KB of LDS per CU");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int n0 = blockIdx.y * NP;
  for (int i = tid; i < 32 * NP; i += 64 * NW) {
    const int k = i / NP, n = n0 + i % NP;
    Bs[i] = (k < P.K && n < P.N) ? P.b[(size_t)k * P.ldb + n] : 0.f;
  }
  __syncthreads();
  const int KS = (P.K + 1) >> 1;                 // k-steps: lane half lhi owns k = lhi KS .. lhi KS + KS - 1
  const int npc = 8 * P.K;                       // 16-byte pieces per row tile (<= 256)
  const int nfull = P.M >> 5;
  const int gw = blockIdx.x * NW + wave, GW = gridDim.x * NW;
  float *const as = As + wave * 1024, *const cw = Cs + wave * 1024;
  const int c4 = (lane & 7) * 4, r0 = lane >> 3;
  f32x4 f[4];
  auto req = [&](int t) __attribute__((always_inline)) {
    const float *p = P.a + (size_t)t * 32 * P.K;
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (lane + 64 * q < npc) f[q] = ld4(p + 4 * (lane + 64 * q));
  };
  auto products = [&](f32x16 (&acc)[TN]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    const float *ap = as + l31 * P.K + lhi * KS;
    const float *bp = Bs + lhi * KS * NP + l31;
    for (int s = 0; s < KS; s++) {
      const float a = (lhi * KS + s < P.K) ? ap[s] : 0.f;
#pragma unroll
      for (int j = 0; j < TN; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[s * NP + j * 32], acc[j], 0, 0, 0);
    }
  };
  if (gw < nfull) req(gw);
  for (int t = gw; t < nfull; t += GW) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (lane + 64 * q < npc) st4(as + 4 * (lane + 64 * q), f[q]);
    __builtin_amdgcn_wave_barrier();
    req(t + GW < nfull ? t + GW : t);
    f32x16 acc[TN];
    products(acc);
    float *const cp = P.c + (size_t)(t * 32 + r0) * P.ldc + n0 + c4;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      if (n0 + j * 32 < P.N) {      // (the output width is a multiple of 32: whole blocks)
#pragma unroll
        for (int r = 0; r < 16; r++) cw[((r & 3) + 8 * (r >> 2) + 4 * lhi) * 32 + l31] = acc[j][r];
        __builtin_amdgcn_wave_barrier();
        f32x4 o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) o[p] = ld4(cw + (r0 + 8 * p) * 32 + c4);
#pragma unroll
        for (int p = 0; p < 4; p++) st4_nt(cp + (size_t)(8 * p) * P.ldc + j * 32, o[p]);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if ((P.M & 31) != 0 && gw == nfull % GW) {   // the ragged last tile: element by element
    const int m0 = nfull * 32;
    const size_t total = (size_t)P.M * P.K;
    for (int i = lane; i < 32 * P.K; i += 64) {
      const size_t e = (size_t)m0 * P.K + i;
      as[i] = e < total ? P.a[e] : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    f32x16 acc[TN];
    products(acc);
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col = n0 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (row < P.M && col < P.N) P.c[(size_t)row * P.ldc + col] = acc[j][r];
      }
    }
  }
}
}  // namespace

// (tests/test_pwconv_cases_host.py::test_universe_restates_the_launchers reads this switch as text and tests/pwconv_cases.py universe()
// lists its instantiations: an instantiation added, dropped or renamed here is added there, with a case that reaches it)
void pw::launch_ws(const GemmArgs &A, const GemmPlan &P, void *stream) {
  constexpr int NW = DL3_WS2_NW;
  const dim3 grid(P.grid[0], P.grid[1], P.grid[2]), blk(256), blkw(64 * NW);
#define DL3_GO(KERNEL_, BLK_) hipLaunchKernelGGL((KERNEL_), grid, BLK_, P.lds, (hipStream_t)stream, A)
  switch (P.kernel) {
    case PW_NARROW_FLAT: DL3_GO((pw_ws2_kernel<32, 1, NW, false, false, false, true>), blkw); break;
    case PW_NARROWK: DL3_GO((pw_narrowk_kernel<8, NW>), blkw); break;
    case PW_WS2:
      if (P.two) {
        if (P.add) DL3_GO((pw_ws2_kernel<48, 2, NW, true, true, true>), blkw);
        else DL3_GO((pw_ws2_kernel<48, 2, NW, true, true, false>), blkw);
      } else if (!P.fwd) {
        switch (P.tn) {
          case 5: DL3_GO((pw_ws2_kernel<20, 5, NW, true>), blkw); break;
          case 3: DL3_GO((pw_ws2_kernel<12, 3, NW, true>), blkw); break;
          default: DL3_GO((pw_ws2_kernel<8, 4, NW, true>), blkw); break;
        }
      } else {
        switch (P.tn) {
          case 5: DL3_GO((pw_ws2_kernel<20, 5, NW>), blkw); break;
          case 3: DL3_GO((pw_ws2_kernel<12, 3, NW>), blkw); break;
          default: DL3_GO((pw_ws2_kernel<8, 4, NW>), blkw); break;
        }
      }
      break;
    default:   // PW_WS: (KQ, TN, workgroups per CU: the most the registers allow without spilling)
      switch (P.kq * 10 + P.tn) {
        case 23: DL3_GO((pw_fwd_ws_kernel<2, 3, 4>), blk); break;
        case 35: DL3_GO((pw_fwd_ws_kernel<3, 5, 3>), blk); break;
        case 41: DL3_GO((pw_fwd_ws_kernel<4, 1, 4>), blk); break;
        case 46: DL3_GO((pw_fwd_ws_kernel<4, 6, 3>), blk); break;
        case 121: DL3_GO((pw_fwd_ws_kernel<12, 1, 4>), blk); break;
        case 181: DL3_GO((pw_fwd_ws_kernel<18, 1, 3>), blk); break;
        default: DL3_GO((pw_fwd_ws_kernel<24, 1, 3>), blk); break;
      }
  }
#undef DL3_GO
}
