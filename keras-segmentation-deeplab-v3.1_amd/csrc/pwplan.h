// pwplan.h — the 1x1-convolution launch planner: which kernel a launch of csrc/pwgemm.hip takes, on which grid, and how many
// statistic partial rows / weight-gradient slabs it writes.  Host-only C++17: no HIP type, no device call, no allocation
// (g++ -fsyntax-only pwplan.h).  The decision exists ONCE, here: pwgemm.hip's launch_gemm and the family launchers of the
// kernel files (csrc/pwargs.h) switch over the template instantiations a plan names and test nothing themselves, and every
// sizing and route query of the C ABI (dl3_pwconv_partials, _route, _fwd_impl, _bwd_weight_workspace, _bwd_weight_splits)
// is the planner's answer for the operand forms listed at the end of this file.  A route that is added or retuned in
// plan_gemm_one / plan_wgrad moves the queries with it; the launches refuse a plan that writes more partial rows than the
// caller's buffer holds.
// EXACTLY ONE translation unit includes this header (pwgemm.hip; tests/test_host.py::test_pwplan_is_included_once): a second
// inclusion would duplicate its per-process state, g_gemm_math and the `static` knob caches.  The kernel files take csrc/pwargs.h.
//
// Knobs: DL3_WS2, DL3_NARROW, DL3_COLSPLIT and DL3_WGRAD_ROW are read once per process, DL3_GEMM_CFG, DL3_GEMM_PRE,
// DL3_GEMM_PY, DL3_WGRAD_CFG and DL3_GEMM_MATH / dl3_set_gemm_math at every call (tests set them in-process).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/dl3.h"
#include "pwargs.h"  // GemmArgs, WgradArgs, GemmKernel, GemmPlan, WgradPlan; DL3_STREAM_KMAX, DL3_WGRAD_MS, DL3_WS2_NW

#ifndef DL3_WGRAD_WGS_DEFAULT
#define DL3_WGRAD_WGS_DEFAULT 1024
#endif
#ifndef DL3_GEMM_PY_DEFAULT
#define DL3_GEMM_PY_DEFAULT 2048
#endif

namespace {  // (the planner and its state: this unit's own)
using namespace pw;

inline int pw_cdiv(int a, int b) { return (a + b - 1) / b; }
inline bool al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
inline int env_int(const char *name) {
  const char *e = getenv(name);
  return e ? atoi(e) : -1;
}

int g_gemm_math = -1;  // DL3_MATH_ENV
inline bool split_math() {
  if (g_gemm_math >= 0) return g_gemm_math == 1;
  const char *e = getenv("DL3_GEMM_MATH");  // "split": fp32 as 3 x bf16 on the bf16 matrix pipe; default: f32 MFMA
  return e && e[0] == 's';
}

// a dl3_pwconv_fwd* / _bwd_data call: one launch, or two over disjoint column ranges of the same output (the column split)
struct GemmLaunch {
  int n;
  GemmArgs args[2];
  GemmPlan plan[2];
  int rows() const { return n == 2 && plan[1].rows > plan[0].rows ? plan[1].rows : plan[0].rows; }
};

// ---- route predicates and grids ----------------------------------------------------------
// shapes and row counts the K-split kernel takes: 1 024 - 16 384 rows
inline int ksplit_tn(int M, int K, int N) {
  // (a pure function of the shape; the DL3_KSPLIT / DL3_KSPLIT_ROWS knobs of round 5's A/B are gone)
  if (M > 16384 || M < 1024 || K < 192 || K > DL3_STREAM_KMAX || K % 4 != 0 || N % 4 != 0) return 0;
  const int tn = pw_cdiv(N, 32);
  // 64-, 96- and 160-wide outputs: the ones the 64-column-per-wave kernels pad (to 128, 128 and 256 columns)
  return (tn == 2 || tn == 3 || tn == 5) ? tn : 0;
}

// the layer shapes the weight-stationary HBM kernel is instantiated for: (K, N) -> TN (KQ = K / 8); 0: not served
inline int ws_tn(int K, int N) {
  if (K % 8 != 0 || N % 4 != 0) return 0;
  const int tn = pw_cdiv(N, 32);
  // MobileNetV2's HBM-bound 1x1 convolutions (alpha = 1): 32->16, 16->96, 96->24, 24->144, 144->24, 144->32, 32->192, 192->32
  switch (K) {
    case 16: return tn == 3 ? tn : 0;
    case 24: return tn == 5 ? tn : 0;
    case 32: return (tn == 1 || tn == 6) ? tn : 0;
    case 96: return tn == 1 ? tn : 0;
    case 144: return tn == 1 ? tn : 0;
    case 192: return tn == 1 ? tn : 0;
    default: return 0;
  }
}
inline int ws_grid(int M) {
  // persistent: three workgroups per CU, never more waves than 32-row tiles
  const int tiles = pw_cdiv(M, 32);
  const int g = pw_cdiv(tiles, 4);
  return g < 768 ? g : 768;
}
// forward launch served by the weight-stationary kernel of the HBM-bound layers?
inline bool ws_wanted(const GemmArgs &A, bool fwd, bool vec) {
  if (!fwd || !vec || A.ep_add || A.a2) return false;
  if (A.ldc % 4 != 0 || !al16(A.c)) return false;  // 16-byte stores
  if (A.M < 32768) return false;
  return ws_tn(A.K, A.N) != 0;
}

// round 6: the weight-stationary kernel for MFMA-bound short reductions (pw_ws2_kernel): row groups per column tile — one
// workgroup per CU over all column tiles
inline int ws2_groups(int M, int ntn) {
  const int tiles = pw_cdiv(M, 32);
  int g = 256 / ntn;
  if (g < 1) g = 1;
  const int cap = pw_cdiv(tiles, DL3_WS2_NW);
  return g < cap ? g : cap;
}
// DL3_WS2=0: the tiled stream kernel serves everything
inline bool ws2_on() {
  static const int env = env_int("DL3_WS2");
  return env != 0;
}
// shapes it takes: a reduction of 160, 96 or 64 (MobileNetV2's 64 x 64 blocks, deeplabv3p.py:175-198) into an output at least twice
// as wide, from a row count below which a wave walks too few tiles to pay for loading its 60-100 KB weight slice — measured per
// direction (profiles/r06_ab_calls.txt calls 34 / 35, tiled -> weight-stationary): forward 160 -> 960 at 65 536 rows 0.218 -> 0.228 ms,
// at 98 304 0.339 -> 0.312; bwd-data 960 <- 160 at 32 768 rows 0.151 -> 0.158, at 65 536 0.295 -> 0.261 (the tiled kernel's masked
// epilogue is the longer one); reduction 64: 131 072 rows either way.
inline bool ws2_shape(int M, int K, int N, bool bwd) {
  if (!ws2_on()) return false;
  const int minrows = K == 64 ? 131072 : (bwd ? 65536 : 98304);
  return M >= minrows && N % 4 == 0 && ((K == 160 && N >= 320) || (K == 96 && N >= 192) || (K == 64 && N >= 128));
}
inline int ws2_tn(int K) { return K == 160 ? 5 : (K == 96 ? 3 : 4); }
// 1: forward, 2: bwd-data (single-tensor dY, mask and BatchNorm-backward sums from the forward input, no addend), 3: bwd-data
// of the expand convolutions 64 -> 384 (two-tensor operand over a reduction of 384, 64-wide gradient, optional residual), 0: no
inline int ws2_wanted(const GemmArgs &A, bool fwd, bool vec) {
  if (!ws2_on() || !vec || (A.bias && !fwd) || A.ldc % 4 != 0 || !al16(A.c)) return 0;
  if (!fwd && A.a2) {
    if (A.M < 131072 || A.K != 384 || A.N != 64 || !A.ka || A.bias || A.stat_mode == 1 || !A.ep_x) return 0;
    if (A.ld_epx % 4 != 0 || !al16(A.ep_x)) return 0;
    if (A.ep_add && (A.add_div != 1 || A.ld_add % 4 != 0 || !al16(A.ep_add))) return 0;
    return 3;
  }
  if (A.ep_add || A.a2 || !ws2_shape(A.M, A.K, A.N, !fwd)) return 0;
  if (fwd) return 1;
  if (A.ka || !A.ep_x || A.ld_epx % 4 != 0 || !al16(A.ep_x) || A.stat_mode == 1) return 0;
  return 2;
}

// round 6: the logits layer (N = classes <= 32 off a 256-wide input): 1 = forward with the packed narrow output (pw_ws2_kernel
// FLAT), 2 = bwd-data over the narrow reduction (pw_narrowk_kernel), 0 = no.  DL3_NARROW=0: the tiled kernels (A/B aid).
inline bool narrow_on() {
  static const int env = env_int("DL3_NARROW");
  return env != 0;
}
inline bool narrow_shape(int M, int K, int N) { return narrow_on() && M >= 8192 && K == 256 && N <= 32; }
inline int narrow_wanted(const GemmArgs &A, bool fwd, bool avec) {
  if (A.a2 || A.ep_add || A.M < 8192 || !narrow_on()) return 0;
  if (fwd && avec && narrow_shape(A.M, A.K, A.N) && A.ldc == A.N && al16(A.c)) return 1;
  // (16 384 rows: measured 8 192 rows 0.011 -> 0.013 ms, 65 536 rows 0.039 -> 0.023)
  if (A.M >= 16384 && A.K <= 32 && A.N == 256 && !A.ka && A.a_act == DL3_ACT_NONE && !A.ep_x && !A.bias && A.stat_mode == 0 && A.lda == A.K &&
      A.ldc % 4 == 0 && al16(A.a) && al16(A.c))
    return 2;
  return 0;
}
inline int narrow_groups(int M) {
  const int cap = pw_cdiv(pw_cdiv(M, 32), DL3_WS2_NW);
  return cap < 256 ? cap : 256;
}
// ... and its weight gradient (pw_wgrad_narrow_kernel): slabs = workgroups, one per CU, never more waves than 16-row spans
// (from 131 072 rows: at 65 536 the eight-wave meeting and the 256-slab fold cost what the loop saves, 0.053 -> 0.056 ms)
inline bool wgrad_narrow_shape(int M, int K, int N) { return narrow_on() && M >= 131072 && K == 256 && N <= 32; }
inline int wgrad_narrow_slabs(int M) {
  const int cap = pw_cdiv(pw_cdiv(M, 16), DL3_WS2_NW);
  return cap < 256 ? cap : 256;
}

// ---- tile configuration of the tiled kernels ------------------------------------------------
struct GemmCfg { int id, BM, BN; };
const GemmCfg kGemmCfgs[] = {{0, 128, 128}, {1, 256, 64}, {2, 256, 32}, {3, 128, 160}, {4, 128, 96},
                             {5, 32, 256},  {6, 32, 128}};  // 5, 6: four waves side by side, for small M
constexpr int kNumGemmCfgs = 7;

// small: the 32-row configurations may be chosen (they exist for the stream kernel only)
inline GemmCfg pick_gemm(int M, int K, int N, bool two, bool small, bool fwd) {
  const int forced = env_int("DL3_GEMM_CFG");  // tuning aid (tools/gemm_tune.py)
  if (forced >= 0 && forced < kNumGemmCfgs && (small || kGemmCfgs[forced].BM != 32)) return kGemmCfgs[forced];
  // measured exception (tools/gemm_tune.py): a forward GEMM with a very short reduction and a wide output
  // (24 -> 144 at 128x128) is a pure streaming kernel and wants the tall 256x64 tile
  // (forward launches only: the single-tensor bwd-data launches of round 4 are `!two` as well — 144 <- 24 at 128x128 ran
  // 0.71 -> 0.83 ms through this exception)
  if (fwd && !two && K < 32 && N > 128 && M >= 65536) return kGemmCfgs[1];
  double best = 1e30;
  GemmCfg bc = kGemmCfgs[0];
  for (const GemmCfg &c : kGemmCfgs) {
    if (c.BM == 32 && !small) continue;
    // measured on MI355X (tools/gemm_tune.py): ~80 TFLOP/s sustained fp32 MFMA, ~3 TB/s streaming; re-reads of A by
    // the other column tiles of a row tile are L2 hits thanks to the XCD remap (charged at 1/4)
    const double ntn = pw_cdiv(N, c.BN), mp = (double)pw_cdiv(M, c.BM) * c.BM;
    // fewer workgroups than the chip holds (2 per CU) leave matrix pipes idle; the 32-row configs pay ~15 % more
    // per MFMA (every wave re-reads the shared A rows through L1) and are for exactly that case
    const double blocks = (double)pw_cdiv(M, c.BM) * ntn;
    const double util = blocks < 512.0 ? blocks / 512.0 : 1.0;
    const double t_mfma = 2.0 * mp * K * ntn * c.BN / 80e12 / util * (c.BM == 32 ? 1.15 : 1.0);
    const double t_mem = 4.0 * ((double)M * K * (1.0 + 0.25 * (ntn - 1)) * (two ? 2 : 1) + (double)M * N) / 3e12;
    const double cost = (t_mfma > t_mem ? t_mfma : t_mem) + 0.25 * (t_mfma + t_mem);
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// masked bwd-data launch whose epilogue operand can be prefetched (pw_gemm_stream_kernel EPI 2)
inline bool pre_ok(const GemmArgs &A) {
  return A.ep_x && !A.bias && !A.ep_add && env_int("DL3_GEMM_PRE") != 0;
}
// ... and for which the 128x96 prefetching tile beats the cost model's choice: short reductions (the epilogue is as
// long as the main loop) into a wide output made of whole 96-column tiles, with enough row tiles to fill the chip
inline bool pre_wanted(const GemmArgs &A) {
  return A.K <= 320 && A.N % 96 == 0 && A.N >= 2 * A.K && A.M >= 65536;
}

inline int gemm_grid_y(int M, int N, const GemmCfg &c, int K) {
  const int mtiles = pw_cdiv(M, c.BM), ntn = pw_cdiv(N, c.BN);
  // target number of workgroups per launch (DL3_GEMM_PY overrides: tuning aid).  Measured on MI355X, whole step:
  const int pytot = env_int("DL3_GEMM_PY");
  // plenty of row tiles (>= 4 per resident workgroup): 512 workgroups = exactly two per CU, each a persistent loop over
  // its row tiles (sweep at B=64: 256 -> 64.3 ms, 384 -> 66.4, 512 -> 57.7, 640 -> 63.0, 768 -> 60.3, 2048 -> 58.4: any
  // count that is not a whole number of waves of the chip leaves a ragged last wave); fewer tiles: several waves of
  // short workgroups balance better (B=2: 2048 -> 4.97 ms, 512 -> 5.08)
  // round 6: ... and 5-16 LONG tiles per resident workgroup (reduction >= 512, at most 1 024 row tiles: Xception at B = 16 / 32)
  // do not want the persistent loop either: a workgroup that walks 5 or 6 such tiles wastes up to a fifth of the launch on
  // the quantisation, which the dispatcher's own balancing of one- or two-tile workgroups does not (same-call A/B, cfg4 B=16:
  // 736 -> 736 forward 0.680 -> 0.630 ms, 1536 -> 1536 2.65 -> 2.46; 85.2 -> 87.4 img/s; MobileNetV2 B=16 / 128 unchanged / -0.5 %)
  const long tiles = (long)mtiles * ntn;
  const bool long_few = K >= 512 && mtiles <= 1024 && tiles < 8192;
  const int dflt = long_few ? 4096 : (tiles >= 2048 ? 512 : DL3_GEMM_PY_DEFAULT);
  int py = (pytot > 0 ? pytot : dflt) / ntn;
  if (py < 32) py = 32;
  if (mtiles <= py) return mtiles;
  const int iters = pw_cdiv(mtiles, py);  // every workgroup loops over the same number of row tiles ...
  const int even = pw_cdiv(mtiles, iters);
  // ... unless that leaves more than a tenth of the chip's 512 slots empty (512 row tiles x 5 column tiles: 86 x 5 = 430
  // workgroups of 6 tiles, most CUs carry 12 tile-times; 102 x 5 = 510 workgroups of 5 or 6 carry 10-11: the Xception
  // 736 -> 736 GEMM at 65536 rows 0.810 -> 0.733 ms forward, 0.924 -> 0.869 bwd-data).
  if ((long)even * ntn * 10 < 512L * 9) return py;
  return even;
}

// ---- one launch ---------------------------------------------------------------------------
struct OperandVec { bool a, b; };  // 16-byte loads possible on the activation operand(s) / on the weights
inline OperandVec operand_vec(const GemmArgs &A) {
  const bool avec = (A.K % 4 == 0) && (A.lda % 4 == 0) && al16(A.a) && (!A.a2 || ((A.lda2 % 4 == 0) && al16(A.a2)));
  const bool bvec = (A.N % 4 == 0) && (A.ldb % 4 == 0) && al16(A.b);
  return {avec, bvec};
}

// the cascade: narrow -> weight-stationary MFMA -> weight-stationary HBM -> K-split -> stream tile (prefetching or split-math
// variants) -> LDS-staged tile.  split: the matrix math of the launch (the weight-stationary and K-split kernels are f32 only)
inline GemmPlan plan_gemm_one(const GemmArgs &A, bool split) {
  GemmPlan P{};
  P.route = DL3_ROUTE_TILED;
  P.two = A.a2 != nullptr;
  P.add = A.ep_add != nullptr;
  const OperandVec v = operand_vec(A);
  const bool vec = v.a && v.b;
  P.vmode = vec ? 1 : (v.a ? 2 : 0);
  const bool stream = vec && A.K <= DL3_STREAM_KMAX;
  // (a per-image addend stays on the forward instantiation when its straight-line epilogue can take it: 32-row blocks
  // inside one image)
  P.fwd = !P.two && !A.ep_x && A.stat_mode != 2 && !(A.ep_add && A.add_div > 1 && A.add_div % 32 != 0);
  P.grid[0] = P.grid[1] = P.grid[2] = 1;
  if (const int nr = split ? 0 : narrow_wanted(A, P.fwd, v.a)) {
    P.route = DL3_ROUTE_NARROW;
    if (nr == 1) {
      P.kernel = PW_NARROW_FLAT;
      P.grid[1] = P.rows = ws2_groups(A.M, 1);
    } else {   // (no statistic sums on this route: narrow_wanted)
      P.kernel = PW_NARROWK;
      P.grid[0] = narrow_groups(A.M);
      P.grid[1] = A.N / 256;
    }
    return P;
  }
  if (const int w2 = split ? 0 : ws2_wanted(A, P.fwd, vec)) {
    P.route = DL3_ROUTE_WS_MFMA;
    P.kernel = PW_WS2;
    P.tn = w2 == 3 ? 2 : ws2_tn(A.K);
    P.kq = A.K / 8;
    P.grid[0] = w2 == 3 ? 1 : pw_cdiv(A.N, 32 * P.tn);
    P.grid[1] = P.rows = ws2_groups(A.M, P.grid[0]);
    return P;
  }
  if (!split && ws_wanted(A, P.fwd, vec)) {
    P.route = DL3_ROUTE_WS_HBM;
    P.kernel = PW_WS;
    P.kq = A.K / 8;
    P.tn = ws_tn(A.K, A.N);
    P.grid[0] = P.rows = ws_grid(A.M);
    return P;
  }
  if (vec && !split) {
    if (const int ktn = ksplit_tn(A.M, A.K, A.N)) {
      P.route = DL3_ROUTE_KSPLIT;
      P.kernel = PW_KSPLIT;
      P.tn = ktn;
      P.grid[0] = P.rows = pw_cdiv(A.M, 32);
      return P;
    }
  }
  GemmCfg c = pick_gemm(A.M, A.K, A.N, P.two, stream, P.fwd);
  if (stream && pre_ok(A) && pre_wanted(A)) c = kGemmCfgs[4];
  P.cfg = c.id;
  P.mtiles = pw_cdiv(A.M, c.BM);
  P.grid[0] = pw_cdiv(A.N, c.BN);
  P.grid[1] = P.rows = gemm_grid_y(A.M, A.N, c, A.K);
  // stream-A kernel: 10-25 % faster than the LDS-staged kernel on every layer shape, forward and bwd-data
  // (tools/gemm_tune.py).  The two-tensor bwd-data operand uses 16-deep K-tiles so that its register budget does not
  // spill.  (Unaligned operands take the LDS-staged kernel.)
  P.kernel = stream ? PW_STREAM : PW_LDS;
  if (stream) {
    P.pre = c.id == 4 && pre_ok(A);
    // (the 32-row small-M tiles keep the f32 MFMA: their split weight tiles exceed the LDS)
    P.split = split && c.id != 5 && c.id != 6;
    if (P.split) P.lds = 4u * (P.two ? 3 : 2) * (unsigned)pw_cdiv(A.K, 32) * 32;
  }
  return P;
}

// round 6: Xception's 728-channel layers (deeplabv3p.py:300-306) are stored 736 wide — 23 column blocks of 32,
// which no tile width divides: six 128-wide tiles compute 24 (the stream kernel multiplies zero weight columns like any other).
// 23 = 2 x 4 + 3 x 5: such a launch is issued as TWO over disjoint column ranges of the same output, [0, N - 480) on the
// 128-wide tiles and the last 480 columns on the 160-wide ones — 23 blocks exactly, both launches several full rounds of the
// chip.  The operand rows are read by both (the second pass over a 65 536 x 736 operand is 0.19 GB against 0.65 ms of MFMA
// time); partial sums land in disjoint columns of the same rows.  (First cut, 640 + 96 columns: the 128 x 96 tile of the
// narrow launch costs 0.78 of a 128-wide one — forward 0.749 -> 0.712 ms, bwd-data 0.798 -> 0.796.)  DL3_COLSPLIT=0: one launch.
constexpr int kColsplitTail = 480;
inline bool colsplit_shape(int M, int K, int N) {
  static const int env = env_int("DL3_COLSPLIT");
  return env != 0 && M >= 32768 && K >= 256 && K <= DL3_STREAM_KMAX && N >= kColsplitTail + 128 && N % 128 == 96 && N % 160 != 0;
}

inline GemmLaunch plan_gemm(const GemmArgs &A, bool split = split_math()) {
  GemmLaunch L{};
  L.n = 1;
  L.args[0] = A;
  const OperandVec v = operand_vec(A);
  // (single-tensor operand only: the two-tensor bwd-data form, which the engine does not use once the weight-gradient launch
  // has written dY, came out 2 % slower in two launches — 0.834 -> 0.851 ms)
  if (v.a && v.b && !A.a2 && !split && colsplit_shape(A.M, A.K, A.N)) {
    const int n1 = A.N - kColsplitTail;
    GemmArgs &T = L.args[1] = A;
    L.n = 2;
    L.args[0].N = n1;
    T.N = kColsplitTail;
    T.b += n1; T.c += n1;
    if (A.bias) T.bias += n1;
    if (A.ep_x) T.ep_x += n1;
    if (A.ep_scale) { T.ep_scale += n1; T.ep_shift += n1; }
    if (A.ep_mean) { T.ep_mean += n1; T.ep_invstd += n1; }
    if (A.ep_add) T.ep_add += n1;
    if (A.part) T.part += 2 * (size_t)n1;
    L.args[0].part_ld = T.part_ld = A.N;
  }
  for (int i = 0; i < L.n; i++) L.plan[i] = plan_gemm_one(L.args[i], split);
  return L;
}

// ---- the weight gradient -----------------------------------------------------------------
struct WgCfg { int id, BKT, BNT; };
const WgCfg kWgCfgs[] = {{0, 64, 64},  {1, 128, 128}, {2, 160, 128}, {3, 128, 160}, {4, 64, 128},
                         {5, 128, 64}, {6, 32, 128},  {7, 128, 32},  {8, 96, 128},  {9, 128, 96}};

// M splits the tile cost model reasons with: ~1024 workgroups, capped by slab traffic and by rows per split
inline int wgrad_splits_model(int M, int K, int N, const WgCfg &c, int target = DL3_WGRAD_WGS_DEFAULT) {
  const long tiles = (long)pw_cdiv(K, c.BKT) * pw_cdiv(N, c.BNT);
  long S = target / tiles;
  const long cap_traffic = (long)((double)M * (K + N) / (4.0 * K * N));
  const long cap_rows = M / 64;
  if (S > cap_traffic) S = cap_traffic;
  if (S > cap_rows) S = cap_rows;
  if (S < 1) S = 1;
  return (int)S;
}

// ... and the M splits a launch gets.  Every split writes a K x N slab that the fold reads back; for the 160-wide tiles
// on a small weight matrix (<= 160 x 960) at 32k-128k rows that is a fifth of the launch's bytes, and two workgroups per CU
// (half the slabs) are faster.  Measured in situ (round 4, calls 16 / 17, B=16: M = 65536): 160 x 960 291 -> 258 us,
// 960 x 160 253 -> 230, 576 x 160 180 -> 156; whole step 1 055 / 1 068 / 1 071 -> 1 068 / 1 082 / 1 086 img/s.  NOT a general
// rule: the same halving on Xception's 736 x 736 at the same M costs 24 % of the launch, on 64 x 384 5 %, and at
// M = 16384 (B=4) the 160-wide shapes lose 12 % (profiles/r04_ab_calls.txt, call 17).
inline int wgrad_splits(int M, int K, int N, const WgCfg &c) {
  const int S = wgrad_splits_model(M, K, N, c);
  const bool wide = (c.id == 2 || c.id == 3) && (long)K * N <= 160L * 960 && M >= 32768;
  if (wide && 2.0 * (double)S * K * N > 0.1 * (double)M * (K + N)) return wgrad_splits_model(M, K, N, c, DL3_WGRAD_WGS_DEFAULT / 2);
  return S;
}

inline WgCfg pick_wgrad(int M, int K, int N, bool two) {
  const int forced = env_int("DL3_WGRAD_CFG");
  if (forced >= 0 && forced < 10) return kWgCfgs[forced];
  // measured shortcuts (tools/gemm_tune.py, MI355X, M >= 32k rows): small weight matrices want the 64x64 tile (more
  // workgroups per M split), 160-multiples want the 160-wide tiles so the big operand is read once
  if (M >= 32768) {
    if (K >= 32 && N >= 32 && (long)K * N <= 32768) return kWgCfgs[0];
    if (N % 160 == 0 && K >= 128 && K % 160 != 0) return kWgCfgs[3];
    if (K % 160 == 0 && K % 128 != 0 && N >= 128 && N % 160 != 0) return kWgCfgs[2];
    if (K % 160 == 0 && N % 160 == 0 && K >= 320 && N >= 320) return kWgCfgs[3];
  }
  double best = 1e30;
  WgCfg bc = kWgCfgs[0];
  for (const WgCfg &c : kWgCfgs) {
    const double ntk = pw_cdiv(K, c.BKT), ntn = pw_cdiv(N, c.BNT);
    // few rows: the M split is capped (partial-slab traffic), so small tiles are what fills the chip
    const double blocks = ntk * ntn * wgrad_splits_model(M, K, N, c);
    const double util = blocks < 512.0 ? blocks / 512.0 : 1.0;
    const double t_mfma = 2.0 * M * ntk * c.BKT * ntn * c.BNT / 80e12 / util;
    const double t_mem = 4.0 * ((double)M * K * (1.0 + 0.25 * (ntn - 1)) +
                                (double)M * N * (1.0 + 0.25 * (ntk - 1)) * (two ? 2 : 1)) / 3e12;
    const double cost = (t_mfma > t_mem ? t_mfma : t_mem) + 0.25 * (t_mfma + t_mem);
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// the weight gradient of a launch with tile configuration c takes the one-tile-row kernel: K fits one tile row of it — the
// straight-line kernel of the expand convolutions (DL3_WGRAD_ROW=0: off — A/B aid)
inline bool wgrad_row_ok(const WgCfg &c, int M, int K, int N, bool split) {
  static const int row_env = env_int("DL3_WGRAD_ROW");
  return row_env != 0 && !split && pw_cdiv(K, c.BKT) == 1 && K % 4 == 0 && N % 4 == 0 && (c.id == 2 || c.id == 8) && M >= 32768;
}

inline int colsum_rows(int M) {
  int pr = M / 256;
  if (pr < 1) pr = 1;
  if (pr > 256) pr = 256;
  return pr;
}

// two: two-tensor dY (cA given); xvec / dvec: 16-byte loads possible on x / on g and yraw; dy_out: the launch writes dY;
// dw: the launch folds its slabs itself
inline WgradPlan plan_wgrad(int M, int K, int N, bool two, bool xvec, bool dvec, bool dy_out, bool dw, bool split = split_math()) {
  WgradPlan P{};
  const WgCfg c = pick_wgrad(M, K, N, two);
  P.cfg = c.id;
  P.split = split;
  P.S = wgrad_splits(M, K, N, c);
  P.Mper = pw_cdiv(pw_cdiv(M, P.S), DL3_WGRAD_MS) * DL3_WGRAD_MS;
  P.vec = (xvec && dvec) ? 1 : (xvec ? 2 : 0);
  // the logits layer: N = classes, the whole K x N gradient in every wave's accumulators
  P.narrow = xvec && !two && !dy_out && dw && !split && wgrad_narrow_shape(M, K, N);
  P.row = !P.narrow && xvec && dvec && wgrad_row_ok(c, M, K, N, split);
  P.route = P.narrow ? DL3_ROUTE_NARROW : (P.row ? DL3_ROUTE_WGRAD_ROW : DL3_ROUTE_TILED);
  if (P.narrow) {   // (one slab and one row of column sums per workgroup)
    P.grid[0] = P.slabs = P.colsum_rows = wgrad_narrow_slabs(M);
    P.grid[1] = P.grid[2] = 1;
  } else {
    P.grid[0] = pw_cdiv(N, c.BNT);
    P.grid[1] = pw_cdiv(K, c.BKT);
    P.grid[2] = P.slabs = P.S;
    P.colsum_rows = colsum_rows(M);
  }
  return P;
}

// ---- the queries: the planner's answers for the operand forms the header documents ------------------
// operand pointers of a canonical form: only their presence and their alignment are looked at
float *const kPlanOperand = reinterpret_cast<float *>(uintptr_t(1) << 20);

enum {
  PF_TWO = 1,        // bwd-data with the two-tensor dY (cA * g + cB * yraw + cC)
  PF_MASK = 2,       // bwd-data with the forward input as epilogue operand (activation mask, BatchNorm-backward sums)
  PF_ADD = 4,        // an addend of the output's shape (residual)
  PF_UNALIGNED = 8,  // every operand 4 bytes off a 16-byte boundary
};
// the GEMM [M, K] x [K, N] with rows back to back, statistic sums asked for (BatchNorm sums forward, BatchNorm-backward sums
// with PF_MASK)
inline GemmArgs gemm_form(int M, int K, int N, unsigned flags) {
  GemmArgs A{};
  float *const p = kPlanOperand + ((flags & PF_UNALIGNED) ? 1 : 0);
  A.a = p; A.lda = K;
  if (flags & PF_TWO) { A.a2 = p; A.lda2 = K; A.ka = A.kb = A.kc = p; }
  A.b = p; A.ldb = N;
  A.c = p; A.ldc = N;
  A.M = M; A.K = K; A.N = N;
  A.add_div = 1; A.add_scale = 1.f;
  A.stat_mode = 1;
  if (flags & PF_MASK) { A.ep_x = p; A.ld_epx = N; A.ep_mean = A.ep_invstd = p; A.stat_mode = 2; }
  if (flags & PF_ADD) { A.ep_add = p; A.ld_add = N; }
  A.part = p;
  return A;
}

// the launch dl3_pwconv_route's dir names (include/dl3.h), for a layer K -> N over M rows: 16-byte aligned operands, rows back
// to back.  dir 0: forward, no addend; 1: bwd-data with the single-tensor dY, a mask operand and no addend; 3: bwd-data with
// the single-tensor dY and neither mask, addend nor sums.  (bwd-data reduces over N and is K wide.)
inline GemmArgs canonical_args(int dir, int M, int K, int N) {
  if (dir == 0) return gemm_form(M, K, N, 0);
  GemmArgs A = gemm_form(M, N, K, dir == 1 ? PF_MASK : 0);
  if (dir == 3) { A.stat_mode = 0; A.part = nullptr; }
  return A;
}

inline int query_route(int dir, int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return DL3_ROUTE_TILED;
  // dir 2: the weight gradient with the two-tensor operand; 4: with a single-tensor dY, folded by the launch (dw given)
  if (dir == 2 || dir == 4) return plan_wgrad(M, K, N, dir == 2, true, true, false, dir == 4).route;
  const int r = plan_gemm(canonical_args(dir == 0 || dir == 3 ? dir : 1, M, K, N)).plan[0].route;
  // dir 3 answers for the logits layer only (include/dl3.h): the narrow route or not — kept as it was
  return dir == 3 && r != DL3_ROUTE_NARROW ? DL3_ROUTE_TILED : r;
}

inline int query_fwd_impl(int M, int K, int N) {
  switch (query_route(0, M, K, N)) {
    case DL3_ROUTE_WS_HBM: return 1;
    case DL3_ROUTE_WS_MFMA:
    case DL3_ROUTE_NARROW: return 2;
    default: return 0;
  }
}

// Floors of dl3_pwconv_partials: rows that no plan writes, kept because the row count sizes the arenas and is an argument of
// the bn_finalize / fold launches of every lowered plan.  Dropping one is a change of its own, with a GPU A/B.
inline int partials_floor(int M, int K, int N) {
  int p = 0;
  const auto up = [&p](int q) { p = q > p ? q : p; };
  // the weight-stationary HBM grid for the kernel's (K, N) pairs below the route's 32 768-row threshold
  if (ws_tn(K, N)) up(ws_grid(M));
  // the 128x96 tile for every output made of whole 96-column tiles (the prefetching variant takes it for pre_wanted shapes only)
  if (N % 96 == 0) up(gemm_grid_y(M, N, kGemmCfgs[4], K));
  // the stream kernel's pick (32-row tiles allowed) for shapes it cannot take: a dimension that is no multiple of 4, or a
  // reduction beyond DL3_STREAM_KMAX
  if (K % 4 != 0 || N % 4 != 0 || K > DL3_STREAM_KMAX)
    for (int form = 0; form < 3; form++) up(gemm_grid_y(M, N, pick_gemm(M, K, N, form == 2, true, form == 0), K));
  return p;
}

// P for the [M, K] x [K, N] GEMM: the most rows any launch of that shape writes, whichever operand form and math it is given
// (the buffer is sized when a plan is lowered, and its row count is an argument of the bn_finalize / fold launches)
inline int query_partials(int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  static const unsigned kForms[] = {
      0,                            // forward (dl3_pwconv_fwd): every forward route
      PF_ADD,                       // forward with an addend (dl3_pwconv_fwd_add): tiled or K-split only
      PF_MASK,                      // bwd-data, single-tensor dY, masked: weight-stationary MFMA / the prefetching 128x96 tile
      PF_MASK | PF_ADD,             // ... with a residual: the cost model's tile
      PF_TWO | PF_MASK,             // bwd-data, two-tensor dY: the 384 -> 64 weight-stationary form / the prefetching tile
      PF_TWO | PF_MASK | PF_ADD,    // ... with a residual
  };
  int p = partials_floor(M, K, N);
  for (int split = 0; split < 2; split++)        // f32 MFMA / split math (which keeps every launch on the tiled kernels)
    for (unsigned un = 0; un < 2; un++)          // aligned (stream kernel, 32-row tiles allowed) / unaligned (LDS-staged kernel)
      for (const unsigned f : kForms) {
        const GemmLaunch L = plan_gemm(gemm_form(M, K, N, f | (un ? PF_UNALIGNED : 0)), split != 0);
        p = L.rows() > p ? L.rows() : p;
        // (a floor as well: each slice of a column split sized as a launch of its own in every form — a slice is never split again)
        for (int i = 0; L.n == 2 && i < 2; i++) {
          const int q = query_partials(M, K, L.args[i].N);
          p = q > p ? q : p;
        }
      }
  return p;
}

// the workspace of dl3_pwconv_bwd_weight*: slabs and column-sum rows of the largest of the launch's operand forms
inline size_t query_wgrad_workspace(int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  int S = 0, crows = 0;
  // two-tensor dY (slabs left to the caller or folded) / single-tensor dY folded by the launch (the narrow route's form) /
  // single-tensor dY with the slabs left to the caller
  const WgradPlan forms[] = {plan_wgrad(M, K, N, true, true, true, true, false, false), plan_wgrad(M, K, N, false, true, true, false, true, false),
                             plan_wgrad(M, K, N, false, true, true, false, false, false)};
  for (const WgradPlan &P : forms) {
    S = P.slabs > S ? P.slabs : S;
    crows = P.colsum_rows > crows ? P.colsum_rows : crows;
  }
  return ((size_t)S * K * N + (size_t)crows * N) * sizeof(float);
}

inline int query_wgrad_splits(int M, int K, int N, bool two) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  return plan_wgrad(M, K, N, two, true, true, false, false).S;
}

}  // namespace
