// pwargs.h — what crosses the translation units of the 1x1-convolution GEMMs: the argument structs the kernels take, the plans
// csrc/pwplan.h writes, and the launchers of the kernel files (called from pwgemm.hip).  Host-only C++17 (g++ -fsyntax-only
// pwargs.h): no HIP type, a stream crosses as void *.  No state lives here: any number of units may include it.
#pragma once
// build macros the kernels themselves read (the planner sizes grids and workspaces by the same values)
#ifndef DL3_STREAM_KMAX
#define DL3_STREAM_KMAX 2048  // largest reduction depth the stream kernel takes (coefficient vectors in LDS)
#endif
#ifndef DL3_WGRAD_MS
#define DL3_WGRAD_MS 16
#endif
#ifndef DL3_WS2_NW
#define DL3_WS2_NW 8  // waves per workgroup of the weight-stationary MFMA kernels (pw_ws2_kernel, pw_narrowk_kernel, pw_wgrad_narrow_kernel)
#endif

namespace pw {  // (named: a launcher called across translation units cannot take an anonymous-namespace type)
struct GemmArgs {
  const float *a; int lda;
  const float *a2; int lda2;
  const float *ka, *kb, *kc; int a_act;
  const float *b; int ldb;
  const float *bias;
  float *c; int ldc;
  int M, K, N;
  const float *ep_x; int ld_epx;
  const float *ep_scale, *ep_shift; int ep_act;
  const float *ep_add; int ld_add; int add_div; float add_scale;
  int stat_mode;  // 0 none, 1: sum c, sum c^2 ; 2: sum c, sum c*xhat
  const float *ep_mean, *ep_invstd;
  float *part;
  int part_rows;  // rows the caller's partial buffer holds: the launch writes GemmPlan::rows of them and zeroes the rest itself
  int part_ld;    // columns per partial row (0: N) — a launch over a column slice of the output (plan_gemm) writes into the whole matrix's rows
  int mtiles;
  const void *bp; int nsub;  // split math: weights pre-split into 3 bf16 planes in MFMA fragment order (pack_b_kernel)
};
// weight gradient: dW[K,N] (+)= sum_m T(X)[m][k] * dY[m][n]; grid (ntn, ntk, S)
struct WgradArgs {
  const float *x; int ldx;
  const float *xs, *xt; int x_act;
  const float *g; int ldg;
  const float *y; int ldy;
  const float *cA, *cB, *cC;
  float *ws;  // [S][K][N]
  int M, K, N, Mper;
  float *dyout; int lddy;  // nullable: dY = cA*g + cB*y + cC written out [M][N] by the workgroups of the first K-tile row
};

// ---- what a launch is ------------------------------------------------------------------
enum GemmKernel {
  PW_LDS,          // pw_gemm_kernel<cfg>: unaligned operands or a reduction beyond DL3_STREAM_KMAX; vmode
  PW_STREAM,       // pw_gemm_stream_kernel<cfg>: two / fwd / pre (the prefetching epilogue, cfg 4 only) / split (MATH 1)
  PW_KSPLIT,       // pw_ksplit32_kernel<tn, two>
  PW_WS,           // pw_fwd_ws_kernel<kq, tn>
  PW_WS2,          // pw_ws2_kernel<kq, tn>: forward (fwd), bwd-data (!fwd; two: the 384 -> 64 form, add: with its residual)
  PW_NARROW_FLAT,  // pw_ws2_kernel<32, 1, FLAT>: the logits layer's forward, packed output rows
  PW_NARROWK,      // pw_narrowk_kernel<8>: the logits layer's bwd-data
};
struct GemmPlan {
  int route;  // DL3_ROUTE_*
  GemmKernel kernel;
  int cfg;     // tiled kernels: index into kGemmCfgs
  int kq, tn;  // the weight-stationary and K-split kernels' instantiation
  int vmode;   // 1 = 16-byte loads on both operands, 0 = scalar loads on both (tiny GEMMs with K = number of classes), 2 = on
               // the activation operand only (N = number of classes — the logits layer's forward)
  bool two, fwd, pre, add, split;
  int grid[3];
  unsigned lds;  // dynamic LDS bytes
  int mtiles;    // tiled kernels: row tiles the workgroups loop over
  int rows;      // statistic partial rows the launch writes (it zeroes rows .. part_rows)
};
struct WgradPlan {
  int route;  // DL3_ROUTE_TILED, _WGRAD_ROW or _NARROW
  int cfg;    // index into kWgCfgs (tiled and one-tile-row kernels)
  bool narrow, row;
  int vec;    // tiled kernel: 1 = 16-byte loads of x and of g / y, 0 = scalar loads of both, 2 = 16-byte loads of x only
  bool split;
  int S, Mper;  // M splits of the tiled / one-tile-row launch and rows per split
  int grid[3];
  int slabs;        // K x N slabs at the head of the workspace the launch writes
  int colsum_rows;  // rows of N column sums behind them when a bias gradient is asked for
};

// ---- the family launchers: csrc/pwplan.h decides (route, instantiation, grid, LDS bytes, partial rows); a launcher holds the switch
// over the template instantiations of its file that a plan names and nothing else: no shape test, no environment variable
void launch_lds(const GemmArgs &A, const GemmPlan &P, void *stream);     // PW_LDS
int launch_stream(GemmArgs A, const GemmPlan &P, void *stream);          // PW_STREAM; -1: no split-math weight scratch (nothing launched)
void launch_ws(const GemmArgs &A, const GemmPlan &P, void *stream);      // PW_WS, PW_WS2, PW_NARROW_FLAT, PW_NARROWK
void launch_ksplit(const GemmArgs &A, const GemmPlan &P, void *stream);  // PW_KSPLIT
void launch_rows(const GemmArgs &A, void *stream);                       // dl3_pwconv_fwd_rows
// cpart: the narrow kernel's column sums for the bias gradient, nullable; the tiled routes' come from launch_colsum (part[rows][N])
void launch_wgrad(const WgradArgs &A, const WgradPlan &P, float *cpart, void *stream);
void launch_colsum(const float *g, int ldg, int M, int N, int rows, float *part, void *stream);
}  // namespace pw
