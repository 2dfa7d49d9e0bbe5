// pwgemm.hip — Conv2D 1x1 as fp32 GEMM on the CDNA4 matrix cores: the C entry points and the dispatch
// (deeplabv3p.py:78-79,:175,:194,:377,:385,:406,:420,:438; utils.py:189,:195).
//
// v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD).  One kernel family serves
//   forward   Y[M,N]  = T(X)[M,K] . W[K,N]            (prologue: BN+ReLU6 of the producer on load,
//                                                      epilogue: bias, BN batch-stat partials)
//   bwd-data  dX[M,K] = dY[M,N] . W^T[N,K]            (prologue: BN-backward affine of two tensors on
//                                                      load, epilogue: activation mask, residual
//                                                      gradient add, BN-backward stat partials)
// and a second one the weight gradient dW[K,N] = T(X)^T . dY (reduction over M = N*H*W, split
// over workgroups, folded deterministically).
//
// Fragment layouts (cdna_hip_programming.md §3): A lane l holds A[i=l&31][k=l>>5], B lane l holds
// B[k=l>>5][j=l&31]; C/D reg r of lane l is row (r&3)+8*(r>>2)+4*(l>>5), column l&31.
// LDS tiles are k-major (As[k][m], Bs[k][n]) so fragment reads are 32 consecutive floats per
// half-wave: conflict-free ds_read_b32.
// The kernels live one family per file, each with the launcher that switches over its instantiations (csrc/pwargs.h):
// pwstream.hip (PW_STREAM), pwlds.hip (PW_LDS), pwws.hip (PW_WS, PW_WS2, PW_NARROW_FLAT, PW_NARROWK), pwsmall.hip (PW_KSPLIT, the
// per-image rows), pwwgrad.hip (the weight gradient).  This file plans a call (csrc/pwplan.h: the one unit that includes it),
// checks its arguments and hands it to a launcher; the transposes are its only kernels.
#include "common.h"
#include "pwplan.h"  // the launch planner (host-only); GemmArgs, WgradArgs and the family launchers: pwargs.h

namespace {
// one launch of the plan P over the operands A; -1: the split-math weight scratch is unavailable (nothing launched).  Like
// every family launcher this is a switch over what the plan names and nothing else: no shape test, no environment variable.
int launch_gemm(GemmArgs A, const GemmPlan &P, void *stream) {
  A.mtiles = P.mtiles;
  switch (P.kernel) {
    case PW_STREAM: return launch_stream(A, P, stream);
    case PW_LDS: launch_lds(A, P, stream); break;
    case PW_KSPLIT: launch_ksplit(A, P, stream); break;
    default: launch_ws(A, P, stream); break;  // PW_WS, PW_WS2, PW_NARROW_FLAT, PW_NARROWK
  }
  return 0;
}

__global__ __launch_bounds__(256) void transpose_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                        int rows, int cols) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = in[(size_t)(r0 + i) * cols + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < cols && r0 + tx < rows) out[(size_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}

// all weight transposes of a backward pass in one launch: desc[m] = {in, out, rows, cols, first tile, tiles per row}
__global__ __launch_bounds__(256) void transpose_batched_kernel(const long long *__restrict__ desc, int n) {
  __shared__ float tile[32][33];
  int m = 0;
  while (m + 1 < n && (long long)blockIdx.x >= desc[(m + 1) * 6 + 4]) ++m;  // n is a few dozen
  const float *in = (const float *)desc[m * 6 + 0];
  float *out = (float *)desc[m * 6 + 1];
  const int rows = (int)desc[m * 6 + 2], cols = (int)desc[m * 6 + 3];
  const int t = blockIdx.x - (int)desc[m * 6 + 4], tx_ = (int)desc[m * 6 + 5];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = (t % tx_) * 32, r0 = (t / tx_) * 32;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = in[(size_t)(r0 + i) * cols + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < cols && r0 + tx < rows) out[(size_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}
}  // namespace

extern "C" int dl3_set_gemm_math(int mode) {
  DL3_CHECK_ARG(mode >= -1 && mode <= 1, "set_gemm_math: mode must be DL3_MATH_ENV, DL3_MATH_F32 or DL3_MATH_SPLIT");
  g_gemm_math = mode;
  return DL3_OK;
}

extern "C" int dl3_get_gemm_math(void) { return split_math() ? 1 : 0; }

// the queries are the planner's answers for the operand forms include/dl3.h documents (csrc/pwplan.h, query_*)
extern "C" int dl3_pwconv_partials(int M, int K, int N) { return query_partials(M, K, N); }
extern "C" int dl3_pwconv_fwd_impl(int M, int K, int N) { return query_fwd_impl(M, K, N); }
extern "C" int dl3_pwconv_route(int dir, int M, int K, int N) { return query_route(dir, M, K, N); }
extern "C" size_t dl3_pwconv_bwd_weight_workspace(int M, int K, int N) { return query_wgrad_workspace(M, K, N); }
extern "C" int dl3_pwconv_bwd_weight_splits(int M, int K, int N, int two_tensor_dy) {
  return query_wgrad_splits(M, K, N, two_tensor_dy != 0);
}

static int gemm_common_check(const char *name, int M, int K, int N) {
  DL3_CHECK_ARG(M > 0 && K > 0 && N > 0, "%s: non-positive dimension", name);
  return DL3_OK;
}

// plans the call (one launch, or the two of a column split), refuses a plan that would write more statistic partial rows than
// A.part_rows — before anything is launched — and launches it
static int run_gemm(const char *name, const GemmArgs &A, void *stream) {
  const GemmLaunch L = plan_gemm(A);
  for (int i = 0; i < L.n; i++)
    DL3_CHECK_ARG(!A.part || L.plan[i].rows <= A.part_rows,
                  "%s: M=%d K=%d N=%d: the launch writes %d statistic partial rows, the buffer holds %d (dl3_pwconv_partials)", name,
                  A.M, A.K, A.N, L.plan[i].rows, A.part_rows);
  for (int i = 0; i < L.n; i++)
    DL3_CHECK_ARG(launch_gemm(L.args[i], L.plan[i], stream) >= 0,
                  "%s: split-math weight scratch unavailable (first launch inside a stream capture?)", name);
  DL3_LAUNCH_CHECK(name);
  return DL3_OK;
}

// (tools/pwplan_probe.cpp builds the GemmArgs of a forward and of a bwd-data call the way pwconv_fwd and dl3_pwconv_bwd_data below do,
// and the xvec / dvec of the weight gradient: a change to what these functions put into a field the planner reads goes there too)
// dl3_pwconv_fwd (add == NULL) and dl3_pwconv_fwd_add
static int pwconv_fwd(const char *name, const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                      const float *w, const float *bias, float *y, int ldy, int M, int K, int N, float *stat_partial,
                      bool with_add, const float *add, int ldadd, int add_div, void *stream) {
  int rc = gemm_common_check(name, M, K, N);
  if (rc) return rc;
  DL3_CHECK_ARG(x && w && y && (add || !with_add), "%s: null pointer", name);
  DL3_CHECK_ARG(ldx >= K && ldy >= N && (!with_add || (ldadd >= N && add_div >= 1)),
                with_add ? "%s: bad leading dimension / add_div" : "%s: leading dimension too small", name);
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "%s: scale/shift must come together", name);
  GemmArgs A{};
  A.a = x; A.lda = ldx; A.a2 = nullptr; A.lda2 = 0;
  A.ka = in_scale; A.kb = nullptr; A.kc = in_shift; A.a_act = in_act;
  A.b = w; A.ldb = N; A.bias = bias; A.c = y; A.ldc = ldy;
  A.M = M; A.K = K; A.N = N;
  A.ep_add = add; A.ld_add = with_add ? ldadd : 0; A.add_div = with_add ? add_div : 1; A.add_scale = 1.f;
  A.stat_mode = stat_partial ? 1 : 0;
  A.part = stat_partial;
  A.part_rows = stat_partial ? dl3_pwconv_partials(M, K, N) : 0;
  return run_gemm(name, A, stream);
}

extern "C" int dl3_pwconv_fwd(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                              const float *w, const float *bias, float *y, int ldy, int M, int K, int N,
                              float *stat_partial, void *stream) {
  return pwconv_fwd("pwconv_fwd", x, ldx, in_scale, in_shift, in_act, w, bias, y, ldy, M, K, N, stat_partial, false, nullptr, 0, 1,
                    stream);
}

extern "C" int dl3_pwconv_fwd_add(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                                  const float *w, const float *bias, float *y, int ldy, int M, int K, int N,
                                  float *stat_partial, const float *add, int ldadd, int add_div, void *stream) {
  return pwconv_fwd("pwconv_fwd_add", x, ldx, in_scale, in_shift, in_act, w, bias, y, ldy, M, K, N, stat_partial, true, add, ldadd,
                    add_div, stream);
}

extern "C" int dl3_pwconv_fwd_rows(const float *x, int ldx, const float *in_scale, const float *in_shift, int in_act,
                                   const float *w, const float *bias, float *y, int ldy, int M, int K, int N,
                                   const float *add, int ldadd, int add_div, void *stream) {
  int rc = gemm_common_check("pwconv_fwd_rows", M, K, N);
  if (rc) return rc;
  DL3_CHECK_ARG(x && w && y, "pwconv_fwd_rows: null pointer");
  DL3_CHECK_ARG(ldx >= K && ldy >= N && (!add || (ldadd >= N && add_div >= 1)), "pwconv_fwd_rows: bad leading dimension / add_div");
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "pwconv_fwd_rows: scale/shift must come together");
  DL3_UNSUPPORTED(M > 65535, "pwconv_fwd_rows: a few rows (one per image), not %d", M);
  GemmArgs A{};
  A.a = x; A.lda = ldx; A.ka = in_scale; A.kc = in_shift; A.a_act = in_act;
  A.b = w; A.ldb = N; A.bias = bias; A.c = y; A.ldc = ldy;
  A.M = M; A.K = K; A.N = N;
  A.ep_add = add; A.ld_add = ldadd; A.add_div = add_div < 1 ? 1 : add_div; A.add_scale = 1.f;
  launch_rows(A, stream);
  DL3_LAUNCH_CHECK("pwconv_fwd_rows");
  return DL3_OK;
}

extern "C" int dl3_pwconv_bwd_data(const float *g, int ldg, const float *yraw, int ldyraw, const float *cA,
                                   const float *cB, const float *cC, const float *wT, float *dx, int lddx,
                                   const float *x, int ldx, const float *in_scale, const float *in_shift,
                                   int in_act, const float *dx_add, int ldadd, int add_div, float add_scale,
                                   const float *x_mean, const float *x_invstd, float *dstat_partial, int M,
                                   int K, int N, void *stream) {
  int rc = gemm_common_check("pwconv_bwd_data", M, K, N);
  if (rc) return rc;
  DL3_CHECK_ARG(g && wT && dx, "pwconv_bwd_data: null pointer");
  DL3_CHECK_ARG(!cA || (yraw && cB && cC), "pwconv_bwd_data: cA needs yraw, cB, cC");
  DL3_CHECK_ARG(in_act == DL3_ACT_NONE || x, "pwconv_bwd_data: activation mask needs x");
  DL3_CHECK_ARG(!dstat_partial || (x && x_mean && x_invstd), "pwconv_bwd_data: dstat needs x, x_mean, x_invstd");
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "pwconv_bwd_data: scale/shift must come together");
  // GEMM [M, N] x [N, K] -> [M, K]
  GemmArgs A{};
  A.a = g; A.lda = ldg;
  A.a2 = cA ? yraw : nullptr; A.lda2 = ldyraw;
  A.ka = cA; A.kb = cB; A.kc = cC; A.a_act = DL3_ACT_NONE;
  A.b = wT; A.ldb = K; A.bias = nullptr; A.c = dx; A.ldc = lddx;
  A.M = M; A.K = N; A.N = K;
  const bool need_x = (in_act != DL3_ACT_NONE) || dstat_partial;
  A.ep_x = need_x ? x : nullptr; A.ld_epx = ldx;
  A.ep_scale = in_scale; A.ep_shift = in_shift; A.ep_act = in_act;
  A.ep_add = dx_add; A.ld_add = ldadd; A.add_div = add_div < 1 ? 1 : add_div; A.add_scale = add_scale;
  A.stat_mode = dstat_partial ? 2 : 0;
  A.ep_mean = x_mean; A.ep_invstd = x_invstd;
  A.part = dstat_partial;
  A.part_rows = dstat_partial ? dl3_pwconv_partials(M, N, K) : 0;
  return run_gemm("pwconv_bwd_data", A, stream);
}

static int pwconv_bwd_weight_impl(const float *x, int ldx, const float *in_scale, const float *in_shift,
                                     int in_act, const float *g, int ldg, const float *yraw, int ldyraw,
                                     const float *cA, const float *cB, const float *cC, float *dw, float *dbias,
                                     int M, int K, int N, void *workspace, size_t workspace_bytes, float *dy_out, int lddy,
                                     void *stream) {
  int rc = gemm_common_check("pwconv_bwd_weight", M, K, N);
  if (rc) return rc;
  DL3_CHECK_ARG(!dy_out || (lddy >= N && lddy % 4 == 0 && al16(dy_out)),
                "pwconv_bwd_weight_dy: dy_out must be 16-byte aligned with a leading dimension >= N that is a multiple of 4");
  DL3_CHECK_ARG(x && g && workspace, "pwconv_bwd_weight: null pointer");
  DL3_CHECK_ARG(dw || !dbias, "pwconv_bwd_weight: dbias without dw (slabs left in the workspace) is not supported");
  DL3_CHECK_ARG(!cA || (yraw && cB && cC), "pwconv_bwd_weight: cA needs yraw, cB, cC");
  DL3_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "pwconv_bwd_weight: scale/shift must come together");
  DL3_UNSUPPORTED(dbias && cA, "pwconv_bwd_weight: dbias with a BN-backward gradient operand is not needed by the path");
  if (workspace_bytes < dl3_pwconv_bwd_weight_workspace(M, K, N)) {
    dl3_set_error("pwconv_bwd_weight: workspace %zu < %zu bytes", workspace_bytes,
                  dl3_pwconv_bwd_weight_workspace(M, K, N));
    return DL3_EWORKSPACE;
  }
  const bool two = cA != nullptr;
  const bool xvec = (K % 4 == 0) && (ldx % 4 == 0) && al16(x);
  const bool dvec = (N % 4 == 0) && (ldg % 4 == 0) && al16(g) && (!two || ((ldyraw % 4 == 0) && al16(yraw)));
  const WgradPlan P = plan_wgrad(M, K, N, two, xvec, dvec, dy_out != nullptr, dw != nullptr);
  WgradArgs A{};
  A.x = x; A.ldx = ldx; A.xs = in_scale; A.xt = in_shift; A.x_act = in_act;
  A.g = g; A.ldg = ldg; A.y = two ? yraw : nullptr; A.ldy = ldyraw;
  A.cA = cA; A.cB = cB; A.cC = cC;
  A.ws = (float *)workspace;
  A.M = M; A.K = K; A.N = N;
  A.dyout = dy_out; A.lddy = lddy;
  A.Mper = P.Mper;
  float *cpart = dbias ? A.ws + (size_t)P.slabs * K * N : nullptr;   // the column sums of the bias gradient, behind the slabs
  launch_wgrad(A, P, cpart, stream);
  DL3_LAUNCH_CHECK(P.narrow ? "pwconv_bwd_weight(narrow)" : "pwconv_bwd_weight");
  if (!dw) return DL3_OK;  // the caller folds the [S][K][N] slabs itself (dl3_reduce_partials / _batched)
  rc = dl3_reduce_partials(A.ws, P.slabs, K * N, dw, stream);
  if (rc || !dbias) return rc;
  if (!P.narrow) {   // (the narrow kernel wrote its column sums itself)
    launch_colsum(g, ldg, M, N, P.colsum_rows, cpart, stream);
    DL3_LAUNCH_CHECK("pwconv_bwd_weight(colsum)");
  }
  return dl3_reduce_partials(cpart, P.colsum_rows, N, dbias, stream);
}

extern "C" int dl3_pwconv_bwd_weight(const float *x, int ldx, const float *in_scale, const float *in_shift,
                                     int in_act, const float *g, int ldg, const float *yraw, int ldyraw,
                                     const float *cA, const float *cB, const float *cC, float *dw, float *dbias,
                                     int M, int K, int N, void *workspace, size_t workspace_bytes, void *stream) {
  return pwconv_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, g, ldg, yraw, ldyraw, cA, cB, cC, dw, dbias, M, K, N,
                                workspace, workspace_bytes, nullptr, 0, stream);
}

extern "C" int dl3_pwconv_bwd_weight_dy(const float *x, int ldx, const float *in_scale, const float *in_shift,
                                        int in_act, const float *g, int ldg, const float *yraw, int ldyraw,
                                        const float *cA, const float *cB, const float *cC, float *dw, float *dbias,
                                        int M, int K, int N, void *workspace, size_t workspace_bytes, float *dy_out,
                                        int lddy, void *stream) {
  DL3_CHECK_ARG(dy_out, "pwconv_bwd_weight_dy: dy_out is NULL (use dl3_pwconv_bwd_weight)");
  return pwconv_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, g, ldg, yraw, ldyraw, cA, cB, cC, dw, dbias, M, K, N,
                                workspace, workspace_bytes, dy_out, lddy, stream);
}

extern "C" int dl3_transpose(const float *in, float *out, int rows, int cols, void *stream) {
  DL3_CHECK_ARG(in && out && rows > 0 && cols > 0, "transpose: bad argument");
  dim3 grid(dl3_cdiv(cols, 32), dl3_cdiv(rows, 32));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, rows, cols);
  DL3_LAUNCH_CHECK("transpose");
  return DL3_OK;
}

extern "C" int dl3_transpose_batched(const long long *desc, int n, int total_tiles, void *stream) {
  DL3_CHECK_ARG(desc && n > 0 && total_tiles > 0, "transpose_batched: bad argument");
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, desc, n);
  DL3_LAUNCH_CHECK("transpose_batched");
  return DL3_OK;
}
