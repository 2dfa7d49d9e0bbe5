// pwplan_probe.cpp — the 1x1-convolution launch planner (csrc/pwplan.h) asked from the host, one JSON line per argument: which
// kernel, instantiation, grid and buffer sizes plan_gemm / plan_wgrad give for a launch of a stated shape and operand form.
// tests/test_pwconv_cases_host.py compiles it with the host compiler and holds every case of tests/pwconv_cases.py to the
// plan it declares.  A separate program: the one-inclusion rule of csrc/ (tests/test_host.py) is about the library's units.
//
//   g++ -std=c++17 -I <package>/csrc tools/pwplan_probe.cpp -o pwplan_probe
//   pwplan_probe f:M:K:N:flags:split:ldx:ldy:add_div  b:M:K:N:flags:split:ldg:lddx:ldx:add_div  w:M:K:N:flags:split  q:M:K:N
//
// f: a dl3_pwconv_fwd / _fwd_add call, b: a dl3_pwconv_bwd_data call, w: a dl3_pwconv_bwd_weight / _dy call — all with the
// LAYER's (M, K, N) and leading dimensions, the operands built as csrc/pwgemm.hip builds them; q: the sizing queries of the C
// ABI.  split: 0 f32 MFMA, 1 split math.  The knobs the planner reads from the environment (DL3_GEMM_CFG, DL3_WGRAD_CFG,
// DL3_GEMM_PRE, DL3_GEMM_PY per call; DL3_WS2, DL3_NARROW, DL3_COLSPLIT, DL3_WGRAD_ROW once per process) are this process's.
#include <stdio.h>
#include <string.h>

#include "pwplan.h"

namespace {
enum {
  F_TWO = 1,         // b, w: two-tensor dY (cA given)
  F_ACT = 2,         // in_act != DL3_ACT_NONE
  F_ADD = 4,         // f: an addend (dl3_pwconv_fwd_add); b: dx_add
  F_UNALIGNED = 8,   // f, b: every operand 4 bytes off a 16-byte boundary; w: x
  F_STATS = 16,      // f: stat_partial; b: dstat_partial (with x, x_mean, x_invstd)
  F_BIAS = 32,       // f: bias
  F_XFORM = 64,      // in_scale / in_shift given
  F_DUNALIGNED = 128,  // w: g (and yraw) 4 bytes off a 16-byte boundary
  F_DYOUT = 256,     // w: dy_out given (dl3_pwconv_bwd_weight_dy)
  F_DW = 512,        // w: dw given (the launch folds its slabs)
};

const char *kernel_name(GemmKernel k) {
  switch (k) {
    case PW_LDS: return "lds";
    case PW_STREAM: return "stream";
    case PW_KSPLIT: return "ksplit";
    case PW_WS: return "ws";
    case PW_WS2: return "ws2";
    case PW_NARROW_FLAT: return "flat";
    case PW_NARROWK: return "narrowk";
  }
  return "?";
}

void print_gemm(const GemmLaunch &L) {
  printf("{\"n\": %d, \"rows\": %d, \"plans\": [", L.n, L.rows());
  for (int i = 0; i < L.n; i++) {
    const GemmPlan &P = L.plan[i];
    // the tile a workgroup (tiled kernels) or a wave (weight-stationary, K-split) walks: rows x columns, and the depth of a K step
    int bm = 32, bn = 32, kt = 0;
    if (P.kernel == PW_STREAM || P.kernel == PW_LDS) {
      bm = kGemmCfgs[P.cfg].BM; bn = kGemmCfgs[P.cfg].BN;
      kt = P.kernel == PW_LDS ? 16 : (P.split ? 32 : 16);
    } else if (P.kernel == PW_KSPLIT || P.kernel == PW_WS || P.kernel == PW_WS2) {
      bn = 32 * P.tn; kt = 8;
    } else if (P.kernel == PW_NARROWK) {
      bn = 256; kt = 8;
    }
    printf("%s{\"route\": %d, \"kernel\": \"%s\", \"cfg\": %d, \"kq\": %d, \"tn\": %d, \"vmode\": %d, \"two\": %d, \"fwd\": %d, "
           "\"pre\": %d, \"add\": %d, \"split\": %d, \"grid\": [%d, %d, %d], \"lds\": %u, \"mtiles\": %d, \"rows\": %d, "
           "\"M\": %d, \"K\": %d, \"N\": %d, \"BM\": %d, \"BN\": %d, \"KT\": %d}",
           i ? ", " : "", P.route, kernel_name(P.kernel), P.cfg, P.kq, P.tn, P.vmode, (int)P.two, (int)P.fwd, (int)P.pre, (int)P.add,
           (int)P.split, P.grid[0], P.grid[1], P.grid[2], P.lds, P.mtiles, P.rows, L.args[i].M, L.args[i].K, L.args[i].N, bm, bn, kt);
  }
  printf("]}\n");
}

int field(char *&s) {
  if (!s) return 0;
  char *e = strchr(s, ':');
  const int v = atoi(s);
  s = e ? e + 1 : nullptr;
  return v;
}
}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    char *s = argv[i];
    const char kind = s[0];
    if (!kind || s[1] != ':') { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    s += 2;
    const int M = field(s), K = field(s), N = field(s);
    if (kind == 'q') {
      printf("{\"route\": [%d, %d, %d, %d, %d], \"fwd_impl\": %d, \"partials\": %d, \"partials_bwd\": %d, \"workspace\": %zu, "
             "\"splits\": [%d, %d]}\n", query_route(0, M, K, N), query_route(1, M, K, N), query_route(2, M, K, N),
             query_route(3, M, K, N), query_route(4, M, K, N), query_fwd_impl(M, K, N), query_partials(M, K, N),
             query_partials(M, N, K), query_wgrad_workspace(M, K, N), query_wgrad_splits(M, K, N, false),
             query_wgrad_splits(M, K, N, true));
      continue;
    }
    const unsigned flags = (unsigned)field(s);
    const bool split = field(s) != 0;
    float *const p = kPlanOperand + ((flags & F_UNALIGNED) ? 1 : 0);
    if (kind == 'f') {
      const int ldx = field(s), ldy = field(s), add_div = field(s);
      GemmArgs A{};
      A.a = p; A.lda = ldx;
      if (flags & F_XFORM) A.ka = A.kc = p;
      A.a_act = (flags & F_ACT) ? DL3_ACT_RELU : DL3_ACT_NONE;
      A.b = p; A.ldb = N; A.bias = (flags & F_BIAS) ? p : nullptr; A.c = p; A.ldc = ldy;
      A.M = M; A.K = K; A.N = N;
      A.ep_add = (flags & F_ADD) ? p : nullptr; A.ld_add = (flags & F_ADD) ? N : 0;
      A.add_div = (flags & F_ADD) ? add_div : 1; A.add_scale = 1.f;
      A.stat_mode = (flags & F_STATS) ? 1 : 0;
      A.part = (flags & F_STATS) ? p : nullptr;
      A.part_rows = A.part ? query_partials(M, K, N) : 0;
      print_gemm(plan_gemm(A, split));
    } else if (kind == 'b') {
      const int ldg = field(s), lddx = field(s), ldx = field(s), add_div = field(s);
      GemmArgs A{};
      A.a = p; A.lda = ldg;
      if (flags & F_TWO) { A.a2 = p; A.lda2 = ldg; A.ka = A.kb = A.kc = p; }
      A.a_act = DL3_ACT_NONE;
      A.b = p; A.ldb = K; A.c = p; A.ldc = lddx;
      A.M = M; A.K = N; A.N = K;
      const bool need_x = (flags & (F_ACT | F_STATS)) != 0;
      A.ep_x = need_x ? p : nullptr; A.ld_epx = ldx;
      if (flags & F_XFORM) A.ep_scale = A.ep_shift = p;
      A.ep_act = (flags & F_ACT) ? DL3_ACT_RELU : DL3_ACT_NONE;
      A.ep_add = (flags & F_ADD) ? p : nullptr; A.ld_add = add_div > 1 ? K : lddx;
      A.add_div = add_div < 1 ? 1 : add_div; A.add_scale = 2.f;
      A.stat_mode = (flags & F_STATS) ? 2 : 0;
      if (flags & F_STATS) { A.ep_mean = A.ep_invstd = p; A.part = p; }
      A.part_rows = A.part ? query_partials(M, N, K) : 0;
      print_gemm(plan_gemm(A, split));
    } else if (kind == 'w') {
      const bool two = flags & F_TWO, xvec = K % 4 == 0 && !(flags & F_UNALIGNED), dvec = N % 4 == 0 && !(flags & F_DUNALIGNED);
      const WgradPlan P = plan_wgrad(M, K, N, two, xvec, dvec, (flags & F_DYOUT) != 0, (flags & F_DW) != 0, split);
      printf("{\"route\": %d, \"kernel\": \"%s\", \"cfg\": %d, \"vec\": %d, \"split\": %d, \"S\": %d, \"Mper\": %d, "
             "\"grid\": [%d, %d, %d], \"slabs\": %d, \"colsum_rows\": %d, \"BKT\": %d, \"BNT\": %d, \"MS\": %d}\n",
             P.route, P.narrow ? "wgrad_narrow" : (P.row ? "wgrad_row" : "wgrad"), P.cfg, P.vec, (int)P.split, P.S, P.Mper, P.grid[0],
             P.grid[1], P.grid[2], P.slabs, P.colsum_rows, kWgCfgs[P.cfg].BKT, kWgCfgs[P.cfg].BNT, DL3_WGRAD_MS);
    } else {
      fprintf(stderr, "bad argument %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
