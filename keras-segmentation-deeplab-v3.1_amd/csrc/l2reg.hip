// l2reg.hip — the L2 weight penalty of Keras' kernel_regularizer=l2(l) over the regularised runs of a flat arena
// (dl3_l2_penalty): the value l * sum(w^2) in double, and its gradient 2*l*w added onto the gradient arena in front of
// the clip and the step.  DESIGN.md §19.
// [TF-semantics: Keras 2.2.4 keras/regularizers.py (L1L2.__call__) and keras/engine/training.py (total_loss += the
// layers' losses), restated from memory.]
#include "common.h"

#define L2_TILE 1024         // elements of ONE run per workgroup trip: 256 lanes x one 16-byte load
#define L2_MAX_BLOCKS 2048   // 256 CUs x 8 workgroups, as dl3_grad_sumsq: the rest is grid-stride over the tiles

static inline int l2_blocks(long long tiles) { return (int)(tiles > L2_MAX_BLOCKS ? L2_MAX_BLOCKS : (tiles < 1 ? 1 : tiles)); }

// the addend of one element onto g: ((2l) * w) / sc — the step's later multiplication by sc returns 2*l*w
__device__ __forceinline__ float l2_addend(float w, float c2, float sc) { return (c2 * w) / sc; }

// pass 1: workgroup b takes the tiles b, b + gridDim, ...; a tile's run is the last one whose first tile is <= the tile
// (binary search over runs[.][2]), its elements [first + k*L2_TILE, first + min(length, (k+1)*L2_TILE)).  Lane t of a
// tile takes the elements 4t .. 4t+3 (VEC: p, g and the run's start 16-byte aligned; a quad cut by the run's end goes
// element by element) or t, t+256, ... (scalar).  partial[b] = sum over its tiles of coef * (the tile's sum of squares):
// which element goes to which lane depends on (the table, gridDim) only.
template <bool GRAD>
__global__ __launch_bounds__(256) void l2_penalty_kernel(const float *__restrict__ p, float *__restrict__ g,
                                                         const long long *__restrict__ runs,
                                                         const float *__restrict__ coef, int S, long long tiles,
                                                         float grad_scale, const float *__restrict__ denom, int base_vec,
                                                         double *__restrict__ partial) {
  __shared__ double sh[4];
  float sc = 1.f;
  if (GRAD) sc = denom ? grad_scale / fmaxf(denom[0], 1e-20f) : grad_scale;  // grad_xform's sc (optim.hip)
  double acc = 0.0;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (runs[3 * mid + 2] <= t)
        lo = mid;
      else
        hi = mid - 1;
    }
    const long long first = runs[3 * lo], k0 = (t - runs[3 * lo + 2]) * L2_TILE, left = runs[3 * lo + 1] - k0;
    const int m = left < L2_TILE ? (int)left : L2_TILE;  // >= 1 by the table's contract; <= 0 does nothing
    const float c = coef[lo], c2 = 2.f * c;
    const float *pt = p + first + k0;
    float *gt = GRAD ? g + first + k0 : nullptr;
    double s = 0.0;
    if (base_vec && (first & 3) == 0) {
      const int i = 4 * (int)threadIdx.x;
      if (i + 4 <= m) {
        const f32x4 w = ld4(pt + i);
        f32x4 gv = GRAD ? ld4(gt + i) : splat4(0.f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (GRAD) gv[k] += l2_addend(w[k], c2, sc);
          s += (double)w[k] * (double)w[k];  // exact: 24 x 24 bits
        }
        if (GRAD) st4(gt + i, gv);
      } else {
        for (int j = i; j < m; j++) {
          const float w = pt[j];
          if (GRAD) gt[j] += l2_addend(w, c2, sc);
          s += (double)w * (double)w;
        }
      }
    } else {
      for (int j = threadIdx.x; j < m; j += 256) {
        const float w = pt[j];
        if (GRAD) gt[j] += l2_addend(w, c2, sc);
        s += (double)w * (double)w;
      }
    }
    acc += (double)c * s;
  }
  const double total = block_sum256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// pass 2: ONE workgroup folds the partials in ascending order (fold_partials256, dl3_grad_sumsq's fold); out[1] is out[0]
// rounded once to float.  P == 0 (no run at all) writes zeros.
__global__ __launch_bounds__(256) void l2_fold_kernel(const double *__restrict__ partial, int P,
                                                      double *__restrict__ out) {
  __shared__ double sh[4];
  const double s = fold_partials256(partial, P, sh);
  if (threadIdx.x == 0) {
    out[0] = s;
    out[1] = (double)(float)s;
  }
}

extern "C" size_t dl3_l2_penalty_workspace_bytes(long long tiles) { return (size_t)l2_blocks(tiles) * sizeof(double); }

extern "C" int dl3_l2_penalty(const float *p, float *g, const long long *runs, const float *coef, int S, long long tiles,
                              float grad_scale, const float *denom, double *out, void *workspace, size_t workspace_bytes,
                              void *stream) {
  DL3_CHECK_ARG(S >= 0 && p && out && runs && (coef || S == 0), "l2_penalty: bad argument");
  DL3_CHECK_ARG(S == 0 ? tiles == 0 : tiles >= S, "l2_penalty: %lld tiles for %d runs (every run has at least one)", tiles, S);
  DL3_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "l2_penalty: out / workspace not 8-byte aligned");
  DL3_CHECK_ARG(!g || (grad_scale > 0.f && grad_scale < __builtin_inff()),
                "l2_penalty: the gradient addend is divided by the scale: grad_scale must be positive and finite");
  if (S > 0 && (!workspace || workspace_bytes < dl3_l2_penalty_workspace_bytes(tiles))) {  // S == 0 folds no partial
    dl3_set_error("l2_penalty: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0,
                  dl3_l2_penalty_workspace_bytes(tiles));
    return DL3_EWORKSPACE;
  }
  double *partial = (double *)workspace;
  const int P = S == 0 ? 0 : l2_blocks(tiles);
  if (P > 0) {
    const int base_vec = ((((uintptr_t)p | (uintptr_t)g) & 15) == 0) ? 1 : 0;
    if (g)
      hipLaunchKernelGGL(l2_penalty_kernel<true>, dim3(P), dim3(256), 0, (hipStream_t)stream, p, g, runs, coef, S, tiles,
                         grad_scale, denom, base_vec, partial);
    else
      hipLaunchKernelGGL(l2_penalty_kernel<false>, dim3(P), dim3(256), 0, (hipStream_t)stream, p, g, runs, coef, S, tiles,
                         grad_scale, denom, base_vec, partial);
    DL3_LAUNCH_CHECK("l2_penalty");
  }
  hipLaunchKernelGGL(l2_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, P, out);
  DL3_LAUNCH_CHECK("l2_penalty fold");
  return DL3_OK;
}
