// optim.hip — the optimizer step beyond plain Adam: the global gradient norm (dl3_grad_sumsq) and one update launch
// for SGD / RMSprop / clipped Adam over the flat parameter arena (dl3_opt_step).  DESIGN.md §11.
// [TF-semantics: Keras 2.2.4 keras/optimizers.py (Optimizer.get_gradients, SGD, RMSprop, Adam.get_updates), restated
// from memory.]
#include "common.h"

#define SUMSQ_MAX_BLOCKS 2048  // 256 CUs x 8 workgroups: one resident wave of workgroups, the rest is grid-stride

static inline int sumsq_blocks(size_t n) {
  size_t b = (n / 4 + 255) / 256;  // one 16-byte load per lane and trip
  if (b > SUMSQ_MAX_BLOCKS) b = SUMSQ_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// pass 1: partial[block] = sum of g[i]^2 over the block's grid-stride share, accumulated in double.  Which element goes
// to which lane depends on (n, VEC, gridDim) only, so a repeat of the launch adds the same numbers in the same order.
template <bool VEC>
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float *__restrict__ g, size_t n,
                                                            double *__restrict__ partial) {
  __shared__ double sh[4];
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  double acc = 0.0;
  if (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += stride) {
      const f32x4 v = ld4(g + 4 * i);
      acc += (double)v.x * (double)v.x;
      acc += (double)v.y * (double)v.y;
      acc += (double)v.z * (double)v.z;
      acc += (double)v.w * (double)v.w;
    }
    const size_t i = 4 * n4 + tid;  // scalar tail: at most 3 elements, lanes 0..2 of workgroup 0
    if (i < n) acc += (double)g[i] * (double)g[i];
  } else {
    for (size_t i = tid; i < n; i += stride) acc += (double)g[i] * (double)g[i];
  }
  const double s = block_sum256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// pass 2: ONE workgroup folds the partials in a fixed order (fold_partials256, common.h)
__global__ __launch_bounds__(256) void sumsq_fold_kernel(const double *__restrict__ partial, int P,
                                                         double *__restrict__ out) {
  __shared__ double sh[4];
  const double s = fold_partials256(partial, P, sh);
  if (threadIdx.x == 0) out[0] = s;
}

extern "C" size_t dl3_grad_sumsq_workspace_bytes(size_t n) { return (size_t)sumsq_blocks(n) * sizeof(double); }

extern "C" int dl3_grad_sumsq(const float *g, size_t n, double *out, void *workspace, size_t workspace_bytes,
                              void *stream) {
  DL3_CHECK_ARG(g && out && n > 0, "grad_sumsq: bad argument");
  DL3_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "grad_sumsq: out / workspace not 8-byte aligned");
  if (!workspace || workspace_bytes < dl3_grad_sumsq_workspace_bytes(n)) {
    dl3_set_error("grad_sumsq: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0,
                  dl3_grad_sumsq_workspace_bytes(n));
    return DL3_EWORKSPACE;
  }
  const int P = sumsq_blocks(n);
  double *partial = (double *)workspace;
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(sumsq_partial_kernel<true>, dim3(P), dim3(256), 0, (hipStream_t)stream, g, n, partial);
  else
    hipLaunchKernelGGL(sumsq_partial_kernel<false>, dim3(P), dim3(256), 0, (hipStream_t)stream, g, n, partial);
  DL3_LAUNCH_CHECK("grad_sumsq");
  hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, P, out);
  DL3_LAUNCH_CHECK("grad_sumsq fold");
  return DL3_OK;
}

// ------------------------------------------------------------------------------------------------------ the update
// what every lane needs of Optimizer.get_gradients, worked out once per lane from two device scalars
struct GradXform {
  float sc;     // grad_scale, or grad_scale / max(denom[0], 1e-20) (adam_norm_kernel's semantics)
  float ratio;  // clipnorm / norm where the global norm reaches clipnorm
  bool clip;
  bool clamp;
  float cv;     // clipvalue
};

__device__ __forceinline__ GradXform grad_xform(const dl3_opt_hyper &h, const float *denom, const double *sumsq) {
  GradXform x;
  x.sc = denom ? h.grad_scale / fmaxf(denom[0], 1e-20f) : h.grad_scale;
  x.clip = false;
  x.ratio = 1.f;
  if (h.clipnorm > 0.f) {
    const float norm = x.sc * (float)sqrt(sumsq[0]);
    if (norm >= h.clipnorm) {
      x.clip = true;
      x.ratio = h.clipnorm / norm;
    }
  }
  x.clamp = h.clipvalue > 0.f;
  x.cv = h.clipvalue;
  return x;
}

__device__ __forceinline__ float eff_grad(float g, const GradXform &x) {
  float gi = g * x.sc;
  if (x.clip) gi = gi * x.ratio;
  if (x.clamp) gi = fminf(fmaxf(gi, -x.cv), x.cv);
  return gi;
}

template <int RULE>
__device__ __forceinline__ void update1(float &p, float gi, float &s0, float &s1, const dl3_opt_hyper &h) {
  if (RULE == DL3_OPT_SGD) {  // c0 = momentum
    const float v = h.c0 * s0 - h.lr_t * gi;
    s0 = v;
    p = h.nesterov ? p + h.c0 * v - h.lr_t * gi : p + v;
  } else if (RULE == DL3_OPT_RMSPROP) {  // c0 = rho
    const float a = h.c0 * s0 + (1.f - h.c0) * (gi * gi);
    s0 = a;
    p -= h.lr_t * gi / (sqrtf(a) + h.eps);
  } else {  // adam_kernel's arithmetic; c0 = beta_1, c1 = beta_2
    const float mi = h.c0 * s0 + (1.f - h.c0) * gi;
    const float vi = h.c1 * s1 + (1.f - h.c1) * gi * gi;
    s0 = mi;
    s1 = vi;
    p -= h.lr_t * mi / (sqrtf(vi) + h.eps);
  }
}

template <int RULE, bool VEC>
__global__ __launch_bounds__(256) void opt_step_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                       float *__restrict__ s0, float *__restrict__ s1, size_t n,
                                                       dl3_opt_hyper h, const float *__restrict__ denom,
                                                       const double *__restrict__ sumsq) {
  const GradXform x = grad_xform(h, denom, sumsq);
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  constexpr bool TWO = RULE == DL3_OPT_ADAM;
  if (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += stride) {
      f32x4 pv = ld4(p + 4 * i), a = ld4(s0 + 4 * i), b = splat4(0.f);
      const f32x4 gv = ld4(g + 4 * i);
      if (TWO) b = ld4(s1 + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        float pk = pv[k], ak = a[k], bk = b[k];
        update1<RULE>(pk, eff_grad(gv[k], x), ak, bk, h);
        pv[k] = pk;
        a[k] = ak;
        b[k] = bk;
      }
      st4(s0 + 4 * i, a);
      if (TWO) st4(s1 + 4 * i, b);
      st4(p + 4 * i, pv);
    }
    const size_t i = 4 * n4 + tid;  // scalar tail: at most 3 elements
    if (i < n) {
      float b = TWO ? s1[i] : 0.f;
      update1<RULE>(p[i], eff_grad(g[i], x), s0[i], b, h);
      if (TWO) s1[i] = b;
    }
  } else {
    for (size_t i = tid; i < n; i += stride) {
      float b = TWO ? s1[i] : 0.f;
      update1<RULE>(p[i], eff_grad(g[i], x), s0[i], b, h);
      if (TWO) s1[i] = b;
    }
  }
}

template <int RULE>
static void launch_opt_step(float *p, const float *g, float *s0, float *s1, size_t n, const dl3_opt_hyper &h,
                            const float *denom, const double *sumsq, hipStream_t stream) {
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0;
  if (vec) {
    size_t b = (n / 4 + 255) / 256;
    b = b > 4096 ? 4096 : (b < 1 ? 1 : b);
    hipLaunchKernelGGL((opt_step_kernel<RULE, true>), dim3((unsigned)b), dim3(256), 0, stream, p, g, s0, s1, n, h, denom,
                       sumsq);
  } else {
    size_t b = (n + 255) / 256;
    b = b > 4096 ? 4096 : b;
    hipLaunchKernelGGL((opt_step_kernel<RULE, false>), dim3((unsigned)b), dim3(256), 0, stream, p, g, s0, s1, n, h,
                       denom, sumsq);
  }
}

extern "C" int dl3_opt_step(float *p, const float *g, float *s0, float *s1, size_t n, int rule, const dl3_opt_hyper *hyper,
                            const float *denom, const double *sumsq, void *stream) {
  DL3_CHECK_ARG(p && g && s0 && hyper && n > 0, "opt_step: bad argument");
  DL3_CHECK_ARG(rule == DL3_OPT_SGD || rule == DL3_OPT_RMSPROP || rule == DL3_OPT_ADAM, "opt_step: unknown rule %d", rule);
  DL3_CHECK_ARG(rule != DL3_OPT_ADAM || s1, "opt_step: Adam needs both slot arrays");
  DL3_CHECK_ARG(!(hyper->clipnorm > 0.f) || sumsq, "opt_step: clipnorm needs the result of dl3_grad_sumsq");
  DL3_CHECK_ARG(hyper->clipnorm >= 0.f && hyper->clipvalue >= 0.f, "opt_step: clipnorm / clipvalue must be >= 0 (0: off)");
  const dl3_opt_hyper h = *hyper;
  if (rule == DL3_OPT_SGD)
    launch_opt_step<DL3_OPT_SGD>(p, g, s0, nullptr, n, h, denom, sumsq, (hipStream_t)stream);
  else if (rule == DL3_OPT_RMSPROP)
    launch_opt_step<DL3_OPT_RMSPROP>(p, g, s0, nullptr, n, h, denom, sumsq, (hipStream_t)stream);
  else
    launch_opt_step<DL3_OPT_ADAM>(p, g, s0, s1, n, h, denom, sumsq, (hipStream_t)stream);
  DL3_LAUNCH_CHECK("opt_step");
  return DL3_OK;
}
