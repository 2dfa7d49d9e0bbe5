// common.h — shared host/device helpers for libdl3 (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/dl3.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void dl3_set_error(const char *fmt, ...);

#define DL3_CHECK_ARG(cond, ...)      \
  do {                                \
    if (!(cond)) {                    \
      dl3_set_error(__VA_ARGS__);     \
      return DL3_EINVAL;              \
    }                                 \
  } while (0)

#define DL3_UNSUPPORTED(cond, ...)    \
  do {                                \
    if (cond) {                       \
      dl3_set_error(__VA_ARGS__);     \
      return DL3_EUNSUPPORTED;        \
    }                                 \
  } while (0)

#define DL3_LAUNCH_CHECK(name)                                              \
  do {                                                                      \
    hipError_t e__ = hipGetLastError();                                     \
    if (e__ != hipSuccess) {                                                \
      dl3_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return DL3_EHIP;                                                      \
    }                                                                       \
  } while (0)

static inline int dl3_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// workgroups of a grid-stride launch: one per per_block items, at least one, at most cap
static inline int dl3_blocks(long n, int per_block, long cap) {
  long b = (n + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}
// M(MAXC) for the smallest register row that holds C <= 32 classes
#define DL3_DISPATCH_MAXC(C, M) \
  do {                          \
    if ((C) <= 8) { M(8); }     \
    else if ((C) <= 24) { M(24); } \
    else { M(32); }             \
  } while (0)

// ---------------------------------------------------------------- device helpers
// Branch-free activation: act is wave-uniform, so the clamp bounds are scalar selects and the activation is
// one v_max + one v_min — no control flow that would make hipcc serialise neighbouring loads behind s_waitcnt.
//   DL3_ACT_NONE: [-inf, +inf]   DL3_ACT_RELU: [0, +inf] (deeplabv3p.py:72)   DL3_ACT_RELU6: [0, 6] (deeplabv3p.py:181)
__device__ __forceinline__ float dl3_act(float v, int act) {
  const float lo = (act != DL3_ACT_NONE) ? 0.f : -__builtin_inff();
  const float hi = (act == DL3_ACT_RELU6) ? 6.f : __builtin_inff();
#ifdef DL3_ACT_MINMAX
  return fminf(fmaxf(v, lo), hi);
#else
  return __builtin_amdgcn_fmed3f(v, lo, hi);  // v_med3_f32: the clamp in ONE VALU instruction (lo <= hi always)
#endif
}
// derivative mask of the activation at pre-activation z: 1 inside the open interval (lo, hi)
__device__ __forceinline__ float dl3_act_mask(float z, int act) {
  const float lo = (act != DL3_ACT_NONE) ? 0.f : -__builtin_inff();
  const float hi = (act == DL3_ACT_RELU6) ? 6.f : __builtin_inff();
  return (z > lo && z < hi) ? 1.f : 0.f;
}
__device__ __forceinline__ f32x4 dl3_act4(f32x4 v, int act) {
  f32x4 r;
  r.x = dl3_act(v.x, act);
  r.y = dl3_act(v.y, act);
  r.z = dl3_act(v.z, act);
  r.w = dl3_act(v.w, act);
  return r;
}
__device__ __forceinline__ f32x4 dl3_mask4(f32x4 z, int act) {
  f32x4 r;
  r.x = dl3_act_mask(z.x, act);
  r.y = dl3_act_mask(z.y, act);
  r.z = dl3_act_mask(z.z, act);
  r.w = dl3_act_mask(z.w, act);
  return r;
}
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }
// streaming store (global_store_dwordx4 ... nt): activations written once and next read by a LATER kernel should not
// evict the lines the current kernel still re-reads from L2
__device__ __forceinline__ void st4_nt(float *p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(p)); }
__device__ __forceinline__ f32x4 splat4(float v) {
  f32x4 r = {v, v, v, v};
  return r;
}

// counter-based keep-mask for Dropout: splitmix64 hash of (seed, element index) -> uniform [0,1)
__device__ __forceinline__ float dl3_uniform(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// Dropout draws a fresh mask every training step: the launch arguments are frozen inside a captured hipGraph, so the
// step number lives in device memory (dl3_counter_add bumps it inside the graph) and is mixed into the seed here.
__device__ __forceinline__ unsigned long long dl3_step_seed(unsigned long long seed, const unsigned long long *step) {
  return step ? seed + step[0] * 0xD1B54A32D192ED03ull : seed;
}

// 64-lane butterfly: every lane ends with the same sum
// (float, double, int, unsigned int: the types __shfl_xor moves)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the 256 lanes of a workgroup in a FIXED order (butterfly inside each wave, waves 0..3 added in index order);
// valid in lane 0
__device__ __forceinline__ double block_sum256(double v, double *sh) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// the second pass of such a sum, ONE workgroup: lane t adds the partials t*c .. t*c + c - 1 in index order, then the fixed
// fold over the lanes; valid in lane 0 (P == 0: 0)
__device__ __forceinline__ double fold_partials256(const double *__restrict__ partial, int P, double *sh) {
  const int c = (P + 255) / 256;
  double acc = 0.0;
  for (int k = 0; k < c; k++) {
    const int i = (int)threadIdx.x * c + k;
    if (i < P) acc += partial[i];
  }
  return block_sum256(acc, sh);
}
