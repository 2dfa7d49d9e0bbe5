// pwdev.h — the device helpers more than one kernel file of the 1x1-convolution GEMMs uses (pwstream.hip, pwwgrad.hip):
// the split-math operand split.  Everything else the families share is common.h.
#pragma once
#include "common.h"
namespace {
// ---- split math (DL3_GEMM_MATH=split): fp32 GEMM on the bf16 matrix pipe ----------------------------------
// v_mfma_f32_32x32x2_f32 runs at the f32 VECTOR rate, 1/16 of v_mfma_f32_32x32x16_bf16.  An fp32 number is EXACTLY the
// sum of three bf16 numbers (its 24-bit significand cut into 8 + 8 + 8 bits by truncation: h = top 16 bits of x,
// m = top 16 bits of x - h, l = x - h - m, every subtraction exact), a bf16 x bf16 product is exact in fp32, and the MFMA
// accumulates in fp32.  a.b = sum over the nine piece products; the six of order >= 2^-16 are computed, the three
// dropped ones (m.l, l.m, l.l) are <= 2^-23 |a||b| — the size of ONE fp32 rounding, which the f32 MFMA commits per
// product anyway.  Six bf16 MFMAs of K=16 (6 x 32 cycles) replace eight f32 MFMAs of K=2 (8 x 64): 2.67x the matrix rate
// at fp32-roundoff-class accuracy (tests/test_gpu_ops.py::test_split_math_error measures both against float64).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 8 consecutive-k fp32 values of one lane -> the three bf16x8 MFMA operands
__device__ __forceinline__ void split3(const f32x4 &v0, const f32x4 &v1, u32x4 &h, u32x4 &m, u32x4 &l) {
  unsigned hb[8], mb[8], lb[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const float x = e < 4 ? v0[e] : v1[e - 4];
    const unsigned xh = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(xh);
    const unsigned xm = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(xm);
    hb[e] = xh; mb[e] = xm; lb[e] = __float_as_uint(r2);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {  // word q = [element 2q+1 : element 2q], upper halves of both
    h[q] = __builtin_amdgcn_perm(hb[2 * q + 1], hb[2 * q], 0x07060302u);
    m[q] = __builtin_amdgcn_perm(mb[2 * q + 1], mb[2 * q], 0x07060302u);
    l[q] = __builtin_amdgcn_perm(lb[2 * q + 1], lb[2 * q], 0x07060302u);
  }
}
}  // namespace
