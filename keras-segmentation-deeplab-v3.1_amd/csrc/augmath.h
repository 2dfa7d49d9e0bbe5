// augmath.h — integer arithmetic the augmentation chain (augment.hip) and the resize front end (cvresize.hip) share:
// cv2.GaussianBlur(5, sigma 0) as two [1 4 6 4 1] passes, and the 256-bit label set kept in registers.
#pragma once

// horizontal pass over interleaved BGR bytes: t points at the tap two pixels to the left
__device__ __forceinline__ int blur5_row(const unsigned char *t) { return t[0] + 4 * t[3] + 6 * t[6] + 4 * t[9] + t[12]; }

// vertical pass over the horizontal sums, `stride` ints per row; (sum + 128) >> 8
__device__ __forceinline__ int blur5_col(const int *h, int stride) {
  return (h[0] + 4 * h[stride] + 6 * h[2 * stride] + 4 * h[3 * stride] + h[4 * stride] + 128) >> 8;
}

// m |= {v}: the word is chosen by selects, not by a runtime index, so the set stays in registers
__device__ __forceinline__ void present_add(unsigned (&m)[8], unsigned v) {
  const unsigned bit = 1u << (v & 31), w = v >> 5;
#pragma unroll
  for (int k = 0; k < 8; k++) m[k] |= (w == (unsigned)k) ? bit : 0u;
}
