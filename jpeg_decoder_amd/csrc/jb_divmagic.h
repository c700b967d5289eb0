// jb_divmagic.h -- division of a tile index by a launch constant as one 32 x 32 -> 64-bit multiply and one shift.
// The host computes the pair once per launch (jb_div_make); the kernels apply it (jb_div_apply) where they used to
// divide: a 32-bit integer division on the GPU is a float reciprocal, a trip through a VGPR and some 25 dependent
// scalar instructions, in front of every tile's first load.
//
// Exact for every numerator n < 2^31 and every divisor 1 <= d < 2^31.  With l = ceil(log2 d), shift = 31 + l and
// mul = ceil(2^shift / d):  mul * d = 2^shift + e with 0 <= e < d <= 2^l, so
//   n * mul / 2^shift = n / d + n * e / (d * 2^shift)  and  n * e / (d * 2^shift) < 2^31 * 2^l / (d * 2^shift) = 1 / d,
// which cannot carry n / d (whose fraction is at most (d - 1) / d) over the next integer.  mul fits 32 bits: for l >= 1,
// d >= 2^(l-1) + 1 and l <= 31 give 2^shift / d <= 2^32 * (1 - 1 / (2^30 + 1)) < 2^32 - 3, and d = 1 gives mul = 2^31;
// the product is below 2^63.  Plain C++: host code, kernels and the stand-alone check (tools/div_check.cpp) share it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JB_DIV_FN __host__ __device__ static inline
#else
#define JB_DIV_FN static inline
#endif

struct JbDiv {
  uint32_t mul;    // ceil(2^shift / d)
  uint32_t shift;  // 31 + ceil(log2 d): 31..62
};

// d < 1 (a launch that never divides by the field) gives the pair of d = 1
JB_DIV_FN JbDiv jb_div_make(int32_t d) {
  const uint64_t dd = d < 1 ? 1u : (uint64_t)d;
  uint32_t l = 0;
  while ((1ull << l) < dd) l++;
  JbDiv r;
  r.shift = 31 + l;
  r.mul = (uint32_t)(((1ull << r.shift) + dd - 1) / dd);
  return r;
}

// floor(n / d) for 0 <= n < 2^31
JB_DIV_FN uint32_t jb_div_apply(uint32_t n, JbDiv k) { return (uint32_t)(((uint64_t)n * k.mul) >> k.shift); }
