// jb_store.h -- the element store of the kernels behind the pixel kernel (jb_resample_kernel, jb_filter_kernel,
// jb_orient_kernel, jb_fit_fill_kernel): channel c of the pixel in column x of an output row, in one of the four output
// formats (JB_FMT_*).  Device code that also compiles for the CPU (JB_KERNELS_HOST / JB_ORIENT_HOST: tools/fuzz stubs
// __device__, __forceinline__ and _Float16 in front of it).
#pragma once
#include <stdint.h>

// row: the output row's first byte (of plane 0 when planar); plane_stride: bytes between the planes; u: the value, 0..255.
// The float formats are the planar store stage's expression (jb_kernels.hip), operation for operation: u8 -> f32 (exact),
// one f32 multiply, one f32 add -- separate instructions: the library is built with -ffp-contract=off, and the CPU
// reference rounds twice -- and for f16 one v_cvt_f16_f32 (round to nearest even).
template <int FORMAT>
static __device__ __forceinline__ void jb_store_element(uint8_t *row, int64_t plane_stride, int64_t x, int c, uint32_t u, const float *scale,
                                                        const float *bias) {
  if constexpr (FORMAT == 0) {
    row[3 * x + c] = (uint8_t)u;
  } else if constexpr (FORMAT == 1) {
    row[(int64_t)c * plane_stride + x] = (uint8_t)u;
  } else {
    const float f = (float)u * scale[c] + bias[c];
    uint8_t *const at = row + (int64_t)c * plane_stride;
    if constexpr (FORMAT == 2) ((float *)at)[x] = f;
    else ((_Float16 *)at)[x] = (_Float16)f;
  }
}
