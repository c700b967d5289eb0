// jb_fit.hip -- "fit" (include/jpegblk.h), JB_FIT_PAD: the border of a letterboxed target.  The resample and filter kernels
// of jb_resample.hip write the inner rectangle (they are launched with the inner size and a moved dst); this kernel
// writes what is left of every image of the call: at most two BANDS -- left and right, or top and bottom -- each a
// rectangle of the target, in one launch.  The bands and the inner rectangle are disjoint, so the order on the stream
// is free.
//
// The work is indexed over the bands alone: a band of w x h elements is walked linearly, row by row, and a workgroup owns
// 256 consecutive elements of it, so the cost follows the bytes written whatever the band's shape -- a band one column wide
// costs h stores, not h waves.  One lane = one pixel of the target = three stores, addressed element-wise through the
// strides exactly as jb_resample_kernel's store stage addresses them, in the same four formats; nothing outside a band is
// written: the gaps between rows, planes and images stay untouched.  No loads: the three fill values come from the kernel's
// arguments and are wave-uniform, converted as the store stage converts a uint8 -- the byte itself, or
// (float)fill[c] * scale[c] + bias[c] as two rounded operations (-ffp-contract=off) and for f16 one v_cvt_f16_f32.
// The body also compiles for the CPU (JB_KERNELS_HOST: tools/fuzz/fit_kernel_check.cpp).
#ifndef JB_KERNELS_HOST
#include <hip/hip_runtime.h>

#include "jb_launch.h"
#endif

#include "jb_kernels.h"
#include "jb_store.h"

static constexpr int kFitFillLanes = 256;  // elements of a band per workgroup

template <int FORMAT>
__global__ __launch_bounds__(kFitFillLanes) void jb_fit_fill_kernel(const JbFitFill p) {
  const uint32_t per_image = (uint32_t)p.wgs[0] + (uint32_t)p.wgs[1];
  const uint32_t b = blockIdx.x;
  const uint32_t img = b / per_image;
  uint32_t t = b - img * per_image;
  // (the band is the workgroup's: everything derived from it is wave-uniform)
  const bool second = t >= (uint32_t)p.wgs[0];
  if (second) t -= (uint32_t)p.wgs[0];
  const uint32_t bx = (uint32_t)(second ? p.bx[1] : p.bx[0]), by = (uint32_t)(second ? p.by[1] : p.by[0]);
  const uint32_t bw = (uint32_t)(second ? p.bw[1] : p.bw[0]), bh = (uint32_t)(second ? p.bh[1] : p.bh[0]);
  // the element of the band: below 65535^2 < 2^32
  const uint32_t n = t * (uint32_t)kFitFillLanes + threadIdx.x;
  if (img >= (uint32_t)p.n_images || n >= bw * bh) return;
  const uint32_t row = n / bw;
  const uint32_t x = bx + (n - row * bw), y = by + row;
  uint8_t *const dst = p.dst + (int64_t)img * p.dst_image_stride + (int64_t)y * p.dst_row_stride;
#pragma unroll
  for (int c = 0; c < 3; c++) jb_store_element<FORMAT>(dst, p.dst_plane_stride, x, c, p.fill[c], p.scale, p.bias);
}

// the grid of a launch (wgs into p); false: an argument outside its range, or more than 2^31 - 1 workgroups.  *n_wgs = 0:
// there is no border, and nothing to launch.
static bool fit_fill_grid(JbFitFill &p, int format, int64_t *n_wgs) {
  if (format < 0 || format > 3 || p.ow < 1 || p.oh < 1 || p.ow > 65535 || p.oh > 65535 || p.n_images < 1) return false;
  int64_t per_image = 0;
  for (int i = 0; i < 2; i++) {
    p.wgs[i] = 0;
    if (p.bw[i] == 0 || p.bh[i] == 0) continue;  // no such band
    if (p.bx[i] < 0 || p.by[i] < 0 || p.bw[i] < 0 || p.bh[i] < 0 || (int64_t)p.bx[i] + p.bw[i] > p.ow || (int64_t)p.by[i] + p.bh[i] > p.oh) return false;
    p.wgs[i] = (int32_t)(((int64_t)p.bw[i] * p.bh[i] + kFitFillLanes - 1) / kFitFillLanes);  // at most 2^24
    per_image += p.wgs[i];
  }
  if (per_image * p.n_images > 0x7fffffffLL) return false;
  *n_wgs = per_image * p.n_images;
  return true;
}

#ifndef JB_KERNELS_HOST
hipError_t jbk_fit_fill_launch(const JbFitFill &q, int format, hipStream_t stream) {
  JbFitFill p = q;
  int64_t n_wgs = 0;
  if (!fit_fill_grid(p, format, &n_wgs)) return hipErrorInvalidValue;
  if (n_wgs == 0) return hipSuccess;
  const dim3 grid((unsigned)n_wgs), block(kFitFillLanes);
  jb_by_format(format, [&](auto F) { hipLaunchKernelGGL(jb_fit_fill_kernel<decltype(F)::value>, grid, block, 0, stream, p); });
  return hipGetLastError();
}
#endif  // JB_KERNELS_HOST
