// jb_color.hip -- "colour chains" (include/jpegblk.h): per-view brightness / contrast / saturation / hue / grayscale /
// solarize on interleaved uint8 views, written in any of the four output formats.  The arithmetic is jb_color_core.h's,
// the text the host statement (jb_color_host) compiles too.  Two kernels:
//
// jb_color_mean_kernel -- only for launches with a JB_COLOR_CONTRAST: grid (slices of kMeanRows rows, views).  A lane
//   applies the ops IN FRONT of the chain's contrast to its pixels and sums their luma in a 32-bit integer (at most
//   4 rows x 256 steps x 4 pixels x 255), the wave reduces with __shfl_xor, the four waves meet in LDS, and one 64-bit
//   integer atomicAdd per workgroup lands in sums[view].  Integer sums: the result does not depend on the order.
// jb_color_apply_kernel -- grid (tiles of 256 columns x 4 rows, views).  A wave is 64 adjacent 4-pixel groups of ONE row
//   of ONE view: the chain (read from the arguments by blockIdx.y: scalar loads) and every branch on an op are
//   wave-uniform.  A lane's 4 pixels are three 4-byte loads at any byte address (gfx950 under ROCm runs with unaligned
//   global access enabled) -- a ragged last group of a row falls back to bytes, nothing beyond the row is touched -- and
//   its stores are 12 bytes interleaved, 4 bytes per plane for planar uint8, 8 for f16, 16 for f32.  The store expression
//   of the float formats is jb_store.h's, operation for operation.
#include <hip/hip_runtime.h>

#include "jb_color_core.h"
#include "jb_kernels.h"
#include "jb_launch.h"

static constexpr int kColorRows = 4;  // rows (= waves) per workgroup of the apply kernel
static constexpr int kMeanRows = 16;  // rows per workgroup of the mean kernel

typedef uint32_t jb_u32_a1 __attribute__((aligned(1)));
typedef uint32_t jb_u32_a2 __attribute__((aligned(2)));

// n (1..4) pixels of a row from byte address `at` into px[4][3]
static __device__ __forceinline__ void color_load(const uint8_t *at, int n, int px[4][3]) {
  if (n == 4) {
    const uint32_t a = *(const jb_u32_a1 *)at, b = *(const jb_u32_a1 *)(at + 4), c = *(const jb_u32_a1 *)(at + 8);
    px[0][0] = a & 0xff, px[0][1] = (a >> 8) & 0xff, px[0][2] = (a >> 16) & 0xff;
    px[1][0] = a >> 24, px[1][1] = b & 0xff, px[1][2] = (b >> 8) & 0xff;
    px[2][0] = (b >> 16) & 0xff, px[2][1] = b >> 24, px[2][2] = c & 0xff;
    px[3][0] = (c >> 8) & 0xff, px[3][1] = (c >> 16) & 0xff, px[3][2] = c >> 24;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int ch = 0; ch < 3; ch++) px[i][ch] = i < n ? at[3 * i + ch] : 0;
  }
}

__global__ __launch_bounds__(256) void jb_color_mean_kernel(const JbColor p, const JbColorTable table) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const int at = jbc_contrast_at(row.chain);
  if (at < 0) return;  // (the whole workgroup: the chain is the view's)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int y0 = (int)blockIdx.x * kMeanRows;
  const int y1 = min(y0 + kMeanRows, p.h);
  const uint8_t *const src = p.src + row.src_offset;
  uint32_t sum = 0;
  for (int y = y0 + wave; y < y1; y += 4) {
    const uint8_t *const line = src + (int64_t)y * p.src_row_stride;
    for (int x = 4 * lane; x < p.w; x += 256) {
      const int n = min(4, p.w - x);
      int px[4][3];
      color_load(line + 3 * (int64_t)x, n, px);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (i < n) {
          jbc_apply_ops(row.chain, 0, at, 0, &px[i][0], &px[i][1], &px[i][2]);
          sum += (uint32_t)jbc_luma(px[i][0], px[i][1], px[i][2]);
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
  __shared__ uint32_t part[4];
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&p.sums[view], (unsigned long long)part[0] + part[1] + part[2] + part[3]);
}

template <int FORMAT>
__global__ __launch_bounds__(64 * kColorRows) void jb_color_apply_kernel(const JbColor p, const JbColorTable table) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t tx = blockIdx.x % (uint32_t)p.tiles_x, ty = blockIdx.x / (uint32_t)p.tiles_x;
  const int y = (int)ty * kColorRows + wave;   // wave-uniform
  const int x = ((int)tx * 64 + lane) * 4;
  if (y >= p.h || x >= p.w) return;
  const int n = min(4, p.w - x);
  int mean = 0;
  if (jbc_contrast_at(row.chain) >= 0) mean = jbc_contrast_mean(p.sums[view], (uint64_t)p.w * (uint64_t)p.h);
  int px[4][3];
  color_load(p.src + row.src_offset + (int64_t)y * p.src_row_stride + 3 * (int64_t)x, n, px);
  const int n_ops = row.chain.n_ops;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i < n) jbc_apply_ops(row.chain, 0, n_ops, mean, &px[i][0], &px[i][1], &px[i][2]);

  uint8_t *const dst = p.dst + row.dst_offset + (int64_t)y * p.dst_row_stride;
  if constexpr (FORMAT == 0) {
    uint8_t *const at = dst + 3 * (int64_t)x;
    if (n == 4) {
      *(jb_u32_a1 *)at = (uint32_t)px[0][0] | (uint32_t)px[0][1] << 8 | (uint32_t)px[0][2] << 16 | (uint32_t)px[1][0] << 24;
      *(jb_u32_a1 *)(at + 4) = (uint32_t)px[1][1] | (uint32_t)px[1][2] << 8 | (uint32_t)px[2][0] << 16 | (uint32_t)px[2][1] << 24;
      *(jb_u32_a1 *)(at + 8) = (uint32_t)px[2][2] | (uint32_t)px[3][0] << 8 | (uint32_t)px[3][1] << 16 | (uint32_t)px[3][2] << 24;
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (i < n) at[3 * i] = (uint8_t)px[i][0], at[3 * i + 1] = (uint8_t)px[i][1], at[3 * i + 2] = (uint8_t)px[i][2];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      uint8_t *const plane = dst + (int64_t)c * p.dst_plane_stride;
      if constexpr (FORMAT == 1) {
        uint8_t *const at = plane + x;
        if (n == 4) {
          *(jb_u32_a1 *)at = (uint32_t)px[0][c] | (uint32_t)px[1][c] << 8 | (uint32_t)px[2][c] << 16 | (uint32_t)px[3][c] << 24;
        } else {
#pragma unroll
          for (int i = 0; i < 3; i++)
            if (i < n) at[i] = (uint8_t)px[i][c];
        }
      } else {
        // the planar store stage's expression, operation for operation: u8 -> f32 (exact), one f32 multiply, one f32 add
        // (separate instructions: built with -ffp-contract=off), for f16 one conversion (round to nearest even)
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float m = (float)px[i][c] * p.scale[c];
          f[i] = m + p.bias[c];
        }
        if constexpr (FORMAT == 2) {
          float *const at = (float *)plane + x;
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (i < n) at[i] = f[i];
        } else {
          _Float16 *const at = (_Float16 *)plane + x;
          if (n == 4) {
            const _Float16 hlf[4] = {(_Float16)f[0], (_Float16)f[1], (_Float16)f[2], (_Float16)f[3]};
            uint32_t w0, w1;
            __builtin_memcpy(&w0, &hlf[0], 4);
            __builtin_memcpy(&w1, &hlf[2], 4);
            *(jb_u32_a2 *)at = w0;
            *((jb_u32_a2 *)at + 1) = w1;
          } else {
#pragma unroll
            for (int i = 0; i < 3; i++)
              if (i < n) at[i] = (_Float16)f[i];
          }
        }
      }
    }
  }
}

hipError_t jbk_color_launch(const JbColor &q, const JbColorTable &table, int format, hipStream_t stream) {
  if (format < 0 || format > 3 || q.w < 1 || q.h < 1 || q.w > 65535 || q.h > 65535 || q.n_views < 1 || q.n_views > kJbCropsPerLaunch || !q.src ||
      !q.dst || !q.sums || q.src_row_stride < 3LL * q.w)
    return hipErrorInvalidValue;
  bool contrast = false;
  for (int i = 0; i < q.n_views; i++) {
    const JbColorRow &r = table.r[i];
    if (r.src_offset < 0 || r.dst_offset < 0 || r.chain.n_ops < 0 || r.chain.n_ops > JB_COLOR_OPS_MAX) return hipErrorInvalidValue;
    if (jbc_contrast_at(r.chain) >= 0) contrast = true;
  }
  JbColor p = q;
  p.tiles_x = (p.w + 255) / 256;
  const int tiles_y = (p.h + kColorRows - 1) / kColorRows;  // (at most 256 x 16,384 workgroups a view)
  if (contrast) {
    hipError_t e = hipMemsetAsync(p.sums, 0, sizeof(unsigned long long) * kJbCropsPerLaunch, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jb_color_mean_kernel, dim3((unsigned)((p.h + kMeanRows - 1) / kMeanRows), (unsigned)p.n_views), dim3(256), 0, stream, p, table);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)(p.tiles_x * tiles_y), (unsigned)p.n_views), block(64 * kColorRows);
  jb_by_format(format, [&](auto F) { hipLaunchKernelGGL(jb_color_apply_kernel<decltype(F)::value>, grid, block, 0, stream, p, table); });
  return hipGetLastError();
}
