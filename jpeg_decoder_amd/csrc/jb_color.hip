// jb_color.hip -- "colour chains" (include/jpegblk.h): per-view brightness / contrast / saturation / hue / grayscale /
// solarize on interleaved uint8 views, written in any of the four output formats.  The arithmetic is jb_color_core.h's,
// the text the host statement (jb_color_host) compiles too.  Three kernels (the third, jb_color_blur_kernel for the views
// whose chain has a JB_COLOR_BLUR, is described where it stands):
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
// jb_color_hist_kernel, jb_color_table_kernel -- only for launches with a JB_COLOR_AUTOCONTRAST / _EQUALIZE: three 256-bin
//   histograms of a view in integers, and the 3 x 256 table bytes from them; ROUNDS of statistics are described in
//   jb_kernels.h and where the two kernels stand.
// jb_color_sharp_kernel -- only for the views whose chain has a JB_COLOR_SHARPNESS: a 64 x 32 tile with a halo of 1.
// Geometric operations (JB_COLOR_SHEAR_X .. JB_COLOR_ROTATE): a launch with one runs the WARP instantiations of the kernels
// above, whose every pixel load is jbc_gather (jb_color_core.h), behind jb_color_warp_table_kernel, which puts the operations'
// integers into the scratch (jb_kernels.h); a launch without one runs the kernels with that text compiled out.
#include <hip/hip_runtime.h>

#include "jb_color_core.h"
#include "jb_kernels.h"
#include "jb_launch.h"

// the weights of the launch's blurs, beside JbColorTable in the arguments of jb_color_blur_kernel
struct JbBlurTable {
  JbBlurWeights k[kJbCropsPerLaunch];
};
static_assert(sizeof(JbColor) + sizeof(JbColorTable) + sizeof(JbBlurTable) <= 4096, "the colour kernels' arguments must fit the 4 KB segment");

// the coefficients of the launch's geometric operations: the arguments of jb_color_warp_table_kernel alone, which copies them
// into the scratch (jb_kernels.h says why they do not travel with the other kernels' arguments)
struct JbWarpTable {
  JbWarp k[kJbCropsPerLaunch][JB_COLOR_WARPS_MAX];
};
static_assert(sizeof(JbWarp) == 32 && sizeof(JbWarpTable) == kJbColorWarpBytes, "the warp table is the scratch's");
static_assert(sizeof(JbColor) + sizeof(JbWarpTable) <= 4096, "the warp table kernel's arguments must fit the 4 KB segment");
static_assert(kJbColorWarpOffset % 16 == 0, "the warp table in the scratch is aligned");

static constexpr int kColorRows = 4;  // rows (= waves) per workgroup of the apply kernel
static constexpr int kMeanRows = 16;  // rows per workgroup of the mean kernel
static constexpr int kHistRows = 32;  // rows per workgroup of the histogram kernel

// the scratch behind p.sums (jb_kernels.h): the 768 counters and the 768 table bytes of statistics operation k of a view
static __device__ __forceinline__ uint32_t *color_counters(const JbColor &p, uint32_t view, int k) {
  return (uint32_t *)(p.sums + kJbCropsPerLaunch) + (view * JB_COLOR_STATS_MAX + (uint32_t)k) * 768u;
}
static __device__ __forceinline__ uint8_t *color_table(const JbColor &p, uint32_t view, int k) {
  return (uint8_t *)(p.sums + kJbCropsPerLaunch) + kJbCropsPerLaunch * JB_COLOR_STATS_MAX * kJbColorCounterBytes + (view * JB_COLOR_STATS_MAX + (uint32_t)k) * 768u;
}
// what a view's operations read beside the pixel.  The mean is read only where the chain has a contrast; a kernel of round k
// applies the ops in front of statistics operation k alone, so it never reads an unfinished statistic.
static __device__ __forceinline__ JbcCtx color_ctx(const JbColor &p, const JbcShape &shape, uint32_t view) {
  JbcCtx s;
  s.mean = shape.contrast >= 0 ? jbc_contrast_mean(p.sums[view], (uint64_t)p.w * (uint64_t)p.h) : 0;
  s.at1 = shape.stat1;
  s.lut[0] = color_table(p, view, 0), s.lut[1] = color_table(p, view, 1);
  return s;
}

// the two JbWarp of a view in the scratch (written by jb_color_warp_table_kernel in front of the launch's other kernels)
static __device__ __forceinline__ const JbWarp *color_warps(const JbColor &p, uint32_t view) {
  return (const JbWarp *)((const uint8_t *)p.sums + kJbColorWarpOffset) + view * JB_COLOR_WARPS_MAX;
}
// grid (1), 256 threads: the table's 512 words into the scratch, two a thread
__global__ __launch_bounds__(256) void jb_color_warp_table_kernel(const JbColor p, const JbWarpTable t) {
  static_assert(sizeof(JbWarpTable) == 2 * 256 * 4, "two words a thread");
  uint32_t *const to = (uint32_t *)((uint8_t *)p.sums + kJbColorWarpOffset);
  const uint32_t *const from = (const uint32_t *)&t;
  to[threadIdx.x] = from[threadIdx.x];
  to[256 + threadIdx.x] = from[256 + threadIdx.x];
}

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

// round: the contrast must be statistics operation `round` of its chain (0 or 1); with round 1 the table of round 0 is applied
// in front of it.  NEW_OPS = false compiles the operations numbered from 10 out, for a launch without any: no such operation stands in front of a chain's
// first statistics operation, and the kernel is then the one it was before there were tables.
// WARP: the launch has a chain with a geometric operation: every pixel is jbc_gather's (the view as it stands in front of the
// contrast, through the geometric operations in front of it); false compiles that out.
template <bool NEW_OPS, bool WARP = false>
__global__ __launch_bounds__(256) void jb_color_mean_kernel(const JbColor p, const JbColorTable table, const int round) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const JbcShape shape = jbc_shape(row.chain);
  const int at = shape.contrast;
  if (at < 0 || jbc_stat_at(shape, round) != at) return;  // (the whole workgroup: the chain is the view's)
  JbcCtx ctx;
  ctx.mean = 0, ctx.at1 = shape.stat1, ctx.lut[0] = color_table(p, view, 0), ctx.lut[1] = nullptr;
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
      if constexpr (WARP) {
        const JbcWarpShape ws = jbc_warp_shape(row.chain);
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i < n) {
            jbc_gather<NEW_OPS>(row.chain, ws, at, ctx, color_warps(p, view), src, p.src_row_stride, p.w, p.h, x + i, y, &px[i][0], &px[i][1], &px[i][2]);
            sum += (uint32_t)jbc_luma(px[i][0], px[i][1], px[i][2]);
          }
        continue;
      }
      color_load(line + 3 * (int64_t)x, n, px);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (i < n) {
          jbc_apply_ops<NEW_OPS>(row.chain, 0, at, ctx, &px[i][0], &px[i][1], &px[i][2]);
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

// jb_color_hist_kernel -- grid (slices of kHistRows rows, views), for the views whose statistics operation `round` is a
// JB_COLOR_AUTOCONTRAST or _EQUALIZE.  The mean kernel's walk: a lane applies the ops in front of that operation (with the
// results of round 0 when round is 1) to its pixels and counts them in the workgroup's three 256-bin histograms in LDS with
// LDS integer atomics (at most 32 x 65535 pixels a workgroup: far inside 32 bits); then the workgroup adds its non-empty bins
// to the view's 768 counters with global integer atomics.  Integer sums: the result does not depend on the order.
template <bool WARP>
__global__ __launch_bounds__(256) void jb_color_hist_kernel(const JbColor p, const JbColorTable table, const int round) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const JbcShape shape = jbc_shape(row.chain);
  const int at = jbc_stat_at(shape, round);
  if (at < 0 || !jbc_is_hist(row.chain.ops[at].op)) return;  // (the whole workgroup)
  const JbcCtx ctx = color_ctx(p, shape, view);
  __shared__ uint32_t hist[768];
  for (int i = (int)threadIdx.x; i < 768; i += 256) hist[i] = 0;
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int y0 = (int)blockIdx.x * kHistRows;
  const int y1 = min(y0 + kHistRows, p.h);
  const uint8_t *const src = p.src + row.src_offset;
  for (int y = y0 + wave; y < y1; y += 4) {
    const uint8_t *const line = src + (int64_t)y * p.src_row_stride;
    for (int x = 4 * lane; x < p.w; x += 256) {
      const int n = min(4, p.w - x);
      int px[4][3];
      if constexpr (WARP) {
        const JbcWarpShape ws = jbc_warp_shape(row.chain);
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i < n) {
            jbc_gather<true>(row.chain, ws, at, ctx, color_warps(p, view), src, p.src_row_stride, p.w, p.h, x + i, y, &px[i][0], &px[i][1], &px[i][2]);
            atomicAdd(&hist[px[i][0]], 1u), atomicAdd(&hist[256 + px[i][1]], 1u), atomicAdd(&hist[512 + px[i][2]], 1u);
          }
        continue;
      }
      color_load(line + 3 * (int64_t)x, n, px);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (i < n) {
          jbc_apply_ops<true>(row.chain, 0, at, ctx, &px[i][0], &px[i][1], &px[i][2]);
          atomicAdd(&hist[px[i][0]], 1u), atomicAdd(&hist[256 + px[i][1]], 1u), atomicAdd(&hist[512 + px[i][2]], 1u);
        }
      }
    }
  }
  __syncthreads();
  uint32_t *const counters = color_counters(p, view, round);
  for (int i = (int)threadIdx.x; i < 768; i += 256)
    if (hist[i]) atomicAdd(&counters[i], hist[i]);
}

// jb_color_table_kernel -- grid (views), 256 threads: thread t makes entry t of the three tables of statistics operation
// `round` from the view's 768 counters.  Per channel: the prefix sum of the counts in front of bin t (a wave scan with
// __shfl_up, the four waves' totals through LDS), the first and last non-empty bins from the waves' ballots; then the entry is
// jb_color_core.h's -- jbc_equalize_entry in integers, jbc_autocontrast_entry in fp64 (built with -ffp-contract=off; the
// fp64 division is correctly rounded).  A kernel of its own, not a prologue of the consumers: 768 entries once a view, where
// every workgroup of the apply, blur or sharpness kernel would repeat the scan.
__global__ __launch_bounds__(256) void jb_color_table_kernel(const JbColor p, const JbColorTable table, const int round) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const JbcShape shape = jbc_shape(row.chain);
  const int at = jbc_stat_at(shape, round);
  if (at < 0 || !jbc_is_hist(row.chain.ops[at].op)) return;  // (the whole workgroup)
  const bool equalize = row.chain.ops[at].op == JB_COLOR_EQUALIZE;
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const uint32_t *const counters = color_counters(p, view, round);
  __shared__ uint32_t counts[768], wave_sum[3][4];
  __shared__ unsigned long long wave_mask[3][4];
  uint32_t before[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const uint32_t n = counters[256 * c + t];
    counts[256 * c + t] = n;
    uint32_t incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += v;
    }
    const unsigned long long mask = __ballot(n != 0);
    if (lane == 63) wave_sum[c][wave] = incl;
    if (lane == 0) wave_mask[c][wave] = mask;
    before[c] = incl - n;
  }
  __syncthreads();
  uint8_t *const lut = color_table(p, view, round);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t total = 0, front = before[c];
    int lo = -1, hi = -1;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const unsigned long long m = wave_mask[c][w];
      if (w < wave) front += wave_sum[c][w];
      total += wave_sum[c][w];
      if (m) {
        if (lo < 0) lo = 64 * w + (__ffsll((long long)m) - 1);
        hi = 64 * w + 63 - __clzll((long long)m);
      }
    }
    if (lo < 0) lo = hi = 0;  // (a view has pixels: not reached)
    int e;
    if (equalize) {
      const uint32_t step = hi > lo ? (total - counts[256 * c + hi]) / 255u : 0u;
      e = jbc_equalize_entry(step, front, t);
    } else {
      e = jbc_autocontrast_entry(lo, hi, t);
    }
    lut[256 * c + t] = (uint8_t)e;
  }
}

// n (1..4) pixels px of a row, behind the chain, to columns x.. of the output row at `dst` (of plane 0 when planar) in FORMAT:
// the ONE store of the colour kernels
template <int FORMAT>
static __device__ __forceinline__ void color_store(const JbColor &p, uint8_t *const dst, const int x, const int n, const int px[4][3]) {
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

// NEW_OPS: the launch has a chain with an operation numbered 10..13; false compiles those out, for the launches of the older kinds
// WARP: the launch has a chain with a geometric operation: a lane's pixels are jbc_gather's, three byte loads each at their own
// positions; false compiles that out
template <int FORMAT, bool NEW_OPS, bool WARP = false>
__global__ __launch_bounds__(64 * kColorRows) void jb_color_apply_kernel(const JbColor p, const JbColorTable table) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const JbcShape shape = jbc_shape(row.chain);
  if (shape.nbhd >= 0) return;  // (the whole workgroup: the view is jb_color_blur_kernel's or jb_color_sharp_kernel's)
  const uint32_t tx = blockIdx.x % (uint32_t)p.tiles_x, ty = blockIdx.x / (uint32_t)p.tiles_x;
  const int y = (int)ty * kColorRows + wave;   // wave-uniform
  const int x = ((int)tx * 64 + lane) * 4;
  if (y >= p.h || x >= p.w) return;
  const int n = min(4, p.w - x);
  const JbcCtx ctx = color_ctx(p, shape, view);
  int px[4][3];
  const int n_ops = row.chain.n_ops;
  if constexpr (WARP) {
    const JbcWarpShape ws = jbc_warp_shape(row.chain);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      px[i][0] = px[i][1] = px[i][2] = 0;
      if (i < n)
        jbc_gather<NEW_OPS>(row.chain, ws, n_ops, ctx, color_warps(p, view), p.src + row.src_offset, p.src_row_stride, p.w, p.h, x + i, y, &px[i][0],
                            &px[i][1], &px[i][2]);
    }
  } else {
    color_load(p.src + row.src_offset + (int64_t)y * p.src_row_stride + 3 * (int64_t)x, n, px);
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < n) jbc_apply_ops<NEW_OPS>(row.chain, 0, n_ops, ctx, &px[i][0], &px[i][1], &px[i][2]);
  }

  color_store<FORMAT>(p, p.dst + row.dst_offset + (int64_t)y * p.dst_row_stride, x, n, px);
}

// The tile of jb_color_blur_kernel<FORMAT, HALO>: kBlurW x kBlurH output pixels and HALO >= 3 (r + 1) samples around them,
// three planes of bytes, twice (a pass reads one buffer and writes the other).  The pitch is an ODD number of 4-byte words:
// in a row pass the lanes of a wave walk along rows one pitch apart, and an odd word pitch spreads 64 of them over the 64
// banks; in a column pass the lanes walk down adjacent columns: adjacent bytes, the same or the next word.
static constexpr int kBlurW = 64, kBlurH = 32;
template <int HALO>
struct BlurTile {
  static constexpr int kW = kBlurW + 2 * HALO, kH = kBlurH + 2 * HALO;
  static constexpr int kPitch = (((kW + 3) / 4) | 1) * 4;
  static constexpr int kPlane = kPitch * kH;
  static constexpr int kBytes = 2 * 3 * kPlane;  // HALO 6: 20,064 bytes; HALO 24: 55,680
};
static_assert(BlurTile<3 * (JB_COLOR_BLUR_BOX_MAX + 1)>::kBytes <= 64 * 1024, "the blur tile must fit a workgroup's LDS");

// the lines [0, n_lines) of one pass, a thread each: line L is plane L / per_plane, row or column L % per_plane + first_line
// (no division: three planes)
template <int HALO>
static __device__ __forceinline__ void blur_pass(const uint8_t *in, uint8_t *out, bool rows, int first_line, int per_plane, int first, int last,
                                                 int lo, int hi, const JbBlurWeights &k) {
  using T = BlurTile<HALO>;
  for (int L = (int)threadIdx.x; L < 3 * per_plane; L += 256) {
    const int c = L >= 2 * per_plane ? 2 : L >= per_plane ? 1 : 0;
    const int line = L - c * per_plane + first_line;
    const int at = c * T::kPlane + (rows ? line * T::kPitch : line);
    jbc_blur_line(in + at, out + at, rows ? 1 : T::kPitch, first, last, lo, hi, k);
  }
}

// jb_color_blur_kernel -- grid (tiles of 64 x 32 pixels, views); only the views whose chain has a JB_COLOR_BLUR.  The
// workgroup loads its tile and 3 (r + 1) samples around it from the uint8 stage, positions clamped to the view, applies the
// ops in front of the blur (with the contrast's mean) to every loaded pixel, runs three row passes and three column passes
// between two LDS buffers -- each over the region the later passes still read: it shrinks by r + 1 a pass, and only
// positions INSIDE the view are computed, because a read outside the view goes to the view's edge sample in EVERY pass
// (jbc_blur_line's clamp) -- then applies the ops behind the blur and stores through color_store.  r, ww, fw and every
// branch on an op are uniform over the workgroup.
// WARP: the launch has a chain with a geometric operation: every loaded sample is jbc_gather's at its clamped position
template <int FORMAT, int HALO, bool NEW_OPS, bool WARP = false>
__global__ __launch_bounds__(256) void jb_color_blur_kernel(const JbColor p, const JbColorTable table, const JbBlurTable blur) {
  using T = BlurTile<HALO>;
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const JbcShape shape = jbc_shape(row.chain);
  const int at = shape.nbhd;
  if (at < 0 || row.chain.ops[at].op != JB_COLOR_BLUR) return;  // (the whole workgroup: the view is jb_color_apply_kernel's)
  const JbBlurWeights k = blur.k[view];
  const int step = k.r + 1, halo = 3 * step;
  if (halo > HALO) return;  // (the launch picks HALO from the largest r: not reached)
  __shared__ uint8_t lds[2][3 * T::kPlane];
  const uint32_t tiles_x = (uint32_t)(p.w + kBlurW - 1) / (uint32_t)kBlurW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kBlurW, y0 = (int)(blockIdx.x / tiles_x) * kBlurH;
  // local (0, 0) of the tile's buffers is the view's (bx, by); bw x bh samples are loaded
  const int bx = x0 - halo, by = y0 - halo, bw = kBlurW + 2 * halo, bh = kBlurH + 2 * halo;
  const JbcCtx ctx = color_ctx(p, shape, view);
  const uint8_t *const src = p.src + row.src_offset;
  // a thread per loaded sample position, 256 adjacent ones a round (rows of bw = 70..112 positions: whole waves stay busy,
  // which a wave per row would not: 76 = 64 + 12).  i / bw as a multiplication: exact while i * (inv * bw - 2^24) < 2^24,
  // and i < 112 * 80, inv * bw - 2^24 < bw <= 112; i * inv < 2^32.
  const uint32_t inv = ((1u << 24) + (uint32_t)bw - 1u) / (uint32_t)bw;
#pragma unroll 4
  for (int i = (int)threadIdx.x; i < bw * bh; i += 256) {
    const int ly = (int)(((uint32_t)i * inv) >> 24), lx = i - ly * bw;
    const int gy = min(max(by + ly, 0), p.h - 1), gx = min(max(bx + lx, 0), p.w - 1);
    int r, g, b;
    if constexpr (WARP) {
      jbc_gather<NEW_OPS>(row.chain, jbc_warp_shape(row.chain), at, ctx, color_warps(p, view), src, p.src_row_stride, p.w, p.h, gx, gy, &r, &g, &b);
    } else {
      const uint8_t *const from = src + (int64_t)gy * p.src_row_stride + 3 * gx;
      r = from[0], g = from[1], b = from[2];
      jbc_apply_ops<NEW_OPS>(row.chain, 0, at, ctx, &r, &g, &b);
    }
    uint8_t *const to = &lds[0][ly * T::kPitch + lx];
    to[0] = (uint8_t)r, to[T::kPlane] = (uint8_t)g, to[2 * T::kPlane] = (uint8_t)b;
  }
  // the view's extent in local coordinates, and the part of the buffers inside the view
  const int vx0 = -bx, vx1 = p.w - 1 - bx, vy0 = -by, vy1 = p.h - 1 - by;
  const int rows0 = max(0, vy0), rows1 = min(bh, vy1 + 1);              // the rows the row passes run over
  const int cols0 = halo, cols1 = min(halo + kBlurW, vx1 + 1);          // the columns the column passes run over
#pragma unroll 1
  for (int pass = 1; pass <= 3; pass++) {
    __syncthreads();
    blur_pass<HALO>(lds[(pass - 1) & 1], lds[pass & 1], true, rows0, rows1 - rows0, max(pass * step, vx0), min(bw - pass * step, vx1 + 1), vx0, vx1, k);
  }
#pragma unroll 1
  for (int pass = 1; pass <= 3; pass++) {
    __syncthreads();
    blur_pass<HALO>(lds[pass & 1], lds[(pass - 1) & 1], false, cols0, cols1 - cols0, max(pass * step, vy0), min(bh - pass * step, vy1 + 1), vy0, vy1, k);
  }
  __syncthreads();
  // the result is in lds[0]: 16 groups of 4 pixels a row, 32 rows
  const int n_ops = row.chain.n_ops;
  for (int item = (int)threadIdx.x; item < (kBlurW / 4) * kBlurH; item += 256) {
    const int ry = item / (kBlurW / 4), x = x0 + 4 * (item % (kBlurW / 4)), y = y0 + ry;
    if (y >= p.h || x >= p.w) continue;
    const int n = min(4, p.w - x);
    const uint8_t *const from = &lds[0][(halo + ry) * T::kPitch + halo + (x - x0)];
    int px[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int c = 0; c < 3; c++) px[i][c] = i < n ? from[c * T::kPlane + i] : 0;
      if (i < n) jbc_apply_ops<NEW_OPS>(row.chain, at + 1, n_ops, ctx, &px[i][0], &px[i][1], &px[i][2]);
    }
    color_store<FORMAT>(p, p.dst + row.dst_offset + (int64_t)y * p.dst_row_stride, x, n, px);
  }
}

// jb_color_sharp_kernel -- grid (tiles of 64 x 32 pixels, views); only the views whose chain has a JB_COLOR_SHARPNESS.  A
// kernel of its own, not a mode of the blur kernel's tile: one pass, a halo of 1, 6.9 KB of LDS.  The blur kernel's order: the
// workgroup loads its tile and one sample around it (positions clamped to the view; a clamped sample is never read, because
// the view's outermost rows and columns are not filtered), the ops in front of the sharpness applied to every loaded pixel;
// then a thread per 4 pixels of a row blends each sample with its SMOOTH (jbc_smooth), applies the ops behind and stores
// through color_store.
static constexpr int kSharpW = kBlurW + 2, kSharpH = kBlurH + 2, kSharpPitch = (((kSharpW + 3) / 4) | 1) * 4, kSharpPlane = kSharpPitch * kSharpH;
template <int FORMAT, bool WARP = false>
__global__ __launch_bounds__(256) void jb_color_sharp_kernel(const JbColor p, const JbColorTable table) {
  const uint32_t view = blockIdx.y;
  const JbColorRow &row = table.r[view];
  const JbcShape shape = jbc_shape(row.chain);
  const int at = shape.nbhd;
  if (at < 0 || row.chain.ops[at].op != JB_COLOR_SHARPNESS) return;  // (the whole workgroup: the view is another kernel's)
  __shared__ uint8_t lds[3 * kSharpPlane];
  const uint32_t tiles_x = (uint32_t)(p.w + kBlurW - 1) / (uint32_t)kBlurW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kBlurW, y0 = (int)(blockIdx.x / tiles_x) * kBlurH;
  const JbcCtx ctx = color_ctx(p, shape, view);
  const uint8_t *const src = p.src + row.src_offset;
  // local (lx, ly) is the view's (x0 - 1 + lx, y0 - 1 + ly); i / kSharpW as a multiplication: exact for i < 66 * 34 (the blur
  // kernel's bound)
  constexpr uint32_t inv = ((1u << 24) + (uint32_t)kSharpW - 1u) / (uint32_t)kSharpW;
#pragma unroll 3
  for (int i = (int)threadIdx.x; i < kSharpW * kSharpH; i += 256) {
    const int ly = (int)(((uint32_t)i * inv) >> 24), lx = i - ly * kSharpW;
    const int gy = min(max(y0 - 1 + ly, 0), p.h - 1), gx = min(max(x0 - 1 + lx, 0), p.w - 1);
    int r, g, b;
    if constexpr (WARP) {
      jbc_gather<true>(row.chain, jbc_warp_shape(row.chain), at, ctx, color_warps(p, view), src, p.src_row_stride, p.w, p.h, gx, gy, &r, &g, &b);
    } else {
      const uint8_t *const from = src + (int64_t)gy * p.src_row_stride + 3 * gx;
      r = from[0], g = from[1], b = from[2];
      jbc_apply_ops<true>(row.chain, 0, at, ctx, &r, &g, &b);
    }
    uint8_t *const to = &lds[ly * kSharpPitch + lx];
    to[0] = (uint8_t)r, to[kSharpPlane] = (uint8_t)g, to[2 * kSharpPlane] = (uint8_t)b;
  }
  __syncthreads();
  const float factor = row.chain.ops[at].value;
  const int n_ops = row.chain.n_ops;
  for (int item = (int)threadIdx.x; item < (kBlurW / 4) * kBlurH; item += 256) {
    const int ry = item / (kBlurW / 4), x = x0 + 4 * (item % (kBlurW / 4)), y = y0 + ry;
    if (y >= p.h || x >= p.w) continue;
    const int n = min(4, p.w - x);
    const bool edge_row = y == 0 || y == p.h - 1;
    int px[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint8_t *const q = &lds[(1 + ry) * kSharpPitch + 1 + (x - x0) + i];  // (i < 4: inside the tile's 64 columns)
      const bool plain = edge_row || x + i == 0 || x + i >= p.w - 1;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint8_t *const s = q + c * kSharpPlane;
        const int v = s[0];
        int sm = v;
        if (!plain)
          sm = jbc_smooth(s[kSharpPitch - 1], s[kSharpPitch], s[kSharpPitch + 1], s[-1], s[0], s[1], s[-kSharpPitch - 1], s[-kSharpPitch],
                          s[-kSharpPitch + 1]);
        px[i][c] = jbc_blend(sm, v, factor);
      }
      if (i < n) jbc_apply_ops<true>(row.chain, at + 1, n_ops, ctx, &px[i][0], &px[i][1], &px[i][2]);
    }
    color_store<FORMAT>(p, p.dst + row.dst_offset + (int64_t)y * p.dst_row_stride, x, n, px);
  }
}

hipError_t jbk_color_launch(const JbColor &q, const JbColorTable &table, int format, hipStream_t stream) {
  if (format < 0 || format > 3 || q.w < 1 || q.h < 1 || q.w > 65535 || q.h > 65535 || q.n_views < 1 || q.n_views > kJbCropsPerLaunch || !q.src ||
      !q.dst || !q.sums || q.src_row_stride < 3LL * q.w)
    return hipErrorInvalidValue;
  bool contrast = false, hists = false, news = false, sharp = false, mean_in[JB_COLOR_STATS_MAX] = {}, hist_in[JB_COLOR_STATS_MAX] = {};
  int blur_r = -1;  // the largest box radius of the launch's blurs
  JbBlurTable blurs = {};
  bool warp = false;  // a chain of the launch has a geometric operation: the WARP instantiations, behind the table's kernel
  JbWarpTable warps = {};
  for (int i = 0; i < q.n_views; i++) {
    const JbColorRow &r = table.r[i];
    if (r.src_offset < 0 || r.dst_offset < 0 || r.chain.n_ops < 0 || r.chain.n_ops > JB_COLOR_OPS_MAX) return hipErrorInvalidValue;
    const JbcShape shape = jbc_shape(r.chain);
    if (jbc_has_new_ops(r.chain)) news = true;
    const JbcWarpShape ws = jbc_warp_shape(r.chain);
    for (int k = 0; k < JB_COLOR_WARPS_MAX; k++) {
      const int at = k == 0 ? ws.warp0 : ws.warp1;
      if (at < 0) continue;
      const char *why;
      // (the caller has checked the chains against the views' size; a geometric operation behind the neighbourhood operation
      // would not be gathered by the tile kernels)
      if (jbc_warp_params(r.chain.ops[at].op, r.chain.ops[at].value, q.w, q.h, &warps.k[i][k], &why) != JB_OK || (shape.nbhd >= 0 && at > shape.nbhd))
        return hipErrorInvalidValue;
      warp = true;
    }
    // the statistics kernels apply the ops in front of their operation: never a neighbourhood operation (jb_color_check refuses
    // a statistics operation behind one), and the scratch holds JB_COLOR_STATS_MAX statistics a view
    if (shape.n_stats > JB_COLOR_STATS_MAX || (shape.nbhd >= 0 && shape.n_stats > 0 && jbc_stat_at(shape, shape.n_stats - 1) > shape.nbhd))
      return hipErrorInvalidValue;
    for (int k = 0; k < shape.n_stats; k++) {
      if (r.chain.ops[jbc_stat_at(shape, k)].op == JB_COLOR_CONTRAST)
        contrast = mean_in[k] = true;
      else
        hists = hist_in[k] = true;
    }
    if (shape.nbhd >= 0 && r.chain.ops[shape.nbhd].op == JB_COLOR_BLUR) {
      bool geometry;
      if (!jbc_blur_weights(r.chain.ops[shape.nbhd].value, &blurs.k[i], &geometry)) return hipErrorInvalidValue;
      blur_r = blurs.k[i].r > blur_r ? blurs.k[i].r : blur_r;
    } else if (shape.nbhd >= 0) {
      sharp = true;
    }
  }
  if (warp) news = true;  // (the WARP instantiations are built with every operation)
  JbColor p = q;
  p.tiles_x = (p.w + 255) / 256;
  const int tiles_y = (p.h + kColorRows - 1) / kColorRows;  // (at most 256 x 16,384 workgroups a view)
  if (contrast || hists) {
    // the sums, and in a launch with a histogram operation the counters of its views behind them
    const size_t bytes = sizeof(unsigned long long) * kJbCropsPerLaunch + (hists ? (size_t)p.n_views * JB_COLOR_STATS_MAX * kJbColorCounterBytes : 0);
    hipError_t e = hipMemsetAsync(p.sums, 0, bytes, stream);
    if (e != hipSuccess) return e;
  }
  if (warp) {
    hipLaunchKernelGGL(jb_color_warp_table_kernel, dim3(1), dim3(256), 0, stream, p, warps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  for (int k = 0; k < JB_COLOR_STATS_MAX; k++) {
    if (mean_in[k]) {
      const dim3 mean_grid((unsigned)((p.h + kMeanRows - 1) / kMeanRows), (unsigned)p.n_views);
      if (warp)
        hipLaunchKernelGGL((jb_color_mean_kernel<true, true>), mean_grid, dim3(256), 0, stream, p, table, k);
      else if (!news)  // (then k is 0: a second statistics operation would be a table operation)
        hipLaunchKernelGGL(jb_color_mean_kernel<false>, dim3((unsigned)((p.h + kMeanRows - 1) / kMeanRows), (unsigned)p.n_views), dim3(256), 0, stream, p, table, k);
      else
        hipLaunchKernelGGL(jb_color_mean_kernel<true>, dim3((unsigned)((p.h + kMeanRows - 1) / kMeanRows), (unsigned)p.n_views), dim3(256), 0, stream, p, table, k);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    if (hist_in[k]) {
      const dim3 hist_grid((unsigned)((p.h + kHistRows - 1) / kHistRows), (unsigned)p.n_views);
      if (warp)
        hipLaunchKernelGGL(jb_color_hist_kernel<true>, hist_grid, dim3(256), 0, stream, p, table, k);
      else
        hipLaunchKernelGGL(jb_color_hist_kernel<false>, hist_grid, dim3(256), 0, stream, p, table, k);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(jb_color_table_kernel, dim3(1, (unsigned)p.n_views), dim3(256), 0, stream, p, table, k);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  const dim3 grid((unsigned)(p.tiles_x * tiles_y), (unsigned)p.n_views), block(64 * kColorRows);
  jb_by_format(format, [&](auto F) {
    if (warp)
      hipLaunchKernelGGL((jb_color_apply_kernel<decltype(F)::value, true, true>), grid, block, 0, stream, p, table);
    else if (news)
      hipLaunchKernelGGL((jb_color_apply_kernel<decltype(F)::value, true>), grid, block, 0, stream, p, table);
    else
      hipLaunchKernelGGL((jb_color_apply_kernel<decltype(F)::value, false>), grid, block, 0, stream, p, table);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || (blur_r < 0 && !sharp)) return e;
  // the tile kernels, the blur's with the small halo (r <= 1: every published pipeline; 20 KB of LDS) or the one for r <= 7 (56 KB)
  const dim3 blur_grid((unsigned)(((p.w + kBlurW - 1) / kBlurW) * ((p.h + kBlurH - 1) / kBlurH)), (unsigned)p.n_views);
  if (blur_r >= 0)
    jb_by_format(format, [&](auto F) {
      constexpr int kLarge = 3 * (JB_COLOR_BLUR_BOX_MAX + 1);
      if (warp && blur_r <= 1)
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, 6, true, true>), blur_grid, dim3(256), 0, stream, p, table, blurs);
      else if (warp)
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, kLarge, true, true>), blur_grid, dim3(256), 0, stream, p, table, blurs);
      else if (blur_r <= 1 && !news)
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, 6, false>), blur_grid, dim3(256), 0, stream, p, table, blurs);
      else if (blur_r <= 1)
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, 6, true>), blur_grid, dim3(256), 0, stream, p, table, blurs);
      else if (!news)
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, kLarge, false>), blur_grid, dim3(256), 0, stream, p, table, blurs);
      else
        hipLaunchKernelGGL((jb_color_blur_kernel<decltype(F)::value, kLarge, true>), blur_grid, dim3(256), 0, stream, p, table, blurs);
    });
  if (sharp)
    jb_by_format(format, [&](auto F) {
      if (warp)
        hipLaunchKernelGGL((jb_color_sharp_kernel<decltype(F)::value, true>), blur_grid, dim3(256), 0, stream, p, table);
      else
        hipLaunchKernelGGL((jb_color_sharp_kernel<decltype(F)::value, false>), blur_grid, dim3(256), 0, stream, p, table);
    });
  return hipGetLastError();
}
