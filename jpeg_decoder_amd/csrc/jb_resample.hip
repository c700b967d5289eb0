// jb_resample.hip -- "fixed output size" (include/jpegblk.h): the exact area resize of a tight interleaved uint8 image
// (what the pixel kernel of jb_kernels.hip wrote into the context's scratch) to the caller's ow x oh output, in any of
// the four output formats.  A second kernel behind the pixel kernel, not a store stage of it: an area filter crosses
// the pixel kernel's tile boundaries, and that kernel has no registers to spare.
//
// On a common grid of iw * ow units per axis source column i covers [i * ow, (i + 1) * ow) and output column j covers
// [j * iw, (j + 1) * iw); wx[j][i] is the integer length of their overlap (sum over i = iw); rows the same with wy, ih,
// oh.  Per channel S = sum_r sum_i wy[k][r] * wx[j][i] * src[r][i] (an exact integer below 2^40) and
// out = floor((S + floor(D / 2)) / D), D = iw * ih: one rounding, half up.  Every weight of a footprint is ow (oh)
// except the first and the last one, so a lane needs two weights per axis and no table.
//
// One lane = one output pixel.  The 64 lanes of a wave are 64 adjacent columns of ONE output row, the 4 waves of a
// workgroup 4 adjacent rows: the source rows of the footprint, their weights and the buffer descriptor of a source row
// are wave-uniform, and adjacent lanes read adjacent byte runs, so a wave covers one contiguous span per source row.
// A pixel is ONE 4-byte load at byte 3 * i of its row (gfx950 under ROCm runs with unaligned buffer access enabled;
// the fourth byte is the next pixel's red, or one byte of the slack behind the scratch, and is not looked at).  The
// descriptor's range (the row + 4 bytes) keeps every load inside the scratch whatever the arithmetic above it does.
// The two divisions per lane that bound the column footprint, and the two per wave for the rows, are outside the loops.
#include <hip/hip_runtime.h>

#include "jb_kernels.h"

static constexpr int kResampleRows = 4;  // output rows (= waves) per workgroup

// the rows of a kernel's by-value table argument
static __device__ __forceinline__ const JbCrop *crops_of(const JbCropTable &table) { return table.c; }

// floor(n / d) for n < 2^41, 1 <= d < 2^32 with a quotient of at most 255: a float estimate (a few units off at the
// worst) and integer correction steps that make it exact whatever the estimate was
static __device__ __forceinline__ uint32_t div_to_u8(uint64_t n, uint32_t d, float rcp_d) {
  uint32_t q = (uint32_t)fminf((float)n * rcp_d, 255.0f);
  while ((uint64_t)q * d > n) q--;
  while ((uint64_t)(q + 1) * d <= n) q++;
  return q;
}

// CROPS ("per-image rectangles"; TABLE is then JbCropTable, a second kernel argument, and empty otherwise): the source of
// image `img` is table.c[img].w x .h at p.src + .tmp_offset instead of p.iw x p.ih at p.src + img * p.src_image_stride --
// img comes from blockIdx, so the table reads are scalar loads and everything derived from them stays wave-uniform.
template <int FORMAT, bool CROPS = false, typename... TABLE>
__global__ __launch_bounds__(64 * kResampleRows) void jb_resample_kernel(const JbResample p, const TABLE... table) {
  static_assert(sizeof...(TABLE) == (CROPS ? 1 : 0), "the table is the second argument of the CROPS instantiations alone");
  // (the wave id is wave-uniform, and only readfirstlane tells the compiler so)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t b = blockIdx.x;
  const uint32_t tx = b % (uint32_t)p.tiles_x, t = b / (uint32_t)p.tiles_x;
  const uint32_t ty = t % (uint32_t)p.tiles_y, img = t / (uint32_t)p.tiles_y;
  uint32_t iw = (uint32_t)p.iw, ih = (uint32_t)p.ih;
  const uint32_t ow = (uint32_t)p.ow, oh = (uint32_t)p.oh;
  const uint32_t k = ty * kResampleRows + (uint32_t)wave;  // output row (wave-uniform)
  const uint32_t j = tx * 64 + (uint32_t)lane;             // output column
  if (k >= oh || j >= ow || img >= (uint32_t)p.n_images) return;
  [[maybe_unused]] int64_t src_offset = 0;
  if constexpr (CROPS) {  // this image's source
    const JbCrop &c = crops_of(table...)[img];
    iw = (uint32_t)c.w, ih = (uint32_t)c.h;
    src_offset = c.tmp_offset;
  }

  // the footprints on the common grid: products below 65535^2 < 2^32
  const uint32_t r0 = k * ih / oh, r1 = ((k + 1) * ih - 1) / oh;  // source rows r0..r1, wave-uniform
  const uint32_t i0 = j * iw / ow, i1 = ((j + 1) * iw - 1) / ow;  // source columns i0..i1
  // the first and the last weight of a footprint (every one between them is ow, resp. oh)
  const uint32_t wx0 = min((i0 + 1) * ow, (j + 1) * iw) - j * iw;
  const uint32_t wx1 = (j + 1) * iw - i1 * ow;  // (used when i1 > i0)
  const uint32_t wy0 = min((r0 + 1) * oh, (k + 1) * ih) - k * ih;
  const uint32_t wy1 = (k + 1) * ih - r1 * oh;  // (used when r1 > r0)

  const uint8_t *const src = p.src + (CROPS ? src_offset : (int64_t)img * p.src_image_stride);
  const int64_t src_row_bytes = 3LL * iw;
  uint64_t acc[3] = {0, 0, 0};
  for (uint32_t r = r0; r <= r1; r++) {
    const __amdgpu_buffer_rsrc_t row =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src + (int64_t)r * src_row_bytes), 0, (int)(3 * iw + 4), 0x00020000);
    // the horizontal partial sum: sum of wx * sample <= 255 * iw < 2^24
    uint32_t px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * i0), 0, 0);
    uint32_t h[3] = {wx0 * (px & 0xffu), wx0 * ((px >> 8) & 0xffu), wx0 * ((px >> 16) & 0xffu)};
    if (i1 > i0) {
      uint32_t m[3] = {0, 0, 0};  // the samples of weight ow
      uint32_t i = i0 + 1;
      for (; i + 8 <= i1; i += 8) {  // eight loads in flight: a long footprint is bound by their latency
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * (i + u)), 0, 0);
#pragma unroll
        for (int u = 0; u < 8; u++) m[0] += v[u] & 0xffu, m[1] += (v[u] >> 8) & 0xffu, m[2] += (v[u] >> 16) & 0xffu;
      }
      for (; i < i1; i++) {
        px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * i), 0, 0);
        m[0] += px & 0xffu, m[1] += (px >> 8) & 0xffu, m[2] += (px >> 16) & 0xffu;
      }
      px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * i1), 0, 0);
#pragma unroll
      for (int c = 0; c < 3; c++) h[c] += ow * m[c] + wx1 * ((px >> (8 * c)) & 0xffu);
    }
    const uint32_t wy = r == r0 ? wy0 : r == r1 ? wy1 : oh;
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] += (uint64_t)wy * h[c];
  }

  const uint32_t d = iw * ih;
  const float rcp_d = 1.0f / (float)d;
  uint8_t *const dst = p.dst + (int64_t)img * p.dst_image_stride + (int64_t)k * p.dst_row_stride;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const uint32_t u = div_to_u8(acc[c] + (d >> 1), d, rcp_d);
    if constexpr (FORMAT == 0) {
      dst[3 * (int64_t)j + c] = (uint8_t)u;
    } else if constexpr (FORMAT == 1) {
      dst[(int64_t)c * p.dst_plane_stride + j] = (uint8_t)u;
    } else {
      // the planar store stage's expression, operation for operation: u8 -> f32 (exact), one f32 multiply, one f32 add
      // (separate instructions: built with -ffp-contract=off), for f16 one v_cvt_f16_f32 (round to nearest even)
      const float f = (float)u * p.scale[c] + p.bias[c];
      uint8_t *const at = dst + (int64_t)c * p.dst_plane_stride;
      if constexpr (FORMAT == 2) ((float *)at)[j] = f;
      else ((_Float16 *)at)[j] = (_Float16)f;
    }
  }
}

// the grid of a launch (tiles_x, tiles_y into p); false: more than 2^31 - 1 workgroups
static bool resample_grid(JbResample &p, dim3 *grid) {
  p.tiles_x = (p.ow + 63) / 64;
  p.tiles_y = (p.oh + kResampleRows - 1) / kResampleRows;
  const int64_t n_wgs = (int64_t)p.tiles_x * p.tiles_y * p.n_images;
  if (n_wgs > 0x7fffffffLL) return false;
  *grid = dim3((unsigned)n_wgs);
  return true;
}

hipError_t jbk_resample_launch_crops(const JbResample &q, const JbCropTable &table, int format, hipStream_t stream) {
  if (format < 0 || format > 3 || q.ow < 1 || q.oh < 1 || q.ow > 65535 || q.oh > 65535 || q.n_images < 1 || q.n_images > kJbCropsPerLaunch)
    return hipErrorInvalidValue;
  for (int i = 0; i < q.n_images; i++)
    if (table.c[i].w < 1 || table.c[i].h < 1 || table.c[i].w > 65535 || table.c[i].h > 65535 || table.c[i].tmp_offset < 0)
      return hipErrorInvalidValue;
  JbResample p = q;
  dim3 grid;
  if (!resample_grid(p, &grid)) return hipErrorInvalidValue;
  const dim3 block(64 * kResampleRows);
  switch (format) {
    case 0: hipLaunchKernelGGL((jb_resample_kernel<0, true, JbCropTable>), grid, block, 0, stream, p, table); break;
    case 1: hipLaunchKernelGGL((jb_resample_kernel<1, true, JbCropTable>), grid, block, 0, stream, p, table); break;
    case 2: hipLaunchKernelGGL((jb_resample_kernel<2, true, JbCropTable>), grid, block, 0, stream, p, table); break;
    default: hipLaunchKernelGGL((jb_resample_kernel<3, true, JbCropTable>), grid, block, 0, stream, p, table); break;
  }
  return hipGetLastError();
}

hipError_t jbk_resample_launch(const JbResample &q, int format, hipStream_t stream) {
  if (format < 0 || format > 3 || q.iw < 1 || q.ih < 1 || q.ow < 1 || q.oh < 1 || q.iw > 65535 || q.ih > 65535 || q.ow > 65535 ||
      q.oh > 65535 || q.n_images < 1)
    return hipErrorInvalidValue;
  JbResample p = q;
  dim3 grid;
  if (!resample_grid(p, &grid)) return hipErrorInvalidValue;
  const dim3 block(64 * kResampleRows);
  switch (format) {
    case 0: hipLaunchKernelGGL(jb_resample_kernel<0>, grid, block, 0, stream, p); break;
    case 1: hipLaunchKernelGGL(jb_resample_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(jb_resample_kernel<2>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(jb_resample_kernel<3>, grid, block, 0, stream, p); break;
  }
  return hipGetLastError();
}
