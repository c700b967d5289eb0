// jb_orient.hip -- "orientation" (include/jpegblk.h): T_o of a tight interleaved uint8 image (what the pixel kernel
// wrote into the context's scratch), into the caller's buffer in any of the four output formats, or -- in front of
// the resample and filter kernels -- into a second tight uint8 region of the same scratch.
//
// One workgroup of 256 lanes moves one 64 x 64 tile of SOURCE pixels through LDS.  Load: wave w takes tile rows
// 16 w .. 16 w + 15, its 64 lanes the 64 columns -- one 4-byte load per lane at byte 3 * x of the row, as
// jb_resample_kernel reads a pixel (the fourth byte is the next pixel's red or slack, and is masked off), through a
// descriptor of the row + 4 bytes: a wave instruction covers one contiguous 192-byte run.  Store: wave w takes 16
// OUTPUT rows of the tile, its lanes 64 adjacent output columns in ascending order -- a mirrored axis reads LDS
// backwards, a transposing orientation reads a column of the tile -- so a wave instruction again covers one contiguous
// run of one row, for all eight orientations: no lane-strided global access.
// LDS: one word per pixel, rows of 65 words.  The row-wise writes (ds_write_b32: bank = word % 32 within a 32-lane
// half) hit 32 consecutive words; the column-wise reads hit words 65 apart = banks 1 apart: neither conflicts.
// Edges are predicated, not padded: a lane whose source pixel lies outside the image stores nothing, and its load is
// cut off by the descriptor's range.
#ifndef JB_ORIENT_HOST
#include <hip/hip_runtime.h>

#include "jb_kernels.h"
#include "jb_launch.h"
#endif
#include "jb_orient.h"
#include "jb_store.h"

static constexpr int kOrientPitch = kJbOrientTile + 1;     // words per LDS row
static constexpr int kOrientRowsPerWave = kJbOrientTile / 4;

// which tile of which image a workgroup has; false: none (a table's image with fewer tiles than the launch's largest)
struct OrientTile {
  uint32_t img, sx0, sy0, sw, sh;
  const uint8_t *src;
  uint8_t *dst;
  int64_t dst_row_stride;
};
static __device__ __forceinline__ const JbOrientRow *orient_rows(const JbOrientTable &table) { return table.r; }
template <bool TABLE, typename... T>
static __device__ __forceinline__ bool orient_tile(const JbOrient &p, uint32_t block, OrientTile &t, const T &...table) {
  t.img = block / (uint32_t)p.tiles_per_image;
  const uint32_t k = block % (uint32_t)p.tiles_per_image;
  if (t.img >= (uint32_t)p.n_images) return false;
  uint32_t tiles_x = (uint32_t)p.tiles_x;
  if constexpr (TABLE) {
    const JbOrientRow &r = orient_rows(table...)[t.img];
    t.sw = (uint32_t)r.sw, t.sh = (uint32_t)r.sh;
    tiles_x = (t.sw + kJbOrientTile - 1) / kJbOrientTile;
    if (k >= tiles_x * ((t.sh + kJbOrientTile - 1) / kJbOrientTile)) return false;
    t.src = p.src + r.src_offset;
    t.dst = p.dst + r.dst_offset;
    t.dst_row_stride = 3LL * (jb_orient_bits(p.orientation).transpose ? t.sh : t.sw);
  } else {
    t.sw = (uint32_t)p.sw, t.sh = (uint32_t)p.sh;
    t.src = p.src + (int64_t)t.img * p.src_image_stride;
    t.dst = p.dst + (int64_t)t.img * p.dst_image_stride;
    t.dst_row_stride = p.dst_row_stride;
  }
  t.sx0 = (k % tiles_x) * kJbOrientTile, t.sy0 = (k / tiles_x) * kJbOrientTile;
  return t.sy0 < t.sh;  // (the grid never has such a tile; the guard keeps every row base inside the image)
}

// the load half of a lane: its 16 source pixels into LDS.  Nothing here is predicated, so the 16 loads are in flight
// together: a row below the image gets a descriptor of range 0 over the last row (the load returns 0), a column right
// of the image reads the next row's first bytes, the slack behind the scratch, or beyond the range 0 -- words the
// store half never looks at.
static __device__ __forceinline__ void orient_load(const OrientTile &t, int wave, int lane, uint32_t *lds) {
  const uint32_t sx = t.sx0 + (uint32_t)lane;
  uint32_t v[kOrientRowsPerWave];
#pragma unroll
  for (int k = 0; k < kOrientRowsPerWave; k++) {
    const uint32_t sy = t.sy0 + (uint32_t)(wave * kOrientRowsPerWave + k);
    const uint32_t row_in = sy < t.sh ? sy : t.sh - 1;
    const __amdgpu_buffer_rsrc_t row = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(t.src + (int64_t)row_in * (3LL * t.sw)), 0,
                                                                        sy < t.sh ? (int)(3 * t.sw + 4) : 0, 0x00020000);
    v[k] = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * sx), 0, 0);
  }
#pragma unroll
  for (int k = 0; k < kOrientRowsPerWave; k++) lds[(wave * kOrientRowsPerWave + k) * kOrientPitch + lane] = v[k] & 0xffffffu;
}

// the store half: 16 output rows of the tile, this lane's column of each
template <int FORMAT>
static __device__ __forceinline__ void orient_store(const JbOrient &p, const OrientTile &t, int wave, int lane, const uint32_t *lds) {
  const JbOrientBits b = jb_orient_bits(p.orientation);
  // the lane runs along the tile's rows when the output's x is the source's y
  const int along = b.transpose ? (b.flip_y ? kJbOrientTile - 1 - lane : lane) : (b.flip_x ? kJbOrientTile - 1 - lane : lane);
  uint32_t word[kOrientRowsPerWave];  // (every word of the tile has been written: the reads need no predicate)
#pragma unroll
  for (int k = 0; k < kOrientRowsPerWave; k++) {
    const int j = wave * kOrientRowsPerWave + k;
    word[k] = lds[(b.transpose ? along : j) * kOrientPitch + (b.transpose ? j : along)];
  }
#pragma unroll
  for (int k = 0; k < kOrientRowsPerWave; k++) {
    const int j = wave * kOrientRowsPerWave + k;
    const int lr = b.transpose ? along : j, lc = b.transpose ? j : along;  // the pixel's place in the tile
    const uint32_t sy = t.sy0 + (uint32_t)lr, sx = t.sx0 + (uint32_t)lc;
    if (sy >= t.sh || sx >= t.sw) continue;
    const uint32_t u = b.flip_y ? t.sh - 1 - sy : sy, v = b.flip_x ? t.sw - 1 - sx : sx;
    const uint32_t oy = b.transpose ? v : u, ox = b.transpose ? u : v;
    const uint32_t px = word[k];
    uint8_t *const row = t.dst + (int64_t)oy * t.dst_row_stride;
#pragma unroll
    for (int c = 0; c < 3; c++) jb_store_element<FORMAT>(row, p.dst_plane_stride, ox, c, (px >> (8 * c)) & 0xffu, p.scale, p.bias);
  }
}

#ifndef JB_ORIENT_HOST
template <int FORMAT, bool TABLE = false, typename... T>
__global__ __launch_bounds__(256) void jb_orient_kernel(const JbOrient p, const T... table) {
  static_assert(sizeof...(T) == (TABLE ? 1 : 0), "the table is the second argument of the TABLE instantiations alone");
  __shared__ uint32_t lds[kJbOrientTile * kOrientPitch];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  OrientTile t;
  if (!orient_tile<TABLE>(p, blockIdx.x, t, table...)) return;  // (block-uniform: nobody is left at the barrier)
  orient_load(t, wave, lane, lds);
  __syncthreads();
  orient_store<FORMAT>(p, t, wave, lane, lds);
}

// the grid of a launch (tiles_x, tiles_per_image into p) for images of at most sw x sh; false: more than 2^31 - 1 workgroups
static bool orient_grid(JbOrient &p, int32_t sw, int32_t sh, dim3 *grid) {
  p.tiles_x = (sw + kJbOrientTile - 1) / kJbOrientTile;
  p.tiles_per_image = p.tiles_x * ((sh + kJbOrientTile - 1) / kJbOrientTile);  // at most 1024^2
  const int64_t n = (int64_t)p.tiles_per_image * p.n_images;
  if (n > 0x7fffffffLL) return false;
  *grid = dim3((unsigned)n);
  return true;
}

hipError_t jbk_orient_launch(const JbOrient &q, int format, hipStream_t stream) {
  if (format < 0 || format > 3 || q.sw < 1 || q.sh < 1 || q.sw > 65535 || q.sh > 65535 || q.n_images < 1 || q.orientation < 1 ||
      q.orientation > 8)
    return hipErrorInvalidValue;
  JbOrient p = q;
  dim3 grid;
  if (!orient_grid(p, p.sw, p.sh, &grid)) return hipErrorInvalidValue;
  jb_by_format(format, [&](auto F) { hipLaunchKernelGGL(jb_orient_kernel<decltype(F)::value>, grid, dim3(256), 0, stream, p); });
  return hipGetLastError();
}

hipError_t jbk_orient_launch_table(const JbOrient &q, const JbOrientTable &table, hipStream_t stream) {
  if (q.n_images < 1 || q.n_images > kJbCropsPerLaunch || q.orientation < 1 || q.orientation > 8) return hipErrorInvalidValue;
  int32_t most = 0;  // the image with the most tiles decides the grid
  JbOrient p = q;
  for (int i = 0; i < q.n_images; i++) {
    const JbOrientRow &r = table.r[i];
    if (r.sw < 1 || r.sh < 1 || r.sw > 65535 || r.sh > 65535 || r.src_offset < 0 || r.dst_offset < 0) return hipErrorInvalidValue;
    const int32_t n = ((r.sw + kJbOrientTile - 1) / kJbOrientTile) * ((r.sh + kJbOrientTile - 1) / kJbOrientTile);
    if (n > most) most = n;
  }
  p.tiles_x = 0;
  p.tiles_per_image = most;  // (at most 32 * 1024^2 workgroups: below 2^31)
  hipLaunchKernelGGL((jb_orient_kernel<0, true, JbOrientTable>), dim3((unsigned)(most * q.n_images)), dim3(256), 0, stream, p, table);
  return hipGetLastError();
}
#endif
