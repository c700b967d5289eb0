// jb_orient.h -- "orientation" (include/jpegblk.h): what the host's rectangle mapper (jb_geometry.cpp), the launch
// (jb_seam.cpp) and the kernel (jb_orient.hip) share.  No HIP types: tools/fuzz builds the kernel's body for the CPU.
#pragma once
#include <stdint.h>

#include "jb_knobs.h"

// The eight Exif codes as three bits.  Output pixel (oy, ox) of T_o(full) is source pixel (sy, sx) of the stored
// h x w frame: (u, v) = transpose ? (ox, oy) : (oy, ox); sy = flip_y ? h - 1 - u : u; sx = flip_x ? w - 1 - v : v.
struct JbOrientBits {
  int transpose, flip_x, flip_y;
};
#if defined(__HIPCC__)
#define JB_ORIENT_HD __host__ __device__
#else
#define JB_ORIENT_HD
#endif
// 1: - - -   2: - x -   3: - x y   4: - - y   5: t - -   6: t - y   7: t x y   8: t x -   (anything else: as 1)
JB_ORIENT_HD static inline JbOrientBits jb_orient_bits(int o) {
  return JbOrientBits{o >= 5 && o <= 8, o == 2 || o == 3 || o == 7 || o == 8, o == 3 || o == 4 || o == 6 || o == 7};
}

// the kernel's square tile of pixels (a wave reads and writes one 64-pixel run of a row per instruction)
constexpr int kJbOrientTile = 64;

// n_images tight interleaved uint8 images of sw x sh at src (src_image_stride bytes apart, at least 4 readable bytes
// behind the last one) -> T_o of each at dst, in `format` (JB_FMT_*): sw x sh for 1..4, sh x sw for 5..8; rows
// dst_row_stride bytes apart (of a plane when planar), planes dst_plane_stride, images dst_image_stride; scale / bias:
// the float formats' affine map.  Nothing outside the output's elements is written.
struct JbOrient {
  const uint8_t *src;
  uint8_t *dst;
  int64_t src_image_stride;
  int64_t dst_image_stride, dst_row_stride, dst_plane_stride;
  int32_t sw, sh;  // each in 1..65535
  int32_t orientation;  // 1..8
  int32_t n_images;
  int32_t tiles_x, tiles_per_image;  // (set by the launch) tiles per source row of tiles; workgroups per image
  float scale[3], bias[3];
};
// "per-image rectangles": a source per image, format 0 and tight on both sides -- image i is sw x sh at p.src +
// src_offset, T_o of it tight at p.dst + dst_offset (p.sw, p.sh and the strides are not looked at).  A kernel argument,
// by value, like JbCropTable.
struct JbOrientRow {
  int32_t sw, sh;
  int64_t src_offset, dst_offset;
};
struct JbOrientTable {
  JbOrientRow r[kJbCropsPerLaunch];
};
