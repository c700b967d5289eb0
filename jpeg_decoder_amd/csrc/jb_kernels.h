// jb_kernels.h -- internal interface between the C-ABI layer (jb_api.cpp) and the HIP
// kernels (jb_kernels.hip).  Not part of the public ABI (include/jpegblk.h).
#pragma once
#include <stdint.h>
#ifdef JB_KERNELS_HOST  // (tools/fuzz/views_kernel_check.cpp: kernel bodies compiled for the CPU, no HIP headers)
typedef int hipError_t;
typedef void *hipStream_t;
#else
#include <hip/hip_runtime_api.h>
#endif

#include "../../include/jpegblk.h"  // (jb_color_chain: the colour launch takes the ABI's structure as it is)
#include "jb_divmagic.h"
#include "jb_knobs.h"
#include "jb_orient.h"

// Kernel arguments of one launch: a batch of images of identical geometry.
struct JbLaunch {
  const int16_t *coef;        // device; decode-order int16 blocks
  const int32_t *qtabs;       // device; per image int32[3][64] (Y, Cb, Cr), natural order
  uint8_t *rgb;               // device; interleaved RGB
  int64_t coef_image_stride;  // bytes
  int64_t qtab_image_stride;  // bytes (0 = tables shared by the batch)
  int64_t rgb_image_stride;   // bytes
  int64_t rgb_row_stride;     // bytes
  int32_t width, height;      // pixels
  int32_t mcus_x, mcus_y;     // coded MCUs per row / column
  int32_t tiles_per_row;      // row-bound tiling: ceil(mcus_x / jbk_mcus_per_tile(hs, vs))
  int32_t tiles_per_image;    // linear: ceil(mcus_x*mcus_y / per_tile); row-bound: tiles_per_row*mcus_y
  int32_t n_tiles;            // n_images * tiles_per_image = workgroups launched
  int32_t linear;             // 1 = tiles follow the MCU stream, 0 = tiles are runs of one MCU row
  int32_t fast_store;         // 1: 12-byte stores (any byte alignment); 0: byte stores (JPEGBLK_BYTE_STORE=1)
  int32_t chroma_q_equal;     // 1 when Cb and Cr use the same table (desc.qtab_id[1] == qtab_id[2])
  int32_t reserved;           // 0 (777 = skip switch of the timing-experiment builds)
  int32_t staged;             // 1 (linear tiling only): the line-aligned store stage for rows that are not 64-byte aligned
  int32_t small_grid;         // 1: every layout, one 64-lane workgroup per jbk_small_mcus() MCUs of an MCU row (row-bound)
  // planar output only (format != 0; every other launch leaves these 0): rgb_row_stride is then the bytes between
  // the rows of ONE plane, rgb_plane_stride the bytes between the R, G and B planes of an image
  int32_t format;             // JB_FMT_* of include/jpegblk.h
  int64_t rgb_plane_stride;   // bytes
  float scale[3], bias[3];    // float formats: value = (float)u8 * scale[c] + bias[c]
  // region of interest only (roi = 1; every other launch leaves these 0): the tile grid covers the MCUs the rectangle
  // touches -- tiles_per_row tiles from MCU column roi_mx on, tiles_per_image / tiles_per_row MCU rows from roi_my on;
  // mcus_x / mcus_y, width / height stay the full image's -- and p.rgb and its strides describe the roi_w x roi_h output
  int32_t roi;                // 1: the ROI store stage (row-bound tiling, scale 1, any format); 2: jbk_launch_crops
  int32_t roi_x, roi_y;       // the rectangle, in pixels of the full-size image
  int32_t roi_w, roi_h;
  int32_t roi_mx, roi_my;     // the MCU that holds (roi_x, roi_y): roi_x / (8 * hs), roi_y / (8 * vs)
  // the tile kernel's prologue divides by these three without a division (jb_divmagic.h).  Set by jbk_launch and
  // jbk_launch_crops from the fields above, once per launch, on their own copy of the arguments: callers leave them alone.
  JbDiv div_tiles_per_image, div_tiles_per_row, div_mcus_x;
};

// "Per-image rectangles" (jb_blocks_to_rgb_device_crops): what JbLaunch's roi_* fields say once for a launch, said per
// image, with the image's place in the scratch.  The table is a kernel ARGUMENT, passed by value next to JbLaunch (or
// JbResample): no upload, no staging to fence, and the caller's array is not needed once the launch call has returned.
struct JbCrop {
  int32_t x, y, w, h;      // the rectangle, in pixels of the full-size image
  int32_t mx, my;          // the MCU that holds (x, y)
  int32_t tiles_per_row;   // row-bound tiles that cover the MCU columns the rectangle touches
  int32_t n_tiles;         // tiles_per_row * MCU rows the rectangle touches: the workgroups of this image that do work
  int64_t tmp_offset;      // bytes from the scratch's base to this image's tight 3 * w * h intermediate
};
struct JbCropTable {
  JbCrop c[kJbCropsPerLaunch];
};

// MCUs covered by one workgroup (a tile is 192 coded blocks in 4:4:4 and 4:2:0, 256 in 4:2:2 and 4:4:0): 64 / 32 / 64 / 64.
int jbk_mcus_per_tile(int hs, int vs);
// MCUs per workgroup of the small-grid kernels (4:2:0: 8, every other layout: 16; never 0)
int jbk_small_mcus(int hs, int vs);
// Can the layout use the linear (MCU-stream) tiling for an image with mcus_x MCUs per row?
int jbk_linear_ok(int hs, int vs, int mcus_x);
// Launch the fused kernel for luma sampling (hs, vs): one 192-lane workgroup per tile, or (p.small_grid) one 64-lane
// workgroup per jbk_small_mcus() MCUs.  scale 2, 4 or 8: the same kernel with an area-reduced store stage -- p.width /
// p.height are the full image's, p.rgb and its strides describe the ceil(W/scale) x ceil(H/scale) output.  p.format =
// JB_FMT_RGB_U8_CHW / _F32_CHW / _F16_CHW: the same kernel with a planar store stage -- p.rgb, p.rgb_row_stride,
// p.rgb_plane_stride and p.rgb_image_stride describe three planes of p.height rows of p.width elements per image,
// p.scale / p.bias the float formats' affine map.  Either exists in the row-bound tiling only (p.linear = p.small_grid
// = 0) and not together: anything else is hipErrorInvalidValue.  p.roi = 1: the same kernel with the ROI store stage, for
// scale 1 and any p.format, row-bound tiling only.
// flat = true: the flat entry of the 4:4:4 kernel -- its leading arguments are scalars, delivered in SGPRs at wave start,
// and every wave issues its coefficient loads from p.coef + blockIdx * 24576 before it has read p.  Only for a launch of
// which jbk_flat_front says 1: anything else is hipErrorInvalidValue.
hipError_t jbk_launch(const JbLaunch &p, int hs, int vs, int scale, hipStream_t stream, bool flat = false);
// May the launch jbk_launch(p, hs, vs, scale) take the flat entry?  The full-size store stages of the whole image (any
// format, either tiling; not the small-grid kernels), and the geometry of jb_flat_front_geometry (include/jpegblk.h).
// Nothing about the output enters it.  Host code only.
inline int jbk_flat_front(const JbLaunch &p, int hs, int vs, int scale) {
  if (scale != 1 || p.roi || p.small_grid || p.staged || p.tiles_per_image < 1) return 0;
  return jb_flat_front_geometry(hs, vs, p.linear, p.mcus_x, p.mcus_y, p.n_tiles / p.tiles_per_image, p.coef_image_stride);
}
// p.roi = 2: the ROI store stage with a rectangle per image (format 0, scale 1, row-bound tiling; at most
// kJbCropsPerLaunch images).  The grid is n_images x p.tiles_per_image, p.tiles_per_image the largest n_tiles of the
// table; a workgroup beyond its image's n_tiles returns at once.  Image i is written as tight interleaved uint8 rows
// at p.rgb + table.c[i].tmp_offset; p.rgb_row_stride, p.rgb_image_stride and p.roi_* are not looked at.
hipError_t jbk_launch_crops(const JbLaunch &p, const JbCropTable &table, int hs, int vs, hipStream_t stream);
const char *jbk_kernel_name(int hs, int vs);

// "Decoder arithmetic" (jb_libjpeg.hip): the pixel launches of JB_ARITH_LIBJPEG, the counterparts of jbk_launch and
// jbk_launch_crops.  Two kernels per launch: the coded blocks of every image's MCU WINDOW -- the MCUs its rectangle
// touches, grown by one MCU on every side where chroma is subsampled, clamped to the frame -- go through libjpeg's
// integer IDCT into uint8 Y, Cb, Cr planes at `planes`; the pixel kernel upsamples, converts and stores from there.
struct JbLjWindow {
  int32_t mx, my, nx, ny;  // first MCU, MCUs per row and per column
  int64_t bytes;           // of one image's three planes (a multiple of 256)
};
// "Draft decode" (include/jpegblk.h): `draft` (1, 2, 4, 8) makes p.width x p.height, the rectangles and the windows those
// of the DRAFT FRAME -- an MCU is 8 hs / draft by 8 vs / draft of its pixels, the planes hold the reduced IDCTs' blocks, and
// the halo is kept only where the upsampler still filters; p.mcus_x, p.mcus_y, hs and vs stay the coded frame's.
// the window of the rectangle (x, y, w, h) of a frame of mcus_x x mcus_y MCUs
JbLjWindow jbk_lj_window(int hs, int vs, int draft, int mcus_x, int mcus_y, int x, int y, int w, int h);
// workgroups of the pixel kernel per image of a w x h output (256 pixels x 4 rows each); 0: more than 2^31 - 1
int jbk_lj_tiles(int w, int h);
// Formats 0-3, the whole image or (p.roi = 1) the rectangle p.roi_*: p.tiles_per_image = jbk_lj_tiles of the output,
// p.n_tiles = images * p.tiles_per_image; p.linear, p.small_grid, p.staged, p.fast_store and p.tiles_per_row are not
// looked at.  planes: device scratch of images * jbk_lj_window(...).bytes, the launch's alone until it has run.
hipError_t jbk_lj_launch(const JbLaunch &p, int hs, int vs, int draft, void *planes, hipStream_t stream);
// p.roi = 2: a rectangle per image as for jbk_launch_crops (format 0; of a table row x, y, w, h and tmp_offset are
// looked at); p.tiles_per_image = the largest jbk_lj_tiles of the rectangles.  planes: the sum of the images' windows.
hipError_t jbk_lj_launch_crops(const JbLaunch &p, const JbCropTable &table, int hs, int vs, int draft, void *planes, hipStream_t stream);

// "Fixed output size" (jb_resample.hip): n_images tight interleaved uint8 images of iw x ih at src (src_image_stride bytes
// apart, at least 4 readable bytes behind the last one) -> their exact area resize to ow x oh at dst, in `format`
// (JB_FMT_*): rows dst_row_stride bytes apart (of a plane when planar), planes dst_plane_stride, images
// dst_image_stride; scale / bias: the float formats' affine map.  Nothing outside the ow x oh elements is written.
struct JbResample {
  const uint8_t *src;
  uint8_t *dst;
  int64_t src_image_stride;
  int64_t dst_image_stride, dst_row_stride, dst_plane_stride;
  int32_t iw, ih, ow, oh;  // each in 1..65535
  int32_t n_images;
  int32_t tiles_x, tiles_y;  // (set by jbk_resample_launch: workgroups per output row / column of rows)
  float scale[3], bias[3];
};
// one workgroup per 64 columns x 4 rows of one image's output; more than 2^31 - 1 of them: hipErrorInvalidValue
hipError_t jbk_resample_launch(const JbResample &p, int format, hipStream_t stream);
// the same with a source per image: image i is table.c[i].w x table.c[i].h at p.src + table.c[i].tmp_offset (p.iw,
// p.ih and p.src_image_stride are not looked at); at most kJbCropsPerLaunch images
hipError_t jbk_resample_launch_crops(const JbResample &p, const JbCropTable &table, int format, hipStream_t stream);

// "Resampling filters" (jb_resample.hip jb_filter_kernel): one image's geometry -- the rectangle the outputs map to, and
// the window of the frame that lies in the scratch (jb_filter_window: tight interleaved uint8, win_w x win_h).  A
// JbCrop row has no room for both, so the filtered kernels have a table type of their own: 40 bytes a row, 32 rows and
// JbFilter together 1.4 KB of the 4 KB argument segment.
struct JbFilterRow {
  int32_t x, y, w, h;                  // the rectangle, in pixels of the full-size image
  int32_t win_x, win_y, win_w, win_h;  // the window, in pixels of the full-size image
  int64_t tmp_offset;                  // bytes from the scratch's base to the window's pixels (the table's rows only)
};
struct JbFilterTable {
  JbFilterRow r[kJbCropsPerLaunch];
};
// base: as for jbk_resample_launch (iw, ih are not looked at; without a table image i's window is at base.src + i *
// base.src_image_stride).  one: the geometry of every image of a launch without a table.
struct JbFilter {
  JbResample base;
  JbFilterRow one;
  int32_t frame_w, frame_h;  // the full-size image: what the filter's bounds are clamped to
  int32_t tx_cap, ty_cap;    // (set by the launch) the taps the LDS weight tables hold per column / row
  int32_t t_rows;            // (set by the launch) the rows of horizontally filtered pixels LDS holds at a time
};
// filter: JB_FILTER_BILINEAR / _BICUBIC.  One workgroup per 64 columns x 8 rows of one image's output.  Every window
// must be jb_filter_window of its rectangle and p.base.ow x oh, and the taps within kJbFilterMaxTaps (the plan's checks).
hipError_t jbk_filter_launch(const JbFilter &p, int filter, int format, hipStream_t stream);
// the same with a geometry per image (p.one is not looked at); at most kJbCropsPerLaunch images
hipError_t jbk_filter_launch_crops(const JbFilter &p, const JbFilterTable &table, int filter, int format, hipStream_t stream);

// "Views" (jb_resample.hip): the K outputs of an image read K sub-rectangles of its UNION, which the pixel kernel wrote
// once -- tight interleaved uint8 rows of src_row_bytes = 3 * union_w at src_offset in the scratch.  A launch takes up to
// kJbCropsPerLaunch ROWS (outputs, not images): row n is output n of p.dst (the caller has moved p.dst to the launch's
// first output), so one pixel launch may be followed by several of these.  Lane j computes output column j exactly as
// without a mirror and stores it at column ow - 1 - j.  32 bytes a row: 32 rows and JbResample are 1.1 KB of the 4 KB
// argument segment.
struct JbViewRow {
  int64_t src_offset;     // bytes from the scratch's base to the union's first pixel
  int32_t src_row_bytes;  // 3 * union_w: at most 3 * 65535
  int32_t dx, dy, w, h;   // the view's rectangle inside the union: dx + w <= union_w, dy + h <= union_h
  int32_t mirror;         // 1: store column j at ow - 1 - j
};
struct JbViewTable {
  JbViewRow r[kJbCropsPerLaunch];
};
// jbk_resample_launch_crops with a view per row: p.n_images = the rows of the launch (p.iw, p.ih and p.src_image_stride
// are not looked at).  A source row is read through a descriptor of the UNION's row + 4 bytes: the scratch's slack
// covers the last row of the last union, as it covers the last image's without views.
hipError_t jbk_resample_launch_views(const JbResample &p, const JbViewTable &table, int format, hipStream_t stream);
// The filtered counterpart: a JbFilterRow already separates rectangle, window and offset -- the window is the union (it
// must CONTAIN jb_filter_window of the row's rectangle, where jbk_filter_launch_crops wants exactly that window), and bit
// n of `mirror` is row n's flag.  40 bytes a row and 4 for the flags: 1.4 KB with JbFilter.
struct JbViewFilterTable {
  JbFilterRow r[kJbCropsPerLaunch];
  uint32_t mirror;
};
hipError_t jbk_filter_launch_views(const JbFilter &p, const JbViewFilterTable &table, int filter, int format, hipStream_t stream);

// "View groups" (jb_resample.hip, MODE = kViewGroups): a view launch whose rows are not evenly spaced behind p.dst -- an
// image's block interleaves groups of different sizes, and a launch's 32 rows may start in the middle of an image -- so
// every row carries the place of its output: dst_offset bytes behind p.dst (p.dst_image_stride is not looked at).  Read by
// blockIdx like the rest of the row: scalar loads, wave-uniform.  40 and 48 bytes a row: 1.4 and 1.7 KB with the arguments.
struct JbViewGroupRow {
  JbViewRow v;
  int64_t dst_offset;  // >= 0
};
struct JbViewGroupTable {
  JbViewGroupRow r[kJbCropsPerLaunch];
};
struct JbViewGroupFilterRow {
  JbFilterRow f;
  int64_t dst_offset;  // >= 0
};
struct JbViewGroupFilterTable {
  JbViewGroupFilterRow r[kJbCropsPerLaunch];
  uint32_t mirror;
};
// jbk_resample_launch_views / jbk_filter_launch_views with their validation, and dst_offset >= 0 of every row
hipError_t jbk_resample_launch_view_groups(const JbResample &p, const JbViewGroupTable &table, int format, hipStream_t stream);
hipError_t jbk_filter_launch_view_groups(const JbFilter &p, const JbViewGroupFilterTable &table, int filter, int format, hipStream_t stream);

// "Colour chains" (jb_color.hip; the arithmetic is jb_color_core.h's): up to kJbCropsPerLaunch VIEWS a launch, each a tight
// or strided interleaved uint8 image of w x h at src + src_offset (rows src_row_stride apart), its chain applied and the
// result written in `format` at dst + dst_offset, addressed as JbResample addresses an output.  Chains and offsets travel
// in the arguments: 88 bytes a row, 2.8 KB with JbColor, of the 4 KB argument segment.
struct JbColorRow {
  int64_t src_offset, dst_offset;  // >= 0
  jb_color_chain chain;            // checked by the caller (jb_color_check)
};
struct JbColorTable {
  JbColorRow r[kJbCropsPerLaunch];
};
struct JbColor {
  const uint8_t *src;
  uint8_t *dst;
  int64_t src_row_stride, dst_row_stride, dst_plane_stride;
  unsigned long long *sums;  // device, kJbColorScratchBytes, the launch's alone until it has run: the views' luma sums
                             // (kJbCropsPerLaunch words), then counters and tables (below)
  int32_t w, h;              // each in 1..65535
  int32_t n_views;
  int32_t tiles_x;  // (set by the launch: workgroups per 4 rows)
  float scale[3], bias[3];
};
// Where a chain of the launch has a JB_COLOR_CONTRAST: `sums` zeroed on the stream, then jb_color_mean_kernel (a workgroup
// per 16 rows of a view; integer sums, one 64-bit atomic per workgroup).  Then jb_color_apply_kernel: one workgroup per 256
// columns x 4 rows of a view, a lane per 4 pixels of a row.  Where a chain of the launch has a JB_COLOR_BLUR, then
// jb_color_blur_kernel too: one workgroup per 64 x 32 pixels of a view; the views with a blur are its, the others the apply
// kernel's, and the workgroups of the other kernel's views return at once.  The launch turns each blur's radius into its
// three integers on the host (jbc_blur_weights): 12 bytes a view beside the table, 3.3 KB of arguments in all.  A launch
// without a blur issues what it issued before there was one.  An argument outside its range, a blur in front of a contrast
// or a box radius above JB_COLOR_BLUR_BOX_MAX: hipErrorInvalidValue.
//
// Statistics that are not one number (JB_COLOR_AUTOCONTRAST, JB_COLOR_EQUALIZE): the scratch behind `sums` holds, for every
// view of a launch and each of its JB_COLOR_STATS_MAX statistics operations, 768 uint32 counters (R, G, B histograms) and,
// behind all counters, 768 table bytes: 256 + 32 * 2 * (3072 + 768) = 246,016 bytes.  ROUND k (0, 1) computes the k-th
// statistics operation of every view that has one, with the results of round 0 applied in front of round 1's: the mean kernel
// for a contrast, jb_color_hist_kernel (a workgroup per 32 rows of a view: LDS integer atomics, then one global integer
// atomic per non-empty bin) and jb_color_table_kernel (a workgroup of 256 threads per view: counters -> table) for the two
// table operations.  A round's kernels are launched only when a view of the launch needs them, and the counters are zeroed
// (with the sums, one memset) only in a launch with a table operation.  Where a chain has a JB_COLOR_SHARPNESS,
// jb_color_sharp_kernel (a 64 x 32 tile, halo 1) writes those views; the apply kernel skips them as it skips blur views.  A
// launch whose chains have none of these issues what it issued before: memset, mean, apply, blur.
//
// Geometric operations (JB_COLOR_SHEAR_X .. JB_COLOR_ROTATE): the launch turns each into Pillow's path and six integers on the
// host (jbc_warp_params; the kernels never see a double): 32 bytes an operation, JB_COLOR_WARPS_MAX a view, 2 KB a launch.
// They do NOT travel in the arguments: JbColor + JbColorTable + JbBlurTable are 3.3 KB of the 4 KB segment, and the blur
// kernel of a chain with a geometric operation in front of its blur wants all three.  Fewer views a launch would have kept
// them in the arguments at the price of a second table type and twice the launches of every augmentation batch; instead the
// coefficients lie in the colour scratch BEHIND the tables (kJbColorWarpOffset), written on the stream in front of the
// launch's kernels by jb_color_warp_table_kernel, which gets them as ITS arguments (2 KB), and read from there by view
// (scalar loads: the view is the workgroup's).  Only a launch with a geometric operation writes them, and only such a launch
// runs the kernels' WARP instantiations, whose every pixel load is jbc_gather (jb_color_core.h); a launch without one
// issues the kernels it issued before there were any, with the warp text compiled out.
// A view WITHOUT a geometric operation in a launch WITH one pays for its neighbours: the WARP instantiations gather it with
// byte loads at its own positions, NEW_OPS is forced on, and its blur runs the NEW_OPS variant; measured per 224 x 224 / 96 x 96
// view with the empty chain, one rotation among the launch's 32: 0.18 / 0.27 us over the plain launch's 0.45 / 0.55
// (DESIGN.md 5.25).  Splitting such a launch in two would cost a launch (about 0.3 us a view) for the same views: not done.
constexpr int64_t kJbColorCounterBytes = 768 * 4, kJbColorTableBytes = 768;
constexpr int64_t kJbColorWarpOffset = 8 * kJbCropsPerLaunch + kJbCropsPerLaunch * JB_COLOR_STATS_MAX * (kJbColorCounterBytes + kJbColorTableBytes);
constexpr int64_t kJbColorWarpBytes = kJbCropsPerLaunch * JB_COLOR_WARPS_MAX * 32;
constexpr int64_t kJbColorScratchBytes = kJbColorWarpOffset + kJbColorWarpBytes;
hipError_t jbk_color_launch(const JbColor &p, const JbColorTable &table, int format, hipStream_t stream);

// "Fit" (jb_fit.hip jb_fit_fill_kernel): the border of n_images letterboxed outputs of ow x oh at dst, addressed as
// JbResample addresses them (rows dst_row_stride bytes apart -- of a plane when planar --, planes dst_plane_stride, images
// dst_image_stride).  A band is the rectangle bw x bh at (bx, by) of every output, in elements; bw or bh = 0: no such band.
// Every element of a band gets fill[c] in `format` (scale / bias: the float formats' affine map); nothing else is written.
struct JbFitFill {
  uint8_t *dst;
  int64_t dst_image_stride, dst_row_stride, dst_plane_stride;
  int32_t ow, oh;  // each in 1..65535: what the bands must lie in
  int32_t n_images;
  int32_t bx[2], by[2], bw[2], bh[2];
  int32_t wgs[2];  // (set by the launch: workgroups per band and image)
  float scale[3], bias[3];
  uint8_t fill[3];
};
// one workgroup per 256 elements of a band of one image; no band at all: nothing is launched.  More than 2^31 - 1
// workgroups, or an argument outside its range (a band that leaves the output): hipErrorInvalidValue.
hipError_t jbk_fit_fill_launch(const JbFitFill &p, int format, hipStream_t stream);

// "Orientation" (jb_orient.hip; the arguments are described in jb_orient.h).  One 256-lane workgroup per 64 x 64 tile of
// source pixels.  More than 2^31 - 1 workgroups, or an argument outside its range: hipErrorInvalidValue.
hipError_t jbk_orient_launch(const JbOrient &p, int format, hipStream_t stream);
// format 0, tight, a source and a destination per image (at most kJbCropsPerLaunch images)
hipError_t jbk_orient_launch_table(const JbOrient &p, const JbOrientTable &table, hipStream_t stream);

// Device-side entropy decoder (jb_huff.hip); structures in jb_huff.h.
struct JbHuffLaunch;
hipError_t jbk_huff_launch(const JbHuffLaunch &p, hipStream_t stream);
// small pinned host blob -> device by a kernel (no copy-engine hand-over in front of the decoding kernels);
// bytes is rounded up to 16: both buffers are allocated with that slack
// zero `bytes` (rounded up to 16) of device memory by a kernel
// (d_small / small_bytes: a second region of at most 4 KB, rounded up to 16 bytes, zeroed by the same launch)
hipError_t jbk_huff_zero(void *d_dst, size_t bytes, hipStream_t stream, void *d_small = nullptr, size_t small_bytes = 0);
hipError_t jbk_huff_fetch(void *d_dst, const void *h_pinned_src, size_t bytes, hipStream_t stream);
