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
//
// "Views" (include/jpegblk.h; MODE = kViews of both kernels): an output's source is a w x h sub-rectangle at (dx, dy) of
// a UNION the pixel kernel wrote once for all the views of an image, and a mirrored view stores column j at ow - 1 - j.
// The footprint, the weights and the sums are those of column j -- the bits are defined by the unmirrored output -- so a
// wave's 64 stores are still one contiguous run, walked backwards.  The bodies also compile for the CPU
// (JB_KERNELS_HOST: tools/fuzz/views_kernel_check.cpp stubs the built-ins and runs a workgroup as 256 threads).
#ifndef JB_KERNELS_HOST
#include <hip/hip_runtime.h>
#define JB_DYNAMIC_LDS(name) extern __shared__ int32_t name[]
#endif

#include "jb_kernels.h"
#include "jb_store.h"

// what a kernel's table argument is: none (one geometry for the launch), a rectangle per image, a view per output, a
// view and a destination per output ("view groups", jb_kernels.h)
enum { kNoTable = 0, kCrops = 1, kViews = 2, kViewGroups = 3 };

static constexpr int kResampleRows = 4;  // output rows (= waves) per workgroup

// the rows of a kernel's by-value table argument
static __device__ __forceinline__ const JbCrop *crops_of(const JbCropTable &table) { return table.c; }
static __device__ __forceinline__ const JbViewRow &view_of(const JbViewTable &table, uint32_t row) { return table.r[row]; }
static __device__ __forceinline__ const JbViewRow &view_of(const JbViewGroupTable &table, uint32_t row) { return table.r[row].v; }
static __device__ __forceinline__ int64_t dst_offset_of(const JbViewGroupTable &table, uint32_t row) { return table.r[row].dst_offset; }
static __device__ __forceinline__ int64_t dst_offset_of(const JbViewGroupFilterTable &table, uint32_t row) { return table.r[row].dst_offset; }

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
// VIEWS (TABLE is JbViewTable): `img` is the launch's row = the output's index behind p.dst; its source is the row's
// w x h at (dx, dy) of the union at p.src + .src_offset, rows .src_row_bytes apart, and .mirror reverses the store.
// VIEW GROUPS (TABLE is JbViewGroupTable): VIEWS, and the row's output lies at p.dst + .dst_offset.
template <int FORMAT, int MODE = kNoTable, typename... TABLE>
__global__ __launch_bounds__(64 * kResampleRows) void jb_resample_kernel(const JbResample p, const TABLE... table) {
  constexpr bool CROPS = MODE == kCrops, GROUPS = MODE == kViewGroups, VIEWS = MODE == kViews || GROUPS;
  static_assert(sizeof...(TABLE) == (MODE != kNoTable ? 1 : 0), "the table is the second argument of the CROPS and VIEWS instantiations alone");
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
  // VIEWS: the union's row length, the view's first column in it, and the column this lane stores (else: constants)
  [[maybe_unused]] uint32_t union_row_bytes = 0, dx = 0, js = j;
  if constexpr (VIEWS) {
    const JbViewRow &v = view_of(table..., img);
    iw = (uint32_t)v.w, ih = (uint32_t)v.h;
    union_row_bytes = (uint32_t)v.src_row_bytes, dx = (uint32_t)v.dx;
    src_offset = v.src_offset + (int64_t)v.dy * v.src_row_bytes;
    if (v.mirror) js = ow - 1 - j;
  }

  // the footprints on the common grid: products below 65535^2 < 2^32
  const uint32_t r0 = k * ih / oh, r1 = ((k + 1) * ih - 1) / oh;  // source rows r0..r1, wave-uniform
  const uint32_t i0 = j * iw / ow, i1 = ((j + 1) * iw - 1) / ow;  // source columns i0..i1
  // the first and the last weight of a footprint (every one between them is ow, resp. oh)
  const uint32_t wx0 = min((i0 + 1) * ow, (j + 1) * iw) - j * iw;
  const uint32_t wx1 = (j + 1) * iw - i1 * ow;  // (used when i1 > i0)
  const uint32_t wy0 = min((r0 + 1) * oh, (k + 1) * ih) - k * ih;
  const uint32_t wy1 = (k + 1) * ih - r1 * oh;  // (used when r1 > r0)

  const uint8_t *const src = p.src + (CROPS || VIEWS ? src_offset : (int64_t)img * p.src_image_stride);
  // (VIEWS: the descriptor is the UNION's row + 4 bytes, the view's columns start 3 * dx into it)
  const int64_t src_row_bytes = VIEWS ? (int64_t)union_row_bytes : 3LL * iw;
  const uint32_t i_dx = VIEWS ? dx : 0;
  uint64_t acc[3] = {0, 0, 0};
  for (uint32_t r = r0; r <= r1; r++) {
    const __amdgpu_buffer_rsrc_t row =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src + (int64_t)r * src_row_bytes), 0, (int)((VIEWS ? union_row_bytes : 3 * iw) + 4), 0x00020000);
    // the horizontal partial sum: sum of wx * sample <= 255 * iw < 2^24
    uint32_t px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * (i0 + i_dx)), 0, 0);
    uint32_t h[3] = {wx0 * (px & 0xffu), wx0 * ((px >> 8) & 0xffu), wx0 * ((px >> 16) & 0xffu)};
    if (i1 > i0) {
      uint32_t m[3] = {0, 0, 0};  // the samples of weight ow
      uint32_t i = i0 + 1;
      for (; i + 8 <= i1; i += 8) {  // eight loads in flight: a long footprint is bound by their latency
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * (i + i_dx + u)), 0, 0);
#pragma unroll
        for (int u = 0; u < 8; u++) m[0] += v[u] & 0xffu, m[1] += (v[u] >> 8) & 0xffu, m[2] += (v[u] >> 16) & 0xffu;
      }
      for (; i < i1; i++) {
        px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * (i + i_dx)), 0, 0);
        m[0] += px & 0xffu, m[1] += (px >> 8) & 0xffu, m[2] += (px >> 16) & 0xffu;
      }
      px = __builtin_amdgcn_raw_buffer_load_b32(row, (int)(3 * (i1 + i_dx)), 0, 0);
#pragma unroll
      for (int c = 0; c < 3; c++) h[c] += ow * m[c] + wx1 * ((px >> (8 * c)) & 0xffu);
    }
    const uint32_t wy = r == r0 ? wy0 : r == r1 ? wy1 : oh;
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] += (uint64_t)wy * h[c];
  }

  const uint32_t d = iw * ih;
  const float rcp_d = 1.0f / (float)d;
  int64_t dst_offset = (int64_t)img * p.dst_image_stride;
  if constexpr (GROUPS) dst_offset = dst_offset_of(table..., img);
  uint8_t *const dst = p.dst + dst_offset + (int64_t)k * p.dst_row_stride;
#pragma unroll
  for (int c = 0; c < 3; c++)
    jb_store_element<FORMAT>(dst, p.dst_plane_stride, js, c, div_to_u8(acc[c] + (d >> 1), d, rcp_d), p.scale, p.bias);
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

// ---- the launchers' checks: host code that the CPU programs of tools/fuzz compile and run too -----------------------------
constexpr int kAnyImages = 0x7fffffff;  // max_images of a launch without a table

// the launch-wide ranges: the format, the target, and the images (a table's rows) of the launch
static bool resample_args_ok(const JbResample &p, int format, int max_images) {
  return format >= 0 && format <= 3 && p.ow >= 1 && p.oh >= 1 && p.ow <= 65535 && p.oh <= 65535 && p.n_images >= 1 && p.n_images <= max_images;
}
static bool crop_row_ok(const JbCrop &c) { return c.w >= 1 && c.h >= 1 && c.w <= 65535 && c.h <= 65535 && c.tmp_offset >= 0; }
// (the view lies in its union's row; what the union's rows hold behind it is the seam's business)
static bool view_row_ok(const JbViewRow &v) {
  return v.w >= 1 && v.h >= 1 && v.w <= 65535 && v.h <= 65535 && v.dx >= 0 && v.dy >= 0 && v.dy <= 65535 && v.src_offset >= 0 &&
         v.src_row_bytes <= 3 * 65535 && 3 * ((int64_t)v.dx + v.w) <= v.src_row_bytes && !(v.mirror & ~1);
}
// "view groups", either table: every row's output lies behind p.dst
template <class TABLE>
static bool dst_offsets_ok(const TABLE &table, int n) {
  for (int i = 0; i < n; i++)
    if (table.r[i].dst_offset < 0) return false;
  return true;
}
// the first n rows of a resample launch's table
static bool rows_ok(const JbCropTable &table, int n) {
  for (int i = 0; i < n; i++)
    if (!crop_row_ok(table.c[i])) return false;
  return true;
}
static bool rows_ok(const JbViewTable &table, int n) {
  for (int i = 0; i < n; i++)
    if (!view_row_ok(table.r[i])) return false;
  return true;
}
static bool rows_ok(const JbViewGroupTable &table, int n) {
  for (int i = 0; i < n; i++)
    if (!view_row_ok(table.r[i].v)) return false;
  return dst_offsets_ok(table, n);
}

#ifndef JB_KERNELS_HOST
#include "jb_launch.h"

// grid, block and the dispatch by format of every resample launch
template <int MODE, typename... TABLE>
static hipError_t resample_dispatch(const JbResample &q, int format, hipStream_t stream, const TABLE &...table) {
  JbResample p = q;
  dim3 grid;
  if (!resample_grid(p, &grid)) return hipErrorInvalidValue;
  jb_by_format(format, [&](auto F) {
    hipLaunchKernelGGL((jb_resample_kernel<decltype(F)::value, MODE, TABLE...>), grid, dim3(64 * kResampleRows), 0, stream, p, table...);
  });
  return hipGetLastError();
}
// a launch with a table: at most kJbCropsPerLaunch rows, each in its ranges
template <int MODE, class TABLE>
static hipError_t resample_table_launch(const JbResample &q, const TABLE &table, int format, hipStream_t stream) {
  if (!resample_args_ok(q, format, kJbCropsPerLaunch) || !rows_ok(table, q.n_images)) return hipErrorInvalidValue;
  return resample_dispatch<MODE>(q, format, stream, table);
}

hipError_t jbk_resample_launch_views(const JbResample &q, const JbViewTable &table, int format, hipStream_t stream) {
  return resample_table_launch<kViews>(q, table, format, stream);
}
hipError_t jbk_resample_launch_view_groups(const JbResample &q, const JbViewGroupTable &table, int format, hipStream_t stream) {
  return resample_table_launch<kViewGroups>(q, table, format, stream);
}
hipError_t jbk_resample_launch_crops(const JbResample &q, const JbCropTable &table, int format, hipStream_t stream) {
  return resample_table_launch<kCrops>(q, table, format, stream);
}
hipError_t jbk_resample_launch(const JbResample &q, int format, hipStream_t stream) {
  if (!resample_args_ok(q, format, kAnyImages) || q.iw < 1 || q.ih < 1 || q.iw > 65535 || q.ih > 65535) return hipErrorInvalidValue;
  return resample_dispatch<kNoTable>(q, format, stream);
}
#endif  // JB_KERNELS_HOST

// ---- "resampling filters" (include/jpegblk.h): Pillow's 8-bit bilinear / bicubic resampling, bit for bit ----------------
// Pillow's two passes inside one workgroup.  A workgroup owns 64 output columns x kFilterRows output rows of one image:
//   1. the integer weights of its 64 columns (wave 0, one lane per column) and of its rows (wave 1, one lane per row), in
//      fp64 with jb_filter.h's arithmetic -- each lane loops over its taps in order, so the ww sum is the sequential one
//      -- into LDS.  The column table is tap-major, kx[t][lane]: a wave's read of tap t is 64 consecutive words, no bank
//      conflict; the row table is read wave-uniformly (a broadcast).
//   2. the horizontal pass for every source row the rows' vertical footprints span, the rows dealt round-robin to the
//      four waves: a lane = an output column, a pixel = ONE 4-byte load as in jb_resample_kernel (four in flight), through
//      a descriptor of the source row whose range keeps every load inside the scratch; T (rounded to uint8, as Pillow
//      rounds between the passes) goes to LDS as one word per pixel, T[row][lane]: conflict-free again.
//   3. one barrier, then the vertical pass out of LDS: a wave = output rows wave and wave + 4, so the row, its bounds and
//      its weights stay wave-uniform; the store is jb_resample_kernel's (jb_store.h).
// kFilterRows = 8: the span of source rows is (8 - 1) * scale + taps, so per output row 1080 -> 224 bilinear filters
// 5.6 source rows where the ideal (infinitely many rows per workgroup) is 4.8 and 4 rows per workgroup would be 6.4; 16
// rows would double T and the accumulators for the last 8 %.  When the span is longer than the T rows that fit LDS
// (q.t_rows; long bicubic reductions only) the passes 2 and 3 run chunk by chunk of t_rows source rows, the vertical sums
// staying in registers: T[r] is complete after pass 2 whatever the chunking, and integer addition is associative.
#include "jb_filter.h"

static constexpr int kFilterRows = 8;
static constexpr int kFilterLdsBytes = 64 << 10;  // what one workgroup may have

static __device__ __forceinline__ const JbFilterRow *rows_of(const JbFilterTable &table) { return table.r; }
static __device__ __forceinline__ const JbFilterRow *rows_of(const JbViewFilterTable &table) { return table.r; }
static __device__ __forceinline__ bool mirror_of(const JbViewFilterTable &table, uint32_t row) { return (table.mirror >> row) & 1u; }
static __device__ __forceinline__ bool mirror_of(const JbViewGroupFilterTable &table, uint32_t row) { return (table.mirror >> row) & 1u; }
static __device__ __forceinline__ const JbFilterRow &group_row_of(const JbViewGroupFilterTable &table, uint32_t row) { return table.r[row].f; }
static __device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one lane's weights of output `i` of axis `a` (i < n: else none) into tab[t * stride], t < taps, zero behind its own
// taps; -> its first source sample (`none` without an output); *count: its taps
static __device__ __forceinline__ int filter_weights(const JbFilterAxis &a, int i, int n, int taps, int none, int32_t *tab, int stride,
                                                     int *count) {
  double center = 0.0;
  int lo = none, m = 0;
  if (i < n) {
    int hi;
    jb_filter_bounds(a, i, &center, &lo, &hi);
    m = min(hi - lo, taps);
  }
  double ww = 0.0;
  for (int t = 0; t < m; t++) ww += jb_filter_weight(a, lo, center, t);
  for (int t = 0; t < taps; t++) {
    int32_t k = 0;
    if (t < m) {
      double w = jb_filter_weight(a, lo, center, t);
      if (ww != 0.0) w = w / ww;
      k = jb_filter_fixed(w);
    }
    tab[t * stride] = k;
  }
  *count = m;
  return lo;
}

// VIEWS (TABLE is JbViewFilterTable): `img` is the launch's row = the output's index behind p.dst; the row's window is its
// image's union, which holds the rectangle's own window, and its bit of table.mirror reverses the store.
// VIEW GROUPS (TABLE is JbViewGroupFilterTable): VIEWS, and the row's output lies at p.dst + its dst_offset.
template <int FILTER, int FORMAT, int MODE = kNoTable, typename... TABLE>
__global__ __launch_bounds__(256) void jb_filter_kernel(const JbFilter q, const TABLE... table) {
  constexpr bool CROPS = MODE != kNoTable, GROUPS = MODE == kViewGroups, VIEWS = MODE == kViews || GROUPS;
  static_assert(sizeof...(TABLE) == (CROPS ? 1 : 0), "the table is the second argument of the CROPS and VIEWS instantiations alone");
  JB_DYNAMIC_LDS(filter_lds);
  const JbResample &p = q.base;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t b = blockIdx.x;
  const uint32_t tx = b % (uint32_t)p.tiles_x, t = b / (uint32_t)p.tiles_x;
  const uint32_t ty = t % (uint32_t)p.tiles_y, img = t / (uint32_t)p.tiles_y;
  if (img >= (uint32_t)p.n_images) return;  // (the whole workgroup)
  JbFilterRow g = q.one;
  int64_t src_offset = (int64_t)img * p.src_image_stride;
  if constexpr (CROPS) {  // this image's geometry: scalar loads, wave-uniform
    if constexpr (GROUPS) g = group_row_of(table..., img);
    else g = rows_of(table...)[img];
    src_offset = g.tmp_offset;
  }
  const int ow = p.ow, oh = p.oh;
  const JbFilterAxis ax = jb_filter_axis(FILTER, q.frame_w, g.x, g.x + g.w, ow);
  const JbFilterAxis ay = jb_filter_axis(FILTER, q.frame_h, g.y, g.y + g.h, oh);
  const int taps_x = min(jb_filter_taps(ax), q.tx_cap), taps_y = min(jb_filter_taps(ay), q.ty_cap);

  int32_t *const kx = filter_lds;                            // [tx_cap][64]
  int32_t *const lox = kx + q.tx_cap * 64;                   // [64]: first source column, relative to the window
  int32_t *const ky = lox + 64;                              // [kFilterRows][ty_cap]
  int32_t *const loy = ky + kFilterRows * q.ty_cap;          // [kFilterRows]: first source row, in the frame
  int32_t *const ny = loy + kFilterRows;                     // [kFilterRows]: taps
  uint32_t *const T = (uint32_t *)(ny + kFilterRows);        // [t_rows][64]: r | g << 8 | b << 16

  const int j = (int)tx * 64 + lane;  // output column
  [[maybe_unused]] int js = j;        // the column this lane stores
  if constexpr (VIEWS)
    if (mirror_of(table..., img)) js = ow - 1 - j;
  const int k0 = (int)ty * kFilterRows;
  if (wave == 0) {
    int count;
    lox[lane] = filter_weights(ax, j, ow, taps_x, g.win_x, kx + lane, 64, &count) - g.win_x;
  } else if (wave == 1 && lane < kFilterRows) {
    int count;
    loy[lane] = filter_weights(ay, k0 + lane, oh, taps_y, g.win_y, ky + lane * q.ty_cap, 1, &count);
    ny[lane] = count;
  }
  __syncthreads();

  const int n_rows = min(kFilterRows, oh - k0);  // >= 1
  const int span_lo = __builtin_amdgcn_readfirstlane(loy[0]);
  const int span_hi = __builtin_amdgcn_readfirstlane(loy[n_rows - 1] + ny[n_rows - 1]);
  const int off0 = 3 * lox[lane];
  const uint8_t *const src = p.src + src_offset;
  const int64_t src_row_bytes = 3LL * g.win_w;
  int acc[kFilterRows / 4][3];
#pragma unroll
  for (int i = 0; i < kFilterRows / 4; i++) acc[i][0] = acc[i][1] = acc[i][2] = 1 << 21;

  for (int base = span_lo; base < span_hi; base += q.t_rows) {
    const int end = min(base + q.t_rows, span_hi);
    // the horizontal pass of source rows base .. end - 1
    for (int r = base + wave; r < end; r += 4) {
      const int wr = min(max(r - g.win_y, 0), g.win_h - 1);  // (inside the window by construction)
      const __amdgpu_buffer_rsrc_t row =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src + (int64_t)wr * src_row_bytes), 0, (int)(3 * g.win_w + 4), 0x00020000);
      int h[3] = {1 << 21, 1 << 21, 1 << 21};
      int tap = 0;
      for (; tap + 4 <= taps_x; tap += 4) {  // four loads in flight
        uint32_t v[4];
        int32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b32(row, off0 + 3 * (tap + u), 0, 0);
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = kx[(tap + u) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 4; u++)
          h[0] += w[u] * (int)(v[u] & 0xffu), h[1] += w[u] * (int)((v[u] >> 8) & 0xffu), h[2] += w[u] * (int)((v[u] >> 16) & 0xffu);
      }
      for (; tap < taps_x; tap++) {
        const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(row, off0 + 3 * tap, 0, 0);
        const int32_t w = kx[tap * 64 + lane];
        h[0] += w * (int)(v & 0xffu), h[1] += w * (int)((v >> 8) & 0xffu), h[2] += w * (int)((v >> 16) & 0xffu);
      }
      T[(r - base) * 64 + lane] = (uint32_t)clip8(h[0] >> 22) | (uint32_t)clip8(h[1] >> 22) << 8 | (uint32_t)clip8(h[2] >> 22) << 16;
    }
    __syncthreads();
    // the vertical pass over what of this chunk lies in each row's footprint
#pragma unroll
    for (int i = 0; i < kFilterRows / 4; i++) {
      const int s = wave + 4 * i;
      if (s < n_rows) {
        const int lo = __builtin_amdgcn_readfirstlane(loy[s]), n = __builtin_amdgcn_readfirstlane(ny[s]);
        const int r1 = min(lo + n, end);
        for (int r = max(lo, base); r < r1; r++) {
          const int32_t w = ky[s * q.ty_cap + (r - lo)];
          const uint32_t v = T[(r - base) * 64 + lane];
          acc[i][0] += w * (int)(v & 0xffu), acc[i][1] += w * (int)((v >> 8) & 0xffu), acc[i][2] += w * (int)((v >> 16) & 0xffu);
        }
      }
    }
    if (end < span_hi) __syncthreads();  // (T is written again)
  }

  if (j >= ow) return;
#pragma unroll
  for (int i = 0; i < kFilterRows / 4; i++) {
    const int s = wave + 4 * i;
    if (s >= n_rows) continue;
    int64_t dst_offset = (int64_t)img * p.dst_image_stride;
    if constexpr (GROUPS) dst_offset = dst_offset_of(table..., img);
    uint8_t *const dst = p.dst + dst_offset + (int64_t)(k0 + s) * p.dst_row_stride;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const uint32_t u = (uint32_t)clip8(acc[i][c] >> 22);
      jb_store_element<FORMAT>(dst, p.dst_plane_stride, js, c, u, p.scale, p.bias);
    }
  }
}

// the launch's grid and LDS: tx_cap / ty_cap / t_rows from the geometry of its n rows; 0 bytes: not launchable
// (contains: a window may be larger than jb_filter_window of its rectangle -- the views' unions)
static size_t filter_plan(JbFilter &p, const JbFilterRow *rows, int n, int filter, dim3 *grid, bool contains = false) {
  if (filter != 1 && filter != 2) return 0;
  if (p.base.ow < 1 || p.base.oh < 1 || p.base.ow > 65535 || p.base.oh > 65535 || p.base.n_images < 1 || p.frame_w < 1 || p.frame_h < 1 ||
      p.frame_w > 65535 || p.frame_h > 65535)
    return 0;
  p.tx_cap = p.ty_cap = 1;
  int span = 1;
  for (int i = 0; i < n; i++) {
    const JbFilterRow &r = rows[i];
    if (r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0 || r.x + (int64_t)r.w > p.frame_w || r.y + (int64_t)r.h > p.frame_h || r.tmp_offset < 0) return 0;
    // the window must be the one the kernel's bounds stay in: what jb_filter_window gives
    const JbFilterAxis ax = jb_filter_axis(filter, p.frame_w, r.x, r.x + r.w, p.base.ow), ay = jb_filter_axis(filter, p.frame_h, r.y, r.y + r.h, p.base.oh);
    int x0, x1, y0, y1;
    jb_filter_span(ax, p.base.ow, &x0, &x1);
    jb_filter_span(ay, p.base.oh, &y0, &y1);
    if (contains) {
      if (r.win_x < 0 || r.win_y < 0 || r.win_w < 1 || r.win_h < 1 || r.win_x > x0 || r.win_y > y0 || r.win_x + (int64_t)r.win_w < x1 ||
          r.win_y + (int64_t)r.win_h < y1 || r.win_x + (int64_t)r.win_w > p.frame_w || r.win_y + (int64_t)r.win_h > p.frame_h)
        return 0;
    } else if (r.win_x != x0 || r.win_y != y0 || r.win_w != x1 - x0 || r.win_h != y1 - y0) {
      return 0;
    }
    const int tx = jb_filter_taps(ax), ty = jb_filter_taps(ay);
    if (tx > kJbFilterMaxTaps || ty > kJbFilterMaxTaps) return 0;
    if (tx > p.tx_cap) p.tx_cap = tx;
    if (ty > p.ty_cap) p.ty_cap = ty;
    int s = (int)((kFilterRows - 1) * ay.scale) + ty + 2;  // the source rows kFilterRows footprints span, at the most
    if (s > r.win_h) s = r.win_h;
    if (s > span) span = s;
  }
  const size_t fixed = ((size_t)p.tx_cap * 64 + 64 + (size_t)kFilterRows * p.ty_cap + 2 * kFilterRows) * 4;
  const size_t room = ((size_t)kFilterLdsBytes - fixed) / 256;  // (at the cap: 74 rows)
  p.t_rows = (int)((size_t)span < room ? (size_t)span : room);
  p.base.tiles_x = (p.base.ow + 63) / 64;
  p.base.tiles_y = (p.base.oh + kFilterRows - 1) / kFilterRows;
  const int64_t n_wgs = (int64_t)p.base.tiles_x * p.base.tiles_y * p.base.n_images;
  if (n_wgs > 0x7fffffffLL) return 0;
  *grid = dim3((unsigned)n_wgs);
  return fixed + (size_t)p.t_rows * 256;
}

#ifndef JB_KERNELS_HOST
// the filter 1 / 2 choice and the dispatch by format of every filtered launch (p, lds, grid: filter_plan's)
template <int MODE, typename... TABLE>
static hipError_t filter_dispatch(const JbFilter &p, int filter, int format, size_t lds, dim3 grid, hipStream_t stream, const TABLE &...table) {
  const auto launch = [&](auto FILTER) {
    jb_by_format(format, [&](auto F) {
      hipLaunchKernelGGL((jb_filter_kernel<decltype(FILTER)::value, decltype(F)::value, MODE, TABLE...>), grid, dim3(256), lds, stream, p, table...);
    });
  };
  if (filter == 1) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
  return hipGetLastError();
}
// a filtered launch: the launch-wide ranges, filter_plan over `rows` (null: the launch's one geometry, q.one), the dispatch
template <int MODE, typename... TABLE>
static hipError_t filter_launch(const JbFilter &q, const JbFilterRow *rows, bool contains, int filter, int format, hipStream_t stream,
                                const TABLE &...table) {
  if (!resample_args_ok(q.base, format, rows ? kJbCropsPerLaunch : kAnyImages)) return hipErrorInvalidValue;
  JbFilter p = q;
  dim3 grid;
  const size_t lds = filter_plan(p, rows ? rows : &p.one, rows ? p.base.n_images : 1, filter, &grid, contains);
  if (!lds) return hipErrorInvalidValue;
  return filter_dispatch<MODE>(p, filter, format, lds, grid, stream, table...);
}

hipError_t jbk_filter_launch(const JbFilter &q, int filter, int format, hipStream_t stream) {
  return filter_launch<kNoTable>(q, nullptr, false, filter, format, stream);
}
hipError_t jbk_filter_launch_crops(const JbFilter &q, const JbFilterTable &table, int filter, int format, hipStream_t stream) {
  return filter_launch<kCrops>(q, table.r, false, filter, format, stream, table);
}
hipError_t jbk_filter_launch_views(const JbFilter &q, const JbViewFilterTable &table, int filter, int format, hipStream_t stream) {
  return filter_launch<kViews>(q, table.r, true, filter, format, stream, table);
}
hipError_t jbk_filter_launch_view_groups(const JbFilter &q, const JbViewGroupFilterTable &table, int filter, int format, hipStream_t stream) {
  if (q.base.n_images < 1 || q.base.n_images > kJbCropsPerLaunch || !dst_offsets_ok(table, q.base.n_images)) return hipErrorInvalidValue;
  JbFilterRow rows[kJbCropsPerLaunch];  // (filter_plan takes the rows without their offsets)
  for (int i = 0; i < q.base.n_images; i++) rows[i] = table.r[i].f;
  return filter_launch<kViewGroups>(q, rows, true, filter, format, stream, table);
}
#endif  // JB_KERNELS_HOST
