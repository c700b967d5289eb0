// jb_seam.cpp -- the pixel launch of every route: the public device seams (jb_blocks_to_rgb_device*) and, through
// seam_launch (jb_ctx.h), the staging ring's submissions of jb_api.cpp.
#include <cstring>
#include <vector>

#include "jb_ctx.h"
#include "jb_kernels.h"

namespace {

// Launches of up to this many 192 / 256-lane workgroups per CU take the small-grid kernels when
// JPEGBLK_SMALL_GRID is unset.  Measured on one box, cold, events around every launch, the kernels interleaved
// (profiles/r03/probe_small_grid.json).  4:4:4: one 1080p image (507 workgroups) 12.1 -> 10.2 us, two (1,014)
// 14.6 -> 13.6, four (2,028) 21.5 -> 20.5, one 1280x720 9.4 -> 8.4, one 640x360 9.4 -> 7.1, one 4096x4096 (4,096)
// 33.6 = 33.9.  4:2:0: one 640x360 11.3 -> 7.8 us, one 1080p (255 workgroups) 12.2 -> 9.4, four (1,020) 17.3 -> 15.6,
// eight (2,040) 28.0 -> 25.7, one 4096x4096 (2,048: BASELINE config 3) 27.5 -> 25.6, two (4,096) 44.6 -> 43.1.
// 4:2:2 / 4:4:0 (all 64 lanes busy): one 1080p 11.2 -> 10.6 / 11.4 -> 9.6 us, one 4096x4096 25.0 -> 23.4 / 25.7 -> 26.3.
constexpr int kSmallGridBelowPerCu = 8;

// The pixel launch of every route -- the public device seams below and the staging ring's submissions -- in three
// steps: argument validation, tile planning, the launch.  `plan` (jb_plan.h) says what the pixels look like: scale 1,
// format 0 is exactly the launch jb_blocks_to_rgb_device has always made; scale 2, 4, 8 the row-bound tiling with the
// area-reduced store stage; a planar format the row-bound tiling with the planar store stage; a rectangle (plan.has_roi)
// the row-bound tiling over the MCUs it touches with the ROI store stage, in any format.  The batch's row / image
// strides describe the output: the reduced image when scale > 1, one plane's rows with a planar format, images of the
// rectangle's size with a rectangle (plan.out_w x plan.out_h in every case).

// 1. validation: the batch against the plan; g: the frame's geometry; plane_stride: bytes between the planes (0: interleaved)
int seam_check(jb_ctx *ctx, const jb_device_batch *b, const JbOutPlan &plan, const char *fn, jb_geometry *g, int64_t *plane_stride) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "%s: ctx is NULL", fn);
  if (!b || !b->d_coef || !b->d_qtabs || !b->d_rgb) return fail(ctx, JB_ERR_NULL, "%s: NULL pointer", fn);
  int rc = check_desc(ctx, &b->desc, g);
  if (rc) return rc;
  if (b->n_images < 1) return fail(ctx, JB_ERR_GEOMETRY, "n_images = %d", b->n_images);
  // "draft decode": the plan is the draft frame's, which exists only where the draft goes with everything else
  if (const char *why = jb_draft_refusal_(ctx->draft, ctx->arithmetic, plan.scale ? plan.scale : 1, plan.orient == JB_ORIENT_STORED ? ctx->orientation : plan.orient))
    return fail(ctx, JB_ERR_UNSUPPORTED, "%s: %s", fn, why);
  if (plan.status != JB_OK) return fail(ctx, plan.status, "%s: %s", fn, plan.why);
  if (ctx->arithmetic == JB_ARITH_LIBJPEG && plan.scale != 1) return fail(ctx, JB_ERR_UNSUPPORTED, "%s: %s", fn, kJbArithScaleText);
  if (plan.orient == JB_ORIENT_EXIF) return fail(ctx, JB_ERR_STATE, "%s: %s", fn, kJbOrientExifText);
  *plane_stride = 0;
  if (plan.planar) {
    if (jb_output_spec_check(&plan.spec, plan.out_h, b->rgb_row_stride) != JB_OK)
      return fail(ctx, JB_ERR_GEOMETRY, "%s: bad output spec (reserved, plane_stride < row stride * height, or scale / bias not finite)", fn);
    *plane_stride = plan.spec.plane_stride ? plan.spec.plane_stride : b->rgb_row_stride * (int64_t)plan.out_h;
  }
  if (b->rgb_row_stride < plan.row_stride)
    return fail(ctx, JB_ERR_GEOMETRY, "rgb_row_stride %lld < %s", (long long)b->rgb_row_stride, plan.planar ? "width * element size" : "3*width");
  if (plan.planar) {
    if (((uintptr_t)b->d_rgb | (uint64_t)b->rgb_row_stride | (uint64_t)*plane_stride | (uint64_t)(b->n_images > 1 ? b->rgb_image_stride : 0)) & (uint64_t)(plan.esize - 1))
      return fail(ctx, JB_ERR_GEOMETRY, "%s: f32 / f16 output wants the pointer and every stride to be multiples of the element size", fn);
    if (b->n_images > 1 && b->rgb_image_stride < 2 * *plane_stride + b->rgb_row_stride * (int64_t)plan.out_h)
      return fail(ctx, JB_ERR_GEOMETRY, "image strides smaller than one image");
  }
  if (((uintptr_t)b->d_coef & 15) || (b->coef_image_stride & 15))
    return fail(ctx, JB_ERR_GEOMETRY, "coefficient pointer and image stride must be multiples of 16 bytes");
  if (((uintptr_t)b->d_qtabs & 3) || (b->qtab_image_stride & 3))
    return fail(ctx, JB_ERR_GEOMETRY, "quant-table pointer and stride must be multiples of 4 bytes");
  if (b->n_images > 1 && (b->coef_image_stride < g->coef_bytes || b->rgb_image_stride < b->rgb_row_stride * (int64_t)plan.out_h))
    return fail(ctx, JB_ERR_GEOMETRY, "image strides smaller than one image");
  return JB_OK;
}

// 2. tile planning: linear, row-bound or small-grid, and the store-stage knobs, into p (its pointers, strides and
// frame fields are set)
int seam_tiles(jb_ctx *ctx, const jb_device_batch *b, const jb_geometry &g, const JbOutPlan &plan, JbLaunch &p) {
  const int per_tile = jbk_mcus_per_tile(b->desc.hs, b->desc.vs);
  if (plan.has_roi) {
    // only the MCUs the rectangle touches: the grid's origin is the MCU that holds its first pixel, one tile row per
    // touched MCU row, row-bound tiles from the origin's column on (always the 192-lane kernel's ROI instantiation)
    const int mw = 8 * b->desc.hs, mh = 8 * b->desc.vs;
    const jb_roi &r = plan.roi;
    p.roi = 1;
    p.roi_x = r.x, p.roi_y = r.y, p.roi_w = r.width, p.roi_h = r.height;
    p.roi_mx = r.x / mw, p.roi_my = r.y / mh;
    const int roi_mcus_x = (r.x + r.width - 1) / mw - p.roi_mx + 1, roi_mcus_y = (r.y + r.height - 1) / mh - p.roi_my + 1;
    p.tiles_per_row = (roi_mcus_x + per_tile - 1) / per_tile;
    p.tiles_per_image = roi_mcus_y * p.tiles_per_row;  // (at most the whole image's: no overflow)
    const int64_t n_tiles = (int64_t)b->n_images * p.tiles_per_image;
    if (n_tiles > 0x7fffffffLL) return fail(ctx, JB_ERR_CAPACITY, "batch too large for one launch (%lld tiles)", (long long)n_tiles);
    p.n_tiles = (int32_t)n_tiles;
    p.fast_store = 1;  // (the ROI stage does not look at it)
    return JB_OK;
  }
  p.tiles_per_row = (g.mcus_x + per_tile - 1) / per_tile;
  // JPEGBLK_ROW_TILING=1 (debug / A-B knob) forces the row-bound tiling; the scaled and planar stages only exist in it
  const bool force_row = ctx->knobs.row_tiling || plan.scale > 1 || plan.planar;
  // linear tiling only where the row-bound one would leave ragged tiles
  p.linear = (force_row || g.mcus_x % per_tile == 0) ? 0 : jbk_linear_ok(b->desc.hs, b->desc.vs, g.mcus_x);
  const int64_t tiles_per_image = p.linear ? ((int64_t)g.mcus_x * g.mcus_y + per_tile - 1) / per_tile
                                           : (int64_t)g.mcus_y * p.tiles_per_row;
  if (tiles_per_image > 0x7fffffffLL) return fail(ctx, JB_ERR_CAPACITY, "image too large");
  p.tiles_per_image = (int32_t)tiles_per_image;
  const int64_t n_tiles = (int64_t)b->n_images * tiles_per_image;
  if (n_tiles > 0x7fffffffLL) return fail(ctx, JB_ERR_CAPACITY, "batch too large for one launch (%lld tiles)", (long long)n_tiles);
  p.n_tiles = (int32_t)n_tiles;
  // Small launches (a single 1080p image is 507 / 255 workgroups on 256 CUs): four times as many one-wave
  // workgroups (jb_kernels.hip jb_small_kernel_*), row-bound.  JPEGBLK_SMALL_GRID = 1 / 0 forces / forbids it; so does
  // JPEGBLK_ROW_TILING=1 (that knob asks for the 192-lane kernel's row-bound instantiation).  (The scaled and planar
  // stages have no small-grid variant.)
  if (jbk_small_mcus(b->desc.hs, b->desc.vs) > 0 && !force_row && b->rgb_row_stride < (1LL << 26) &&  // (the lane's row offset is 32-bit)
      (ctx->knobs.small_grid == 1 || (ctx->knobs.small_grid < 0 && n_tiles <= (int64_t)kSmallGridBelowPerCu * ctx->n_cus))) {
    const int per = jbk_small_mcus(b->desc.hs, b->desc.vs);
    p.tiles_per_row = (g.mcus_x + per - 1) / per;
    const int64_t small_tiles = (int64_t)b->n_images * g.mcus_y * p.tiles_per_row;
    if (small_tiles <= 0x7fffffffLL) {
      p.linear = 0;
      p.small_grid = 1;
      p.tiles_per_image = (int32_t)((int64_t)g.mcus_y * p.tiles_per_row);
      p.n_tiles = (int32_t)small_tiles;
    } else {
      p.tiles_per_row = (g.mcus_x + per_tile - 1) / per_tile;
    }
  }
  // 12-byte stores at any byte address: gfx950 under ROCm runs with unaligned global/buffer access
  // enabled, and odd widths with tightly packed rows (row stride 3*W) are the common case --
  // measured 1.67x faster than byte stores on 679x451 (tests/test_gpu_parity.py covers both).
  // JPEGBLK_BYTE_STORE=1 forces the byte-store path (test / A-B knob; the scaled stage ignores it).
  p.fast_store = ctx->knobs.byte_store ? 0 : 1;
  // (measurement builds of jb_kernels.hip only -- tools/build_variant.sh -DJB_LAB: the staged store stage of the linear
  // tiling; the product's kernels ignore the field)
  p.staged = (p.linear && p.fast_store && !p.small_grid && ctx->knobs.staged_store == 1) ? 1 : 0;
  return JB_OK;
}

// "draft decode": the batch as plans, windows, the resample and filter launches and the pixel kernel's frame fields see
// it -- with the context's DRAFT FRAME; the coefficients keep b's own descriptor and geometry.  Draft 1: b.
jb_device_batch frame_batch(const jb_ctx *ctx, const jb_device_batch *b) {
  jb_device_batch fb = *b;
  fb.desc = jb_draft_desc_(&b->desc, ctx->draft);
  return fb;
}

// the launch's pointers, strides and frame fields (everything but the tiling and the store-stage knobs); b: with the
// frame the pixels are those of (frame_batch)
JbLaunch launch_base(const jb_device_batch *b, const jb_geometry &g) {
  JbLaunch p;
  memset(&p, 0, sizeof p);
  p.coef = b->d_coef;
  p.qtabs = b->d_qtabs;
  p.rgb = b->d_rgb;
  p.coef_image_stride = b->coef_image_stride;
  p.qtab_image_stride = b->qtab_image_stride;
  p.rgb_image_stride = b->rgb_image_stride;
  p.rgb_row_stride = b->rgb_row_stride;
  p.width = b->desc.width;
  p.height = b->desc.height;
  p.mcus_x = g.mcus_x;
  p.mcus_y = g.mcus_y;
  p.chroma_q_equal = (b->desc.qtab_id[1] == b->desc.qtab_id[2]) ? 1 : 0;
  return p;
}

constexpr size_t kTmpSlack = 16;    // bytes behind the last intermediate (jb_resample_kernel reads pixels as 4-byte words)
constexpr size_t kTmpStreams = 64;  // scratches a context keeps before it lets go of all of them

// the scratch of `stream` in `pool` (ctx->tmp: the resized routes' intermediates; ctx->planes: the planes of
// JB_ARITH_LIBJPEG), at least `bytes` large
int scratch_for_stream(jb_ctx *ctx, std::map<hipStream_t, jb_ctx::Tmp> &pool, hipStream_t stream, size_t bytes, void **out) {
  std::lock_guard<std::mutex> lk(ctx->tmp_mu);
  if (pool.size() >= kTmpStreams && !pool.count(stream)) {
    // a caller that keeps coming with new streams: nothing of the old ones may be in flight when their scratch goes
    JB_HIP(ctx, hipDeviceSynchronize());
    for (auto &kv : pool)
      if (kv.second.d) (void)hipFree(kv.second.d);
    pool.clear();
  }
  jb_ctx::Tmp &t = pool[stream];
  if (t.cap < bytes) {
    if (t.d) {
      JB_HIP(ctx, hipStreamSynchronize(stream));  // the launches that still read the old one
      (void)hipFree(t.d);
      t.d = nullptr, t.cap = 0;
    }
    JB_HIP(ctx, hipMalloc(&t.d, bytes));
    t.cap = bytes;
  }
  *out = t.d;
  return JB_OK;
}
int tmp_for_stream(jb_ctx *ctx, hipStream_t stream, size_t bytes, void **out) { return scratch_for_stream(ctx, ctx->tmp, stream, bytes, out); }

// the MCU window (jb_kernels.h) of a rectangle of the batch's frame under JB_ARITH_LIBJPEG: what its planes take
JbLjWindow lj_window(const jb_ctx *ctx, const jb_device_batch *b, const jb_geometry &g, const jb_roi &r) {
  return jbk_lj_window(b->desc.hs, b->desc.vs, ctx->draft, g.mcus_x, g.mcus_y, r.x, r.y, r.width, r.height);
}

// "fit": the resample and filter kernels produce plan.inner of every output -- its size is their ow x oh, and dst is moved
// to its first element (their stores address element-wise through the strides, which stay the output's).  Without a
// JB_FIT_PAD the inner rectangle is the whole output.
int64_t inner_offset(const jb_device_batch *b, const JbOutPlan &plan) {
  return (int64_t)plan.inner.y * b->rgb_row_stride + (int64_t)plan.inner.x * (plan.planar ? plan.esize : 3);
}

// JB_FIT_PAD: the border of images i0 .. i0 + m - 1 (a call's launch: all of them) -- every element of the outputs outside plan.inner -- in one launch
// (jb_fit.hip).  Only one axis pads, so there are at most two bands.
JbFitFill fill_args(const jb_device_batch *b, const JbOutPlan &plan, int64_t plane_stride, int64_t i0, int m) {
  const int64_t rgb_step = b->n_images > 1 ? b->rgb_image_stride : 0;
  const jb_roi &in = plan.inner;
  JbFitFill f;
  memset(&f, 0, sizeof f);
  f.dst = b->d_rgb + i0 * rgb_step;
  f.dst_image_stride = rgb_step;
  f.dst_row_stride = b->rgb_row_stride;
  f.dst_plane_stride = plane_stride;
  f.ow = plan.out_w, f.oh = plan.out_h;
  f.n_images = m;
  if (in.width < plan.out_w) {  // left and right, the full height
    f.bx[0] = 0, f.bw[0] = in.x, f.bx[1] = in.x + in.width, f.bw[1] = plan.out_w - in.x - in.width;
    f.by[0] = f.by[1] = 0, f.bh[0] = f.bh[1] = plan.out_h;
  } else {  // top and bottom, the full width (none when the inner rectangle is the output)
    f.by[0] = 0, f.bh[0] = in.y, f.by[1] = in.y + in.height, f.bh[1] = plan.out_h - in.y - in.height;
    f.bx[0] = f.bx[1] = 0, f.bw[0] = f.bw[1] = plan.out_w;
  }
  for (int c = 0; c < 3; c++) f.scale[c] = plan.spec.scale[c], f.bias[c] = plan.spec.bias[c], f.fill[c] = plan.fill[c];
  return f;
}
// false: the border of n_images outputs wants more workgroups than a launch takes
bool fill_fits(const JbOutPlan &plan, int64_t n_images) {
  if (plan.fit_mode != JB_FIT_PAD) return true;
  const int64_t border = (int64_t)plan.out_w * plan.out_h - (int64_t)plan.inner.width * plan.inner.height;
  return (border / 256 + 2) * n_images <= 0x7fffffffLL;  // (two bands, each rounded up to whole workgroups)
}

// the resample launch of a sub-batch of m images from image i0 on; src: the scratch
JbResample resample_args(const jb_device_batch *b, const JbOutPlan &plan, int64_t plane_stride, const void *src, int64_t i0, int m) {
  const int64_t rgb_step = b->n_images > 1 ? b->rgb_image_stride : 0;
  JbResample q;
  memset(&q, 0, sizeof q);
  q.src = (const uint8_t *)src;
  q.src_image_stride = plan.tmp_image_bytes;
  q.dst = b->d_rgb + i0 * rgb_step + inner_offset(b, plan);
  q.dst_image_stride = rgb_step;
  q.dst_row_stride = b->rgb_row_stride;
  q.dst_plane_stride = plane_stride;
  q.iw = plan.src_w, q.ih = plan.src_h, q.ow = plan.inner.width, q.oh = plan.inner.height;
  q.n_images = m;
  for (int c = 0; c < 3; c++) q.scale[c] = plan.spec.scale[c], q.bias[c] = plan.spec.bias[c];
  return q;
}

// the filtered launch's arguments ("resampling filters"): the resample launch's and the frame
JbFilter filter_args(const jb_device_batch *b, const JbOutPlan &plan, int64_t plane_stride, const void *src, int64_t i0, int m) {
  JbFilter f;
  memset(&f, 0, sizeof f);
  f.base = resample_args(b, plan, plane_stride, src, i0, m);
  f.frame_w = b->desc.width, f.frame_h = b->desc.height;
  return f;
}

// a rectangle and its window as the filtered kernels take them
JbFilterRow filter_row(const jb_roi &r, const jb_roi &win, int64_t tmp_offset) {
  return JbFilterRow{r.x, r.y, r.width, r.height, win.x, win.y, win.width, win.height, tmp_offset};
}

// images i0 .. i0 + m - 1 of b -- the coefficient and table pointers advanced -- written to d_rgb with the given strides
// (the strides between b's images are checked, and meaningful, only when there is more than one)
jb_device_batch sub_batch(const jb_device_batch *b, int64_t i0, int m, uint8_t *d_rgb, int64_t row_stride, int64_t image_stride) {
  const int64_t coef_step = b->n_images > 1 ? b->coef_image_stride : 0;
  jb_device_batch ib = *b;
  ib.n_images = m;
  ib.d_coef = (const int16_t *)((const uint8_t *)b->d_coef + i0 * coef_step);
  ib.coef_image_stride = coef_step;
  ib.d_qtabs = (const int32_t *)((const uint8_t *)b->d_qtabs + i0 * b->qtab_image_stride);
  ib.d_rgb = d_rgb;
  ib.rgb_row_stride = row_stride, ib.rgb_image_stride = image_stride;
  return ib;
}

// 3b's and 3e's second half: the filter or resample launch of a sub-batch of whole images -- i0 .. i0 + m - 1 of fb, the
// batch with the frame the plan was made for, their sources tight at src -- into the caller's buffer
int whole_images_tail(jb_ctx *ctx, const jb_device_batch *fb, const JbOutPlan &plan, int64_t plane_stride, const void *src, int64_t i0, int m,
                      hipStream_t s) {
  if (plan.filter) {
    JbFilter f = filter_args(fb, plan, plane_stride, src, i0, m);
    const jb_roi whole = {0, 0, fb->desc.width, fb->desc.height};
    f.one = filter_row(plan.has_roi ? plan.roi : whole, plan.window, 0);
    JB_HIP(ctx, jbk_filter_launch(f, plan.filter, plan.format, s));
  } else {
    JB_HIP(ctx, jbk_resample_launch(resample_args(fb, plan, plane_stride, src, i0, m), plan.format, s));
  }
  return JB_OK;
}

// "orientation": the batch as the resample and filter launches see it -- the oriented frame (of the draft frame: the two
// never come together, seam_check has refused); everything else is b's
jb_device_batch oriented_batch(const jb_ctx *ctx, const jb_device_batch *b, int orientation) {
  jb_device_batch ob = frame_batch(ctx, b);
  if (jb_orient_bits(orientation).transpose) ob.desc.width = b->desc.height, ob.desc.height = b->desc.width;
  return ob;
}
// the rectangle of b's stored frame that shows as `r` of the oriented one (r lies in it: the plan has checked)
jb_roi stored_rect(const jb_device_batch *b, int orientation, const jb_roi &r) {
  jb_roi st = r;
  (void)jb_orient_map_roi(b->desc.width, b->desc.height, orientation, &r, &st);
  return st;
}

// 3c. a plan with per-image rectangles (plan.crops) and a target size: as 3b, with the rectangles of a sub-batch in a
// table that travels in the arguments of both kernels.  Consecutive images are packed into a sub-batch while their
// intermediates -- back to back, tight, at the prefix sums of 3 * w_i * h_i -- fit the cap of the stream's scratch (an
// image larger than the cap runs alone) and a table holds them.  With a filter other than 0 the pixel kernel writes every
// image's WINDOW (jb_filter_window) in its rectangle's place -- the window's size decides the packing -- and the filtered
// kernel gets rectangle and window in a table of its own.  The pixel kernel's grid gives every image as many
// workgroups as the sub-batch's largest rectangle needs; those beyond an image's own count return at once.
//
// The first half, shared with "views" (3f): the rectangle shown[i] of every image i -- in ORIENTED coordinates -- into the
// stream's scratch, sub-batch by sub-batch, under the context's arithmetic and the plan's orientation.  After the pixel
// (and orient) launches of a sub-batch, tail(i0, m, table, src) makes the launches that read it: images i0 .. i0 + m - 1,
// image i0 + j's shown[] rectangle as tight rows of table.c[j].w x .h at src + table.c[j].tmp_offset.
// "Colour chains": stage_per_image > 0 asks for one more region of the same scratch -- that many bytes for every image of a
// sub-batch, counted towards the cap when images are packed, and the scratch of a colour launch (its 32 sum words, and the
// counters and tables of its histogram operations: kJbColorScratchBytes, about 240 KB) in front of it --
// which the tail gets as `stage`; 0: the scratch and the packing are what they are without the parameter.
struct ColorStage {
  uint8_t *bytes = nullptr;            // m * stage_per_image bytes (and the slack of the scratch behind them)
  unsigned long long *sums = nullptr;  // kJbColorScratchBytes: kJbCropsPerLaunch words, then the counters and the tables
};
constexpr int64_t kColorSumsBytes = kJbColorScratchBytes;
static_assert(kColorSumsBytes % 256 == 0, "the staged outputs behind the colour scratch stay aligned");
template <class Tail>
int rects_into_scratch(jb_ctx *ctx, const jb_device_batch *b, void *stream, int orient, const jb_roi *shown, const jb_geometry &g,
                       int64_t stage_per_image, Tail tail) {
  const int64_t cap = (int64_t)ctx->knobs.resize_tmp_bytes;
  // "orientation": the rectangles are the oriented frame's; the pixel kernel writes each one's rectangle of the STORED
  // frame, jb_orient_kernel turns it into a second region of the scratch
  const bool oriented = orient != JB_ORIENT_STORED;
  std::vector<jb_roi> stored;
  if (oriented)
    for (int64_t i = 0; i < b->n_images; i++) stored.push_back(stored_rect(b, orient, shown[i]));
  const jb_roi *const written = oriented ? stored.data() : shown;
  const auto image_bytes = [&](int64_t i) { return 3LL * written[i].width * written[i].height; };
  const auto bytes_of = [&](int64_t i) { return image_bytes(i) * (oriented ? 2 : 1); };  // (the cap counts both regions)
  // JB_ARITH_LIBJPEG: the planes of every image's window are held to the same cap, in a scratch of their own
  const bool lj = ctx->arithmetic == JB_ARITH_LIBJPEG;
  const auto planes_of = [&](int64_t i) { return lj ? lj_window(ctx, b, g, written[i]).bytes : 0; };
  // the images of the sub-batch that starts at i0; *bytes: their intermediates; *planes: their planes
  const auto pack = [&](int64_t i0, int64_t *bytes, int64_t *planes) {
    int m = 1;
    *bytes = bytes_of(i0), *planes = planes_of(i0);
    while (i0 + m < b->n_images && m < kJbCropsPerLaunch && *bytes + bytes_of(i0 + m) + (m + 1) * stage_per_image <= cap &&
           *planes + planes_of(i0 + m) <= cap)
      *bytes += bytes_of(i0 + m), *planes += planes_of(i0 + m), m++;
    return m;
  };
  int64_t most = 0, most_planes = 0;  // the largest sub-batch: what the scratches must hold
  int most_images = 0;
  for (int64_t i0 = 0; i0 < b->n_images;) {
    int64_t bytes, planes;
    const int m = pack(i0, &bytes, &planes);
    i0 += m;
    if (m > most_images) most_images = m;
    if (bytes > most) most = bytes;
    if (planes > most_planes) most_planes = planes;
  }
  DeviceGuard guard(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  void *tmp = nullptr, *planes_d = nullptr;
  // (oriented: `most` counts both regions; the second one starts where the first one and its slack end)
  const int64_t region = oriented ? round_up(most / 2 + (int64_t)kTmpSlack, 256) : 0;
  const size_t sources = oriented ? (size_t)(2 * region) : (size_t)most + kTmpSlack;
  // ("colour chains": the sums and the staged outputs behind the sources)
  const int64_t stage_at = stage_per_image > 0 ? round_up((int64_t)sources, 256) : 0;
  int rc = tmp_for_stream(ctx, s, stage_per_image > 0 ? (size_t)(stage_at + kColorSumsBytes + most_images * stage_per_image) + kTmpSlack : sources, &tmp);
  if (rc) return rc;
  const void *const resample_src = (const uint8_t *)tmp + region;
  ColorStage stage;
  if (stage_per_image > 0) stage.sums = (unsigned long long *)((uint8_t *)tmp + stage_at), stage.bytes = (uint8_t *)tmp + stage_at + kColorSumsBytes;
  if (lj) rc = scratch_for_stream(ctx, ctx->planes, s, (size_t)most_planes, &planes_d);
  if (rc) return rc;
  const int per_tile = jbk_mcus_per_tile(b->desc.hs, b->desc.vs), mw = 8 * b->desc.hs, mh = 8 * b->desc.vs;
  const jb_device_batch fb = frame_batch(ctx, b);
  for (int64_t i0 = 0; i0 < b->n_images;) {
    int64_t bytes, planes;
    const int m = pack(i0, &bytes, &planes);
    JbCropTable table;
    memset(&table, 0, sizeof table);
    int32_t most_tiles = 0, most_lj_tiles = 0;
    int64_t at = 0;
    for (int j = 0; j < m; j++) {
      const jb_roi &r = written[i0 + j];
      JbCrop &c = table.c[j];
      c.x = r.x, c.y = r.y, c.w = r.width, c.h = r.height;
      c.mx = r.x / mw, c.my = r.y / mh;
      const int mcus_x = (r.x + r.width - 1) / mw - c.mx + 1, mcus_y = (r.y + r.height - 1) / mh - c.my + 1;
      c.tiles_per_row = (mcus_x + per_tile - 1) / per_tile;
      c.n_tiles = mcus_y * c.tiles_per_row;  // (at most the whole image's: no overflow)
      c.tmp_offset = at;
      at += image_bytes(i0 + j);
      if (c.n_tiles > most_tiles) most_tiles = c.n_tiles;
      if (jbk_lj_tiles(c.w, c.h) > most_lj_tiles) most_lj_tiles = jbk_lj_tiles(c.w, c.h);
    }
    const jb_device_batch ib = sub_batch(&fb, i0, m, (uint8_t *)tmp, 0, 0);  // (the strides are per image: the table's)
    JbLaunch p = launch_base(&ib, g);
    p.roi = 2;
    p.tiles_per_image = most_tiles;
    p.n_tiles = m * most_tiles;  // (at most 32 images' worth of tiles: no overflow)
    p.fast_store = 1;            // (the ROI stage does not look at it)
    if (lj) {
      p.tiles_per_image = most_lj_tiles;  // (the tiles of jb_libjpeg.hip's pixel kernel: 256 pixels x 4 rows of the rectangle)
      p.n_tiles = m * most_lj_tiles;
      JB_HIP(ctx, jbk_lj_launch_crops(p, table, b->desc.hs, b->desc.vs, ctx->draft, planes_d, s));
    } else {
      JB_HIP(ctx, jbk_launch_crops(p, table, b->desc.hs, b->desc.vs, s));
    }
    if (oriented) {
      // every image turned into the second region, at its own offset; `table` then describes the oriented sources as
      // the launches of the tail take them (of a row they read w, h and tmp_offset; the pixel launch above has its copy)
      JbOrient q;
      JbOrientTable turn;
      memset(&q, 0, sizeof q);
      memset(&turn, 0, sizeof turn);
      q.src = (const uint8_t *)tmp, q.dst = (uint8_t *)tmp + region;
      q.orientation = orient, q.n_images = m;
      for (int j = 0; j < m; j++) {
        turn.r[j] = JbOrientRow{table.c[j].w, table.c[j].h, table.c[j].tmp_offset, table.c[j].tmp_offset};
        table.c[j].w = shown[i0 + j].width, table.c[j].h = shown[i0 + j].height;
      }
      JB_HIP(ctx, jbk_orient_launch_table(q, turn, s));
    }
    rc = tail(i0, m, table, resample_src, s, stage);
    if (rc) return rc;
    i0 += m;
  }
  return JB_OK;
}

int seam_launch_crops(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const char *fn, const jb_geometry &g,
                      int64_t plane_stride) {
  if (plan.n_crops != b->n_images) return fail(ctx, JB_ERR_GEOMETRY, "%s: %d rectangles for %d images", fn, plan.n_crops, b->n_images);
  // the plan's rectangles and windows are the oriented frame's (ob: the batch with that frame)
  const jb_device_batch ob = oriented_batch(ctx, b, plan.orient);
  std::vector<jb_roi> windows;  // what the pixel kernel writes of every image: with a filter, not the rectangle
  if (plan.filter)
    for (int64_t i = 0; i < b->n_images; i++)
      windows.push_back(jb_filter_window_of_(&ob.desc, &plan.crops[i], plan.inner.width, plan.inner.height, plan.filter));
  const jb_roi *const shown = plan.filter ? windows.data() : plan.crops;
  return rects_into_scratch(ctx, b, stream, plan.orient, shown, g, 0, [&](int64_t i0, int m, const JbCropTable &table, const void *src, hipStream_t s, const ColorStage &) {
    if (plan.filter) {
      JbFilterTable ftable;
      memset(&ftable, 0, sizeof ftable);
      for (int j = 0; j < m; j++) ftable.r[j] = filter_row(plan.crops[i0 + j], shown[i0 + j], table.c[j].tmp_offset);
      JB_HIP(ctx, jbk_filter_launch_crops(filter_args(&ob, plan, plane_stride, src, i0, m), ftable, plan.filter, plan.format, s));
    } else {
      JB_HIP(ctx, jbk_resample_launch_crops(resample_args(&ob, plan, plane_stride, src, i0, m), table, plan.format, s));
    }
    return (int)JB_OK;
  });
}

// "Colour chains" (plan.colors): the resample and filter launches of a tail write format 0 into the stage -- `staged` is
// the plan they take for that: tight outputs of the plan's size, one behind the other -- and jbk_color_launch reads them:
// the chain, then the plan's format at the output's own place.
JbOutPlan staged(const JbOutPlan &plan) {
  JbOutPlan sp = plan;
  sp.format = JB_FMT_RGB_U8_HWC, sp.planar = false, sp.esize = 1;
  memset(&sp.spec, 0, sizeof sp.spec);
  return sp;
}
// the colour launch's arguments but the rows: n staged outputs of the plan's size at `src` -> the plan's format behind dst
JbColor color_args(const JbOutPlan &plan, const uint8_t *src, uint8_t *dst, int64_t dst_row_stride, int64_t plane_stride, int n,
                   const ColorStage &stage) {
  JbColor c;
  memset(&c, 0, sizeof c);
  c.src = src, c.dst = dst;
  c.src_row_stride = 3LL * plan.out_w;
  c.dst_row_stride = dst_row_stride, c.dst_plane_stride = plane_stride;
  c.sums = stage.sums;
  c.w = plan.out_w, c.h = plan.out_h;
  c.n_views = n;
  for (int k = 0; k < 3; k++) c.scale[k] = plan.spec.scale[k], c.bias[k] = plan.spec.bias[k];
  return c;
}
// jb_color_check's status for the n chains of a call, as the call's own refusal (the chain's flat index is in the text)
int colors_check(jb_ctx *ctx, const jb_color_chain *colors, int64_t n, const char *fn) {
  const int rc = jb_color_check(colors, (int)n, nullptr);
  if (rc == JB_OK) return JB_OK;
  const std::string why = jb_last_error(nullptr);
  return fail(ctx, rc, "%s: %s", fn, why.c_str());
}
// behind colors_check: the refusals of the geometric operations that depend on the views' size w x h (jb_color_check_size_), for
// the n checked chains from flat index `first` on
int colors_check_size(jb_ctx *ctx, const jb_color_chain *colors, int64_t first, int64_t n, int32_t w, int32_t h, const char *fn) {
  int64_t bad = 0;
  const char *why = nullptr;
  const int rc = jb_color_check_size_(colors + first, n, w, h, &bad, &why);
  if (rc == JB_OK) return JB_OK;
  return fail(ctx, rc, "%s: colour chain %lld: %s on a view of %d x %d", fn, (long long)(first + bad), why, w, h);
}

// ---- what 3f ("views") and 3g ("view groups") share ------------------------------------------------------------------------
// the union of image i's K sources: the bounding rectangle of its views' rectangles, with a filter of their windows.
// target_of(v) -> JbTarget: the size and the filter view v of an image is resized under.
template <class TargetOf>
jb_roi views_union(const jb_device_batch &ob, const JbOutPlan &plan, int64_t i, TargetOf target_of) {
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  for (int v = 0; v < plan.views_per_image; v++) {
    const jb_view &w = plan.views[i * plan.views_per_image + v];
    const JbTarget t = target_of(v);
    const jb_roi r = {w.x, w.y, w.width, w.height};
    const jb_roi src = t.filter ? jb_filter_window_of_(&ob.desc, &r, t.w, t.h, t.filter) : r;
    if (v == 0 || src.x < x0) x0 = src.x;
    if (v == 0 || src.y < y0) y0 = src.y;
    if (v == 0 || src.x + src.width > x1) x1 = src.x + src.width;
    if (v == 0 || src.y + src.height > y1) y1 = src.y + src.height;
  }
  return jb_roi{x0, y0, x1 - x0, y1 - y0};
}

// A RUN: the views [first, first + n) of every image of the call, resized under one plan -- its target, filter and format --
// into one buffer: output (i, v - first) lies at dst + i * image_stride + (v - first) * view_stride.  "Views" is one run
// of all K views under the call's plan, "view groups" one run per group under jb_view_group_plan_.
struct ViewRun {
  JbOutPlan plan;
  int first, n;
  uint8_t *dst;
  int64_t row_stride, plane_stride, image_stride, view_stride;
};
// the rows of one launch, area or filtered, every one with its output's place behind the launch's dst
struct ViewRows {
  JbViewGroupTable area;
  JbViewGroupFilterTable filtered;
};

// n rows under `rp` (a run's plan, or `staged` of it) -> dst, rows row_stride and planes plane_stride apart.  The ONE place
// that knows the two table flavours: under a call with groups every row travels with its place (the kViewGroups
// launches); under one without, the rows lie `stride` apart from the first one's place on and travel without theirs (the
// kViews launches).  The call's plan decides, not the spacing the rows happen to have.
int launch_view_rows(jb_ctx *ctx, const jb_device_batch &ob, const JbOutPlan &rp, bool grouped, const ViewRows &rows, int n, uint8_t *dst,
                     int64_t row_stride, int64_t plane_stride, int64_t stride, const void *src, hipStream_t s) {
  jb_device_batch rb = ob;  // (resample_args: one "image" at dst -- where the others are is said below, or by the rows)
  rb.d_rgb = dst, rb.rgb_row_stride = row_stride, rb.n_images = 1;
  JbFilter f = filter_args(&rb, rp, plane_stride, src, 0, n);
  if (grouped) {
    if (rp.filter) JB_HIP(ctx, jbk_filter_launch_view_groups(f, rows.filtered, rp.filter, rp.format, s));
    else JB_HIP(ctx, jbk_resample_launch_view_groups(f.base, rows.area, rp.format, s));
    return JB_OK;
  }
  f.base.dst += rp.filter ? rows.filtered.r[0].dst_offset : rows.area.r[0].dst_offset;
  f.base.dst_image_stride = stride;
  if (rp.filter) {
    JbViewFilterTable ft;
    memset(&ft, 0, sizeof ft);
    for (int t = 0; t < n; t++) ft.r[t] = rows.filtered.r[t].f;
    ft.mirror = rows.filtered.mirror;
    JB_HIP(ctx, jbk_filter_launch_views(f, ft, rp.filter, rp.format, s));
  } else {
    JbViewTable vt;
    memset(&vt, 0, sizeof vt);
    for (int t = 0; t < n; t++) vt.r[t] = rows.area.r[t].v;
    JB_HIP(ctx, jbk_resample_launch_views(f.base, vt, rp.format, s));
  }
  return JB_OK;
}

// a run's outputs of a sub-batch -- images i0 .. i0 + m - 1, image i0 + j's union at src + table.c[j].tmp_offset -- cut into
// launches of kJbCropsPerLaunch rows, so one pixel launch may be followed by several.  plan: the call's (its views, chains
// and K).  "Colour chains": the rows go to run_stage instead -- the run's m * n outputs in format 0, tight, in the run's order
// -- and a colour launch takes them from there to their places.
int launch_run(jb_ctx *ctx, const jb_device_batch &ob, const JbOutPlan &plan, const ViewRun &run, const jb_roi *unions, const JbCropTable &table,
               int64_t i0, int m, const void *src, hipStream_t s, const ColorStage &stage, uint8_t *run_stage) {
  const bool grouped = plan.n_groups > 0, colored = plan.colors != nullptr;
  const int64_t staged_bytes = 3LL * run.plan.out_w * run.plan.out_h;
  const int64_t n_rows = (int64_t)m * run.n;
  for (int64_t n0 = 0; n0 < n_rows; n0 += kJbCropsPerLaunch) {
    const int n = (int)(n_rows - n0 < kJbCropsPerLaunch ? n_rows - n0 : kJbCropsPerLaunch);
    ViewRows rows;
    JbColorTable ct;
    memset(&rows, 0, sizeof rows);
    memset(&ct, 0, sizeof ct);
    for (int t = 0; t < n; t++) {
      const int j = (int)((n0 + t) / run.n), v = (int)((n0 + t) % run.n);    // the image of the sub-batch, the view of the run
      const int64_t flat = (i0 + j) * plan.views_per_image + run.first + v;  // the caller's index of the view and of its chain
      const jb_view &w = plan.views[flat];
      const jb_roi &u = unions[i0 + j];
      const int mirror = (w.flags & JB_VIEW_MIRROR) ? 1 : 0;
      int64_t at = (i0 + j) * run.image_stride + v * run.view_stride;  // the output's place behind run.dst
      if (colored) {
        ct.r[t] = JbColorRow{(n0 + t) * staged_bytes, at, plan.colors[flat]};
        at = (n0 + t) * staged_bytes;
      }
      if (run.plan.filter) {
        rows.filtered.r[t] = JbViewGroupFilterRow{filter_row(jb_roi{w.x, w.y, w.width, w.height}, u, table.c[j].tmp_offset), at};
        rows.filtered.mirror |= (uint32_t)mirror << t;
      } else {
        rows.area.r[t] = JbViewGroupRow{JbViewRow{table.c[j].tmp_offset, 3 * u.width, w.x - u.x, w.y - u.y, w.width, w.height, mirror}, at};
      }
    }
    const int rc = colored ? launch_view_rows(ctx, ob, staged(run.plan), grouped, rows, n, run_stage, 3LL * run.plan.out_w, 0, staged_bytes, src, s)
                           : launch_view_rows(ctx, ob, run.plan, grouped, rows, n, run.dst, run.row_stride, run.plane_stride, run.view_stride, src, s);
    if (rc) return rc;
    if (colored)
      JB_HIP(ctx, jbk_color_launch(color_args(run.plan, run_stage, run.dst, run.row_stride, run.plane_stride, n, stage), ct, plan.format, s));
  }
  return JB_OK;
}

// the launches of a call with views, behind its checks: every image's union through 3c's first half, then run by run
// the tail above.  "Colour chains": the chains are checked here, and the stage of a sub-batch holds run 0's outputs of its
// images, then run 1's, ...
int launch_view_runs(jb_ctx *ctx, const jb_device_batch *b, const jb_device_batch &ob, void *stream, const JbOutPlan &plan, const jb_geometry &g,
                     const std::vector<jb_roi> &unions, const ViewRun *runs, int n_runs, const char *fn) {
  const bool colored = plan.colors != nullptr;
  if (colored)
    if (const int rc = colors_check(ctx, plan.colors, plan.n_views, fn)) return rc;
  if (colored)  // (a run's views have the run's size)
    for (int64_t i = 0; i < plan.n_views / plan.views_per_image; i++)
      for (int q = 0; q < n_runs; q++)
        if (const int rc = colors_check_size(ctx, plan.colors, i * plan.views_per_image + runs[q].first, runs[q].n, runs[q].plan.out_w, runs[q].plan.out_h, fn))
          return rc;
  const auto staged_bytes_of = [&](int q) { return 3LL * runs[q].plan.out_w * runs[q].plan.out_h * runs[q].n; };  // of a run, per image
  int64_t staged_per_image = 0;
  for (int q = 0; q < n_runs; q++) staged_per_image += staged_bytes_of(q);
  return rects_into_scratch(ctx, b, stream, plan.orient, unions.data(), g, colored ? staged_per_image : 0,
                            [&](int64_t i0, int m, const JbCropTable &table, const void *src, hipStream_t s, const ColorStage &stage) {
    uint8_t *run_stage = stage.bytes;
    for (int q = 0; q < n_runs; q++) {
      const int rc = launch_run(ctx, ob, plan, runs[q], unions.data(), table, i0, m, src, s, stage, run_stage);
      if (rc) return rc;
      if (colored) run_stage += m * staged_bytes_of(q);
    }
    return (int)JB_OK;
  });
}

// 3f. "views" (plan.views): K outputs per image from ONE pixel launch.  Per image the UNION -- the bounding rectangle of
// its K rectangles, with a filter of their K windows -- goes through 3c's first half; the view kernels then read K
// sub-rectangles of each union, kJbCropsPerLaunch outputs a launch, so one pixel launch may be followed by several.
// (A union may be much larger than its views: accepted, see include/jpegblk.h.)
int seam_launch_views(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const char *fn) {
  jb_geometry g;
  int64_t plane_stride = 0;
  int rc = seam_check(ctx, b, plan, fn, &g, &plane_stride);
  if (rc) return rc;
  const int k = plan.views_per_image;
  if (plan.n_views != (int64_t)b->n_images * k) return fail(ctx, JB_ERR_GEOMETRY, "%s: %d views for %d images", fn, plan.n_views, b->n_images);
  if (b->n_images == 1 && k > 1) {
    // one image, several outputs: the strides between OUTPUTS count all the same (seam_check looks at them for a batch)
    jb_device_batch outputs = *b;
    outputs.n_images = k;
    outputs.coef_image_stride = g.coef_bytes;
    rc = seam_check(ctx, &outputs, plan, fn, &g, &plane_stride);
    if (rc) return rc;
  }
  const jb_device_batch ob = oriented_batch(ctx, b, plan.orient);
  std::vector<jb_roi> unions;
  for (int64_t i = 0; i < b->n_images; i++)
    unions.push_back(views_union(ob, plan, i, [&](int) { return JbTarget{plan.inner.width, plan.inner.height, plan.filter, 0}; }));
  // one run: the outputs are b's "images", one d_rgb index per view, K of them per image
  const ViewRun run = {plan, 0, k, b->d_rgb, b->rgb_row_stride, plane_stride, k * b->rgb_image_stride, b->rgb_image_stride};
  return launch_view_runs(ctx, b, ob, stream, plan, g, unions, &run, 1, fn);
}

// 3g. "view groups" (plan.n_groups): 3f with a target and a filter per GROUP of an image's views.  The union of an image is
// taken over all its K views, each under its own group's resize; the first half is 3c's, unchanged.  The tail makes, per
// group, ceil(m * K_g / 32) launches of the kViewGroups mode: a group's outputs of consecutive images are not evenly
// spaced (the other groups' may lie between them), so every row carries its place behind the group's d_out.
int seam_launch_view_groups(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const jb_view_output *outs, const char *fn) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "%s: ctx is NULL", fn);
  if (!b || !outs) return fail(ctx, JB_ERR_NULL, "%s: NULL pointer", fn);
  jb_geometry g;
  int64_t plane_strides[JB_VIEW_GROUPS_MAX] = {0, 0, 0, 0};
  const int k = plan.views_per_image;
  // every group's buffer against the group's plan, as a batch's d_rgb is checked: the images, then the views of one image
  // (plan.n_groups is 0 for a plan that has failed: one round, which reports it)
  for (int q = 0; q < (plan.n_groups > 0 ? plan.n_groups : 1); q++) {
    JbOutPlan gp = plan.status == JB_OK ? jb_view_group_plan_(plan, q) : plan;
    gp.spec.plane_stride = outs[q].plane_stride;
    jb_device_batch ob = *b;
    // (a failed plan is reported by the check behind the batch's own pointers and descriptor, whatever outs holds)
    ob.d_rgb = plan.status == JB_OK ? (uint8_t *)outs[q].d_out : (uint8_t *)b->d_coef;
    ob.rgb_row_stride = outs[q].row_stride, ob.rgb_image_stride = outs[q].image_stride;
    int rc = seam_check(ctx, &ob, gp, fn, &g, &plane_strides[q]);
    if (rc) return rc;
    if (plan.n_views != (int64_t)b->n_images * k) return fail(ctx, JB_ERR_GEOMETRY, "%s: %d views for %d images", fn, plan.n_views, b->n_images);
    const int kg = plan.groups[q].n_views;
    if (kg > 1) {
      ob.n_images = kg;
      ob.coef_image_stride = g.coef_bytes;
      ob.rgb_image_stride = outs[q].view_stride;
      rc = seam_check(ctx, &ob, gp, fn, &g, &plane_strides[q]);
      if (rc) return rc;
    }
    const int64_t one = gp.planar ? 2 * plane_strides[q] + outs[q].row_stride * (int64_t)gp.out_h : outs[q].row_stride * (int64_t)gp.out_h;
    if (b->n_images > 1 && outs[q].image_stride < (kg - 1) * outs[q].view_stride + one)
      return fail(ctx, JB_ERR_GEOMETRY, "%s: group %d: image_stride smaller than the image's %d outputs", fn, q, kg);
  }
  const jb_device_batch ob = oriented_batch(ctx, b, plan.orient);
  const auto group_of = [&](int v) {
    int q = 0;
    while (v >= plan.groups[q].first + plan.groups[q].n_views) q++;
    return q;
  };
  // every view under ITS group's target and filter; one run per group, into the group's buffer
  std::vector<jb_roi> unions;
  for (int64_t i = 0; i < b->n_images; i++)
    unions.push_back(views_union(ob, plan, i, [&](int v) {
      const JbOutPlan::Group &gr = plan.groups[group_of(v)];
      return JbTarget{gr.out_w, gr.out_h, gr.filter, 0};
    }));
  std::vector<ViewRun> runs;
  for (int q = 0; q < plan.n_groups; q++)
    runs.push_back(ViewRun{jb_view_group_plan_(plan, q), plan.groups[q].first, plan.groups[q].n_views, (uint8_t *)outs[q].d_out, outs[q].row_stride,
                           plane_strides[q], outs[q].image_stride, outs[q].view_stride});
  return launch_view_runs(ctx, b, ob, stream, plan, g, unions, runs.data(), plan.n_groups, fn);
}

// 3b. a plan with a target size: two launches per sub-batch, in stream order -- the pixel kernel (full size or the
// rectangle, interleaved uint8, tight) into the stream's scratch, jb_resample_kernel from there into the caller's buffer
int seam_launch_resized(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const char *fn) {
  jb_geometry g;
  int64_t plane_stride = 0;
  int rc = seam_check(ctx, b, plan, fn, &g, &plane_stride);
  if (rc) return rc;
  if (plan.crops) return seam_launch_crops(ctx, b, stream, plan, fn, g, plane_stride);
  // (with a filter other than 0 the source is the window: the ROI store stage with the window in the rectangle's place)
  const jb_device_batch fb = frame_batch(ctx, b);  // ("draft decode": the source is the draft frame)
  const JbOutPlan inner = jb_out_plan_(&fb.desc, 1, nullptr, plan.filter ? &plan.window : plan.has_roi ? &plan.roi : nullptr);
  if (inner.status != JB_OK) return fail(ctx, inner.status, "%s: %s", fn, inner.why);
  // whole images per sub-batch: as many as the cap holds, one at the least
  const int64_t cap = (int64_t)ctx->knobs.resize_tmp_bytes;
  int64_t per = cap / plan.tmp_image_bytes;
  if (per < 1) per = 1;
  if (per > b->n_images) per = b->n_images;
  if (((int64_t)(plan.inner.width + 63) / 64) * ((plan.inner.height + 3) / 4) * per > 0x7fffffffLL || !fill_fits(plan, b->n_images))
    return fail(ctx, JB_ERR_CAPACITY, "batch too large for one launch");
  DeviceGuard guard(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  void *tmp = nullptr;
  rc = tmp_for_stream(ctx, s, (size_t)(per * plan.tmp_image_bytes) + kTmpSlack, &tmp);
  if (rc) return rc;
  for (int64_t i0 = 0; i0 < b->n_images; i0 += per) {
    const int m = (int)(b->n_images - i0 < per ? b->n_images - i0 : per);
    const jb_device_batch ib = sub_batch(b, i0, m, (uint8_t *)tmp, inner.row_stride, plan.tmp_image_bytes);
    rc = seam_launch(ctx, &ib, s, inner, fn);
    if (rc) return rc;
    rc = whole_images_tail(ctx, &fb, plan, plane_stride, tmp, i0, m, s);
    if (rc) return rc;
  }
  // JB_FIT_PAD: the border of every image of the call in one launch.  Bands and inner rectangles are disjoint, so its place
  // on the stream is free: behind the last sub-batch, so that a sub-batch that fails leaves the bands alone
  if (plan.fit_mode == JB_FIT_PAD) JB_HIP(ctx, jbk_fit_fill_launch(fill_args(b, plan, plane_stride, 0, b->n_images), plan.format, s));
  return JB_OK;
}

// 3e. "orientation": a plan of the oriented frame (plan.orient 2..8).  The pixel launch -- the context's arithmetic,
// format 0, tight -- writes what the output shows of the STORED frame into the stream's scratch: the whole frame, the
// rectangle, or with a filter the window, each mapped back (jb_orient_map_roi).  jb_orient_kernel turns it: without a
// target size into the caller's buffer, in the plan's format; with one into a second tight region of the same scratch,
// which the resample or filter launch then reads exactly as 3b's reads the first.  Sub-batches of whole images: as
// many as the cap holds, both regions counted.
int seam_launch_oriented(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const char *fn) {
  jb_geometry g;
  int64_t plane_stride = 0;
  int rc = seam_check(ctx, b, plan, fn, &g, &plane_stride);
  if (rc) return rc;
  if (plan.crops) return seam_launch_crops(ctx, b, stream, plan, fn, g, plane_stride);
  const jb_device_batch ob = oriented_batch(ctx, b, plan.orient);
  const jb_roi whole = {0, 0, ob.desc.width, ob.desc.height};
  const jb_roi shown = plan.filter ? plan.window : plan.has_roi ? plan.roi : whole;
  const jb_roi stored = stored_rect(b, plan.orient, shown);
  const bool all = stored.width == b->desc.width && stored.height == b->desc.height;
  const JbOutPlan inner = jb_out_plan_(&b->desc, 1, nullptr, all ? nullptr : &stored);
  if (inner.status != JB_OK) return fail(ctx, inner.status, "%s: %s", fn, inner.why);
  const int n_regions = plan.has_resize ? 2 : 1;
  const int64_t image_bytes = inner.image_bytes;  // 3 * stored.width * stored.height, of either region
  int64_t per = (int64_t)ctx->knobs.resize_tmp_bytes / (n_regions * image_bytes);
  if (per < 1) per = 1;
  if (per > b->n_images) per = b->n_images;
  const int64_t tile = kJbOrientTile;
  if (((stored.width + tile - 1) / tile) * ((stored.height + tile - 1) / tile) * per > 0x7fffffffLL ||
      (plan.has_resize && (((int64_t)(plan.inner.width + 63) / 64) * ((plan.inner.height + 3) / 4) * per > 0x7fffffffLL || !fill_fits(plan, b->n_images))))
    return fail(ctx, JB_ERR_CAPACITY, "batch too large for one launch");
  DeviceGuard guard(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const int64_t region = round_up(per * image_bytes + (int64_t)kTmpSlack, 256);
  void *tmp = nullptr;
  rc = tmp_for_stream(ctx, s, (size_t)(n_regions * region), &tmp);
  if (rc) return rc;
  uint8_t *const turned = (uint8_t *)tmp + region;  // (the second region)
  const int64_t rgb_step = b->n_images > 1 ? b->rgb_image_stride : 0;
  for (int64_t i0 = 0; i0 < b->n_images; i0 += per) {
    const int m = (int)(b->n_images - i0 < per ? b->n_images - i0 : per);
    const jb_device_batch ib = sub_batch(b, i0, m, (uint8_t *)tmp, inner.row_stride, image_bytes);
    rc = seam_launch(ctx, &ib, s, inner, fn);
    if (rc) return rc;
    JbOrient q;
    memset(&q, 0, sizeof q);
    q.src = (const uint8_t *)tmp;
    q.src_image_stride = image_bytes;
    q.sw = stored.width, q.sh = stored.height;
    q.orientation = plan.orient;
    q.n_images = m;
    if (!plan.has_resize) {
      q.dst = b->d_rgb + i0 * rgb_step;
      q.dst_image_stride = rgb_step;
      q.dst_row_stride = b->rgb_row_stride;
      q.dst_plane_stride = plane_stride;
      for (int c = 0; c < 3; c++) q.scale[c] = plan.spec.scale[c], q.bias[c] = plan.spec.bias[c];
      JB_HIP(ctx, jbk_orient_launch(q, plan.format, s));
      continue;
    }
    q.dst = turned;
    q.dst_image_stride = image_bytes;
    q.dst_row_stride = 3LL * shown.width;
    JB_HIP(ctx, jbk_orient_launch(q, JB_FMT_RGB_U8_HWC, s));
    rc = whole_images_tail(ctx, &ob, plan, plane_stride, turned, i0, m, s);
    if (rc) return rc;
  }
  if (plan.fit_mode == JB_FIT_PAD) JB_HIP(ctx, jbk_fit_fill_launch(fill_args(b, plan, plane_stride, 0, b->n_images), plan.format, s));  // (as in 3b: last)
  return JB_OK;
}

// 3d. JB_ARITH_LIBJPEG: jb_libjpeg.hip's launch pair in the place of jbk_launch -- any format, the whole image or the
// plan's rectangle, scale 1 (seam_check has refused another).  The planes of a sub-batch of whole images are held to the
// cap of the resized routes' scratch (one image at the least), in the stream's scratch of their own.  p: launch_base's,
// with the planar fields set.
int seam_launch_lj(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const jb_geometry &g, JbLaunch p) {
  const jb_roi whole = {0, 0, p.width, p.height};  // (launch_base: the draft frame)
  const jb_roi &r = plan.has_roi ? plan.roi : whole;
  if (plan.has_roi) p.roi = 1, p.roi_x = r.x, p.roi_y = r.y, p.roi_w = r.width, p.roi_h = r.height;
  p.tiles_per_image = jbk_lj_tiles(r.width, r.height);
  const JbLjWindow win = lj_window(ctx, b, g, r);
  int64_t per = (int64_t)ctx->knobs.resize_tmp_bytes / win.bytes;
  if (per < 1) per = 1;
  if (per > b->n_images) per = b->n_images;
  if (p.tiles_per_image < 1 || per * p.tiles_per_image > 0x7fffffffLL) return fail(ctx, JB_ERR_CAPACITY, "batch too large for one launch");
  DeviceGuard guard(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  void *planes = nullptr;
  int rc = scratch_for_stream(ctx, ctx->planes, s, (size_t)(per * win.bytes), &planes);
  if (rc) return rc;
  const int64_t coef_step = b->n_images > 1 ? b->coef_image_stride : 0, rgb_step = b->n_images > 1 ? b->rgb_image_stride : 0;
  for (int64_t i0 = 0; i0 < b->n_images; i0 += per) {
    const int64_t m = b->n_images - i0 < per ? b->n_images - i0 : per;
    JbLaunch q = p;
    q.coef = (const int16_t *)((const uint8_t *)b->d_coef + i0 * coef_step);
    q.coef_image_stride = coef_step;
    q.qtabs = (const int32_t *)((const uint8_t *)b->d_qtabs + i0 * b->qtab_image_stride);
    q.rgb = b->d_rgb + i0 * rgb_step;
    q.rgb_image_stride = rgb_step;
    q.n_tiles = (int32_t)(m * p.tiles_per_image);
    JB_HIP(ctx, jbk_lj_launch(q, b->desc.hs, b->desc.vs, ctx->draft, planes, s));
  }
  return JB_OK;
}

}  // namespace

// 3. the launch, on `stream` or (null) the context's primary stream; fn: the entry point's name, for the error text
int seam_launch(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan, const char *fn) {
  if (plan.n_groups > 0 && plan.orient != JB_ORIENT_EXIF && ctx && b) {
    // a submission's block buffer (b->d_rgb, images b->rgb_image_stride apart) as the groups' outputs: tight, group g at its offset
    jb_view_output outs[JB_VIEW_GROUPS_MAX];
    for (int q = 0; q < plan.n_groups; q++)
      outs[q] = jb_view_output{b->d_rgb ? b->d_rgb + plan.groups[q].offset : nullptr, b->rgb_image_stride, plan.groups[q].view_bytes, plan.groups[q].row_stride, 0};
    return seam_launch_view_groups(ctx, b, stream, plan, outs, fn);
  }
  if (plan.views && plan.orient != JB_ORIENT_EXIF && ctx && b) return seam_launch_views(ctx, b, stream, plan, fn);
  if (plan.orient != JB_ORIENT_STORED && plan.orient != JB_ORIENT_EXIF && ctx && b) return seam_launch_oriented(ctx, b, stream, plan, fn);
  if (plan.has_resize && ctx && b) return seam_launch_resized(ctx, b, stream, plan, fn);
  jb_geometry g;
  int64_t plane_stride = 0;
  int rc = seam_check(ctx, b, plan, fn, &g, &plane_stride);
  if (rc) return rc;
  const jb_device_batch fb = frame_batch(ctx, b);
  JbLaunch p = launch_base(&fb, g);
  if (plan.planar) {
    p.format = plan.format;
    p.rgb_plane_stride = plane_stride;
    for (int c = 0; c < 3; c++) p.scale[c] = plan.spec.scale[c], p.bias[c] = plan.spec.bias[c];
  }
  if (ctx->arithmetic == JB_ARITH_LIBJPEG) return seam_launch_lj(ctx, b, stream, plan, g, p);
  rc = seam_tiles(ctx, b, g, plan, p);
  if (rc) return rc;
  // the flat front end (jb_kernels.h): wherever every workgroup's coefficients lie at d_coef + workgroup * tile bytes
  const bool flat = ctx->knobs.flat_front && jbk_flat_front(p, b->desc.hs, b->desc.vs, plan.scale);
  DeviceGuard guard(ctx->device);
  JB_HIP(ctx, jbk_launch(p, b->desc.hs, b->desc.vs, plan.scale, stream ? (hipStream_t)stream : ctx->stream, flat));
  ctx->last_front = flat ? JB_FRONT_FLAT : JB_FRONT_GENERAL, ctx->last_linear = p.linear;
  return JB_OK;
}

// the plan of a seam entry point: of b's frame under the context's orientation
static JbOutPlan seam_plan(const jb_ctx *ctx, const jb_device_batch *b, int scale, const jb_output_spec *spec, const jb_roi *roi = nullptr,
                           const JbTarget *target = nullptr, const jb_roi *crops = nullptr, int n_crops = 0, const jb_fit *fit = nullptr) {
  // ("draft decode": of the context's draft frame)
  jb_image_desc frame = {};
  if (b) frame = jb_draft_desc_(&b->desc, ctx ? ctx->draft : 1);
  return jb_out_plan_(b ? &frame : nullptr, scale, spec, roi, target, crops, n_crops, ctx ? ctx->orientation : JB_ORIENT_STORED, fit);
}

extern "C" {

const char *jb_kernel_name(const jb_image_desc *d) {
  if (!d) return "";
  return jbk_kernel_name(d->hs, d->vs);
}

int jb_ctx_last_front(const jb_ctx *ctx, int *linear) {
  if (linear) *linear = ctx ? ctx->last_linear : 0;
  return ctx ? ctx->last_front : JB_FRONT_NONE;
}

int jb_blocks_to_rgb_device(jb_ctx *ctx, const jb_device_batch *b, void *stream) {
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, nullptr), "jb_blocks_to_rgb_device");
}

int jb_blocks_to_rgb_device_scaled(jb_ctx *ctx, const jb_device_batch *b, int denom, void *stream) {
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, denom, nullptr), "jb_blocks_to_rgb_device_scaled");
}

int jb_blocks_to_rgb_device_fmt(jb_ctx *ctx, const jb_device_batch *b, const jb_output_spec *spec, void *stream) {
  if (ctx && !spec) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb_device_fmt: spec is NULL");
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec), "jb_blocks_to_rgb_device_fmt");
}

int jb_blocks_to_rgb_device_roi(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *roi, const jb_output_spec *spec, void *stream) {
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, roi), "jb_blocks_to_rgb_device_roi");
}

int jb_blocks_to_rgb_device_resized(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *roi, int32_t out_w, int32_t out_h,
                                    const jb_output_spec *spec, void *stream) {
  const JbTarget t = {out_w, out_h};
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, roi, &t), "jb_blocks_to_rgb_device_resized");
}

int jb_blocks_to_rgb_device_crops(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *rois, int32_t out_w, int32_t out_h,
                                  const jb_output_spec *spec, void *stream) {
  if (ctx && !rois) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb_device_crops: rois is NULL");
  const JbTarget t = {out_w, out_h};
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, nullptr, &t, rois, b ? b->n_images : 0),
                     "jb_blocks_to_rgb_device_crops");
}

int jb_blocks_to_rgb_device_filtered(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *roi, const jb_resize *rs,
                                     const jb_output_spec *spec, void *stream) {
  if (ctx && !rs) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb_device_filtered: rs is NULL");
  const JbTarget t = rs ? JbTarget{rs->out_w, rs->out_h, rs->filter, rs->reserved} : JbTarget{};
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, roi, &t), "jb_blocks_to_rgb_device_filtered");
}

int jb_blocks_to_rgb_device_fit(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit,
                                const jb_output_spec *spec, void *stream) {
  if (ctx && !rs) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb_device_fit: rs is NULL");
  const JbTarget t = rs ? JbTarget{rs->out_w, rs->out_h, rs->filter, rs->reserved} : JbTarget{};
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, roi, &t, nullptr, 0, fit), "jb_blocks_to_rgb_device_fit");
}

int jb_blocks_to_rgb_device_crops_filtered(jb_ctx *ctx, const jb_device_batch *b, const jb_roi *rois, const jb_resize *rs,
                                           const jb_output_spec *spec, void *stream) {
  if (ctx && (!rois || !rs)) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb_device_crops_filtered: NULL pointer");
  const JbTarget t = rs ? JbTarget{rs->out_w, rs->out_h, rs->filter, rs->reserved} : JbTarget{};
  return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec, nullptr, &t, rois, b ? b->n_images : 0),
                     "jb_blocks_to_rgb_device_crops_filtered");
}

static int views_entry(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, int views_per_image, const jb_resize *rs,
                       const jb_color_chain *colors, const jb_output_spec *spec, void *stream, const char *fn);

int jb_blocks_to_rgb_device_views(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, int views_per_image, const jb_resize *rs,
                                  const jb_output_spec *spec, void *stream) {
  return views_entry(ctx, b, views, views_per_image, rs, nullptr, spec, stream, "jb_blocks_to_rgb_device_views");
}

int jb_blocks_to_rgb_device_views_color(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, int views_per_image, const jb_resize *rs,
                                        const jb_color_chain *colors, const jb_output_spec *spec, void *stream) {
  return views_entry(ctx, b, views, views_per_image, rs, colors, spec, stream, "jb_blocks_to_rgb_device_views_color");
}

static int views_entry(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, int views_per_image, const jb_resize *rs,
                       const jb_color_chain *colors, const jb_output_spec *spec, void *stream, const char *fn) {
  if (ctx && (!views || !rs)) return fail(ctx, JB_ERR_NULL, "%s: NULL pointer", fn);
  if (!ctx || !b) return seam_launch(ctx, b, stream, seam_plan(ctx, b, 1, spec), fn);  // (JB_ERR_NULL)
  const jb_image_desc frame = jb_draft_desc_(&b->desc, ctx->draft);
  JbOutPlan plan = jb_views_plan_(&frame, spec, views, b->n_images < 0 ? 0 : b->n_images, views_per_image, rs, ctx->orientation);
  plan.colors = colors;
  return seam_launch(ctx, b, stream, plan, fn);
}

static int view_groups_entry(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, const jb_view_group *groups, const jb_view_output *outputs,
                             int n_groups, const jb_color_chain *colors, const jb_output_spec *spec, void *stream, const char *fn);

int jb_blocks_to_rgb_device_view_groups_color(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, const jb_view_group *groups,
                                              const jb_view_output *outputs, int n_groups, const jb_color_chain *colors,
                                              const jb_output_spec *spec, void *stream) {
  return view_groups_entry(ctx, b, views, groups, outputs, n_groups, colors, spec, stream, "jb_blocks_to_rgb_device_view_groups_color");
}

int jb_blocks_to_rgb_device_view_groups(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, const jb_view_group *groups,
                                        const jb_view_output *outputs, int n_groups, const jb_output_spec *spec, void *stream) {
  return view_groups_entry(ctx, b, views, groups, outputs, n_groups, nullptr, spec, stream, "jb_blocks_to_rgb_device_view_groups");
}

static int view_groups_entry(jb_ctx *ctx, const jb_device_batch *b, const jb_view *views, const jb_view_group *groups, const jb_view_output *outputs,
                             int n_groups, const jb_color_chain *colors, const jb_output_spec *spec, void *stream, const char *fn) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "%s: ctx is NULL", fn);
  if (!b || !views || !groups || !outputs) return fail(ctx, JB_ERR_NULL, "%s: NULL pointer", fn);
  if (spec && spec->plane_stride != 0) return fail(ctx, JB_ERR_GEOMETRY, "%s: spec->plane_stride must be 0 (every jb_view_output has its own)", fn);
  const jb_image_desc frame = jb_draft_desc_(&b->desc, ctx->draft);
  JbOutPlan plan = jb_view_groups_plan_(&frame, spec, views, b->n_images < 0 ? 0 : b->n_images, groups, n_groups, ctx->orientation);
  if (plan.status == JB_OK) plan.colors = colors;
  // (a plan that has failed has no groups: outputs[0] is then all the check reads, and n_groups < 1 has none to read)
  static const jb_view_output none = {};
  return seam_launch_view_groups(ctx, b, stream, plan, n_groups >= 1 ? outputs : &none, fn);
}

int jb_color_device(jb_ctx *ctx, const uint8_t *d_in, int64_t in_row_stride, int64_t in_image_stride, int32_t w, int32_t h, int32_t n_images,
                    const jb_color_chain *chains, void *d_out, int64_t out_row_stride, int64_t out_image_stride, const jb_output_spec *spec,
                    void *stream) {
  const char *const fn = "jb_color_device";
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "%s: ctx is NULL", fn);
  if (!d_in || !chains || !d_out) return fail(ctx, JB_ERR_NULL, "%s: NULL pointer", fn);
  if (n_images < 1) return fail(ctx, JB_ERR_GEOMETRY, "%s: n_images = %d", fn, n_images);
  // the output as a plan describes it: a w x h frame in the spec's format (sampling and tables are not looked at)
  const jb_image_desc frame = {w, h, 1, 1, {0, 0, 0}, 0};
  const JbOutPlan plan = jb_out_plan_(&frame, 1, spec);
  if (plan.status != JB_OK) return fail(ctx, plan.status, "%s: %s", fn, plan.why);
  int64_t plane_stride = 0;
  if (plan.planar) {
    if (jb_output_spec_check(&plan.spec, h, out_row_stride) != JB_OK)
      return fail(ctx, JB_ERR_GEOMETRY, "%s: bad output spec (reserved, plane_stride < row stride * height, or scale / bias not finite)", fn);
    plane_stride = plan.spec.plane_stride ? plan.spec.plane_stride : out_row_stride * (int64_t)h;
    if (((uintptr_t)d_out | (uint64_t)out_row_stride | (uint64_t)plane_stride | (uint64_t)(n_images > 1 ? out_image_stride : 0)) & (uint64_t)(plan.esize - 1))
      return fail(ctx, JB_ERR_GEOMETRY, "%s: f32 / f16 output wants the pointer and every stride to be multiples of the element size", fn);
  }
  const int64_t one_out = plan.planar ? 2 * plane_stride + out_row_stride * (int64_t)h : out_row_stride * (int64_t)h;
  if (in_row_stride < 3LL * w || out_row_stride < plan.row_stride)
    return fail(ctx, JB_ERR_GEOMETRY, "%s: a row stride is smaller than one row", fn);
  if (n_images > 1 && (in_image_stride < in_row_stride * (int64_t)(h - 1) + 3LL * w || out_image_stride < one_out))
    return fail(ctx, JB_ERR_GEOMETRY, "%s: image strides smaller than one image", fn);
  int rc = colors_check(ctx, chains, n_images, fn);
  if (rc != JB_OK) return rc;
  rc = colors_check_size(ctx, chains, 0, n_images, w, h, fn);
  if (rc != JB_OK) return rc;
  DeviceGuard guard(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  void *tmp = nullptr;
  rc = tmp_for_stream(ctx, s, (size_t)kColorSumsBytes, &tmp);  // (the launches of a stream are ordered: one set of sums)
  if (rc) return rc;
  ColorStage stage;
  stage.sums = (unsigned long long *)tmp;
  for (int64_t i0 = 0; i0 < n_images; i0 += kJbCropsPerLaunch) {
    const int n = (int)(n_images - i0 < kJbCropsPerLaunch ? n_images - i0 : kJbCropsPerLaunch);
    JbColorTable ct;
    memset(&ct, 0, sizeof ct);
    for (int t = 0; t < n; t++) ct.r[t] = JbColorRow{(i0 + t) * (n_images > 1 ? in_image_stride : 0), (i0 + t) * (n_images > 1 ? out_image_stride : 0), chains[i0 + t]};
    JbColor c = color_args(plan, d_in, (uint8_t *)d_out, out_row_stride, plane_stride, n, stage);
    c.src_row_stride = in_row_stride;
    JB_HIP(ctx, jbk_color_launch(c, ct, plan.format, s));
  }
  return JB_OK;
}

}  // extern "C"
