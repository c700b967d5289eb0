// jb_plan.h -- "what the pixels look like": the ONE description of a decode's output that travels from the C ABI
// (include/jpegblk.h) to the kernel launch, and the one function that derives it (jb_geometry.cpp: host-only, like
// this header, so the front end still builds on a CPU-only toolchain for tools/fuzz/).  Every size and stride of the
// output -- staging, arena, ring slots, copies, the launch -- is read from here and computed nowhere else.
#pragma once
#include "../../include/jpegblk.h"

struct JbOutPlan {
  // JB_OK, or why this output cannot be had: JB_ERR_NULL (no descriptor), JB_ERR_GEOMETRY (scale not 1, 2, 4, 8; image
  // size outside 1..65535; unknown format; reserved != 0 on a format-0 spec), JB_ERR_UNSUPPORTED (a format other than 0
  // with a scale other than 1), JB_ERR_GEOMETRY (a rectangle that does not lie in the image), JB_ERR_UNSUPPORTED (a
  // rectangle with a scale other than 1), JB_ERR_GEOMETRY (a target size outside 1..65535), JB_ERR_UNSUPPORTED (a target
  // size with a scale other than 1) -- in that order; with per-image rectangles, JB_ERR_GEOMETRY for the first of them
  // that does not lie in the image (bad_crop: its index) in the single rectangle's place, and JB_ERR_STATE for what is
  // no composition: no target size, or a launch-wide rectangle as well.  Behind all of these, "resampling filters":
  // JB_ERR_GEOMETRY (an unknown filter, or the target's reserved != 0), JB_ERR_STATE (a filter other than 0 without a
  // target size), JB_ERR_UNSUPPORTED (more than kJbFilterMaxTaps taps on an axis; bad_crop with per-image rectangles).
  // Behind all of these, "fit": JB_ERR_GEOMETRY (an unknown mode or anchor, a reserved field not 0), JB_ERR_STATE (a mode other than
  // JB_FIT_STRETCH without a target size), JB_ERR_UNSUPPORTED (such a mode with per-image rectangles); under such a mode the tap cap
  // above is that of src -> the inner size.  Whoever uses a plan reports it where the old code checked the
  // scale: behind the descriptor's own errors.  `why` is the text for jb_last_error (of the last plan this thread made,
  // when it names sizes); the other fields are 0 on failure (orient: 1).
  int status;
  const char *why;
  int32_t scale;          // 1, 2, 4, 8
  int32_t format;         // JB_FMT_*
  int32_t out_w, out_h;   // ceil(W / scale) x ceil(H / scale); with a rectangle, its width x height; with a target, the target
  int32_t esize;          // bytes per element
  bool planar;            // format != JB_FMT_RGB_U8_HWC: three planes of out_h rows
  int64_t row_stride;     // tight rows on the device: of a plane (out_w * esize) when planar, else 3 * out_w
  int64_t image_bytes;    // 3 * out_w * out_h * esize
  bool has_roi;           // the output is the rectangle `roi` of the full-size image (scale 1): the ROI store stage, even
  jb_roi roi;             // when the rectangle is the whole image; else all 0
  jb_output_spec spec;    // planar: the caller's spec (plane_stride, and scale / bias for the float formats); else zero
  // "fixed output size" (include/jpegblk.h): the output is the exact area resize of the src_w x src_h source -- the
  // full-size image, or the rectangle -- to out_w x out_h.  The pixel kernel writes the source as tight interleaved
  // uint8 (tmp_image_bytes per image) into a scratch of the context, jb_resample_kernel reads it.  Else all 0.
  bool has_resize;
  int32_t src_w, src_h;
  int64_t tmp_image_bytes;  // 3 * src_w * src_h
  // "resampling filters" (include/jpegblk.h): filter != JB_FILTER_AREA makes the output the Pillow-exact bilinear /
  // bicubic resize of the rectangle (has_roi: roi; else the whole frame) to out_w x out_h.  The filter reads beyond the
  // rectangle, so the pixel kernel writes `window` -- jb_filter_window: the rectangle grown by the filter's reach, clamped
  // to the frame -- and src_w, src_h, tmp_image_bytes are the WINDOW's.  With per-image rectangles the windows are per
  // image too (jb_filter_window_of_) and all four are 0.  filter 0: window is all 0.
  int32_t filter;
  jb_roi window;
  // "per-image rectangles" (include/jpegblk.h): image i of the launch is the rectangle crops[i] of its full-size decode,
  // resized to the target -- has_resize is set, has_roi is not, src_w / src_h / tmp_image_bytes are 0: the intermediate
  // of image i is 3 * crops[i].width * crops[i].height bytes.  BORROWED: the array is the caller's, and is read before
  // the call that takes the plan returns.  out_w, out_h, row_stride, image_bytes are the target's, as with one rectangle.
  const jb_roi *crops;
  int32_t n_crops;
  int32_t bad_crop;  // status == JB_ERR_GEOMETRY because of a rectangle: which one; else -1
  // "views" (include/jpegblk.h; jb_views_plan_ alone sets these): output i * views_per_image + v of the launch is the
  // rectangle views[i * views_per_image + v] of image i, resized to the target and then mirrored when its flag says so.
  // has_resize is set, crops is not, src_w / src_h / tmp_image_bytes are 0.  BORROWED like crops.  THE IMAGE STAYS THE
  // UNIT: image_bytes is that of an image's views_per_image outputs back to back (view_bytes each); out_w, out_h and
  // row_stride are one output's.  bad_crop indexes the flat array.
  const jb_view *views;
  int32_t views_per_image;  // 0: no views
  int32_t n_views;          // images * views_per_image
  int64_t view_bytes;       // 3 * out_w * out_h * esize
  // "view groups" (include/jpegblk.h; jb_view_groups_plan_ alone sets these): the views_per_image = K views of an image
  // fall into n_groups groups, group g the views [first, first + n_views) of every image under ITS target and filter.
  // THE IMAGE STILL IS THE UNIT: image_bytes is the image's block -- group 0's outputs, then group 1's, ... tight, group g
  // at `offset` -- and out_w, out_h, row_stride, view_bytes, filter and inner are group 0's.  n_groups 0: no groups.
  struct Group {
    int32_t first, n_views;  // s_g, K_g
    int32_t out_w, out_h, filter;
    int64_t row_stride;  // tight rows of one output (of a plane when planar)
    int64_t view_bytes;  // 3 * out_w * out_h * esize
    int64_t offset;      // bytes from the block's first byte to the group's first output
  };
  int32_t n_groups;
  Group groups[JB_VIEW_GROUPS_MAX];
  // "orientation" (include/jpegblk.h): the plan was made for T_o of the frame -- every field above is in oriented
  // coordinates, of the frame with width and height swapped for 5..8.  1: none.  0 (JB_ORIENT_EXIF, which only a file
  // resolves): a plan of the stored frame that no launch takes (JB_ERR_STATE where the launch is asked for).
  int32_t orient;
  // "fit" (include/jpegblk.h): out_w, out_h, row_stride and image_bytes are the TARGET's whatever the mode -- buffers,
  // arena, ring slots and copies are sized from them -- and `inner` is the rectangle of the target that the resample or
  // filter kernel produces: what a launch reads as "the size the kernel writes" is inner.width x inner.height, at
  // (inner.x, inner.y) of every output.  Without a target size, and for every mode but JB_FIT_PAD, (0, 0, out_w, out_h).
  // JB_FIT_PAD: the filter's taps, `window`, src_w, src_h and tmp_image_bytes are those of source -> inner size, and every
  // element of the target outside `inner` gets `fill` (jb_fit_fill_kernel).  JB_FIT_COVER: has_roi / roi are the derived
  // rectangle, and the plan is otherwise that of a caller who had asked for it.
  int32_t fit_mode;  // JB_FIT_*
  jb_roi inner;
  uint8_t fill[3];
  // "colour chains" (include/jpegblk.h; the _color entry points alone set it, on a plan with views): chain colors[i *
  // views_per_image + v] is applied to output (i, v) between the resample or filter kernel and the output format.  BORROWED
  // like views, parallel to it, and NOT checked by the plan: the launch reports jb_color_check's status behind the plan's
  // own.  Null: none -- the launches are those of a plan without the field.
  const jb_color_chain *colors;
};

// a target size for jb_out_plan_, and the filter that gets there (JB_FILTER_*; 0: the exact area resize).  w = h = 0 with
// a filter other than 0 says "a filter and no target": what the plan refuses with JB_ERR_STATE.
struct JbTarget {
  int32_t w, h;
  int32_t filter;
  int32_t reserved;
};

// spec: null or format 0 = interleaved uint8.  Beyond `reserved` on a format-0 spec, the spec's own fields (plane_stride
// against a row stride, finite scale / bias) are jb_output_spec_check's, which needs the caller's strides.
// roi: null = the whole image.  target: null = the size of the image (at the scale) or of the rectangle.
// orientation: JB_ORIENT_* or 2..8; desc stays the STORED frame, the plan is that of the oriented one (a value outside
// 0..8: JB_ERR_GEOMETRY, behind the scale's own check; 2..8 with a scale other than 1: JB_ERR_UNSUPPORTED, behind that).
// crops: null = none; else n_crops rectangles, one per image of the launch (n_crops < 1: nothing to check); wants a target
// and no roi.
// fit: null = JB_FIT_STRETCH; its refusals come behind every other one ("fit", include/jpegblk.h).
// the source window of one rectangle (null: the whole frame) under a plan's filter and target: what jb_filter_window
// returns, without its checks (the plan has made them)
jb_roi jb_filter_window_of_(const jb_image_desc *desc, const jb_roi *roi, int32_t out_w, int32_t out_h, int filter);
JbOutPlan jb_out_plan_(const jb_image_desc *desc, int scale, const jb_output_spec *spec, const jb_roi *roi = nullptr,
                       const JbTarget *target = nullptr, const jb_roi *crops = nullptr, int n_crops = 0, int orientation = 1,
                       const jb_fit *fit = nullptr);
// "fit": src and inner of a sw x sh source at (sx, sy) under a VALID fit (null: stretch) and the target w x h
jb_fit_geometry jb_fit_geometry_of_(const jb_roi &source, int32_t w, int32_t h, const jb_fit *fit);
// "views": the plan of n_images * views_per_image views under `rs` (null: JB_ERR_NULL) -- views_per_image, then every view's
// flags and reserved, then the rectangles, the target ("no target size": JB_ERR_STATE) and the filter, as jb_out_plan_
// checks per-image rectangles.  views may be null when there are none.
JbOutPlan jb_views_plan_(const jb_image_desc *desc, const jb_output_spec *spec, const jb_view *views, int n_images, int views_per_image,
                         const jb_resize *rs, int orientation = 1);
// "view groups": the ONE place that checks a grouped call, in the order jb_view_groups_check documents -- the counts, every
// view's flags and reserved, then every rectangle (bad_crop: the flat index i * K + v), then group by group what
// jb_views_plan_ answers for that group's views alone under groups[g].rs (the tap cap: bad_crop is still the caller's flat
// index).  The plan is group 0's with `views` the caller's flat array, views_per_image = K, the groups filled in and
// image_bytes the block.  groups is read before the call returns; views is BORROWED like jb_views_plan_'s.
JbOutPlan jb_view_groups_plan_(const jb_image_desc *desc, const jb_output_spec *spec, const jb_view *views, int n_images,
                               const jb_view_group *groups, int n_groups, int orientation = 1);
// group g of a grouped plan as a plan of its own: what jb_views_plan_ gives for that group's views, without a `views` array
JbOutPlan jb_view_group_plan_(const JbOutPlan &plan, int g);
// "draft decode" (include/jpegblk.h): the descriptor a plan under draft `denom` (1, 2, 4, 8) is made from -- desc with
// the DRAFT FRAME's width and height; everything that addresses coefficients keeps the true descriptor.  denom 1: desc.
jb_image_desc jb_draft_desc_(const jb_image_desc *desc, int denom);
// why a draft other than 1 does not go with this arithmetic (JB_ARITH_*), scale and orientation: the text of the
// JB_ERR_UNSUPPORTED refusal, or null when it does (draft 1: always)
const char *jb_draft_refusal_(int draft, int arith, int scale, int orientation);
#define kJbDraftArithText "a draft other than 1 needs JB_ARITH_LIBJPEG"
#define kJbDraftScaleText "a draft other than 1 cannot be combined with a scale other than 1"
#define kJbDraftOrientText "a draft other than 1 cannot be combined with an orientation other than JB_ORIENT_STORED"
// "orientation": the refusal of a plan with orient == 0 at a launch, and of a scale with an orientation
#define kJbOrientExifText "JB_ORIENT_EXIF takes the orientation from a file: this entry point has none (set 1..8)"
#define kJbOrientScaleText "an orientation other than 1 cannot be combined with a scale other than 1"
