// jb_geometry.cpp -- the host-only arithmetic of the ABI (include/jpegblk.h): frame geometry and
// quantisation-table resolution.  No HIP dependency, so the front end can be built and fuzzed on
// a CPU-only toolchain with sanitizers (tools/fuzz/).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_filter.h"
#include "jb_orient.h"
#include "jb_plan.h"

extern "C" {

// read_sof's derivations, reference jpeg.cpp:77-80 (block counts) and 110-127 (sampling checks,
// padding of odd block counts when the luma factor is 2)
int jb_geometry_of(const jb_image_desc *d, jb_geometry *g) {
  if (!d || !g) return JB_ERR_NULL;
  if (d->width < 1 || d->height < 1 || d->width > 65535 || d->height > 65535) return JB_ERR_GEOMETRY;
  if ((d->hs != 1 && d->hs != 2) || (d->vs != 1 && d->vs != 2)) return JB_ERR_SAMPLING;
  for (int i = 0; i < 3; i++)
    if (d->qtab_id[i] < 0 || d->qtab_id[i] > 3) return JB_ERR_QTAB;
  memset(g, 0, sizeof *g);
  g->mcu_w = (d->width + 7) / 8;
  g->mcu_h = (d->height + 7) / 8;
  g->mcu_w_real = g->mcu_w + ((d->hs == 2 && (g->mcu_w & 1)) ? 1 : 0);
  g->mcu_h_real = g->mcu_h + ((d->vs == 2 && (g->mcu_h & 1)) ? 1 : 0);
  g->mcus_x = g->mcu_w_real / d->hs;
  g->mcus_y = g->mcu_h_real / d->vs;
  g->blocks_per_mcu = d->hs * d->vs + 2;
  g->n_coded_blocks = (int64_t)g->mcus_x * g->mcus_y * g->blocks_per_mcu;
  g->coef_bytes = g->n_coded_blocks * 128;
  g->rgb_bytes = (int64_t)d->width * d->height * 3;
  return JB_OK;
}

// "flat front end": workgroup t of a launch reads its tile at img * stride + (my * mcus_x + mx0) * 384, (img, my, mx0) its
// image, MCU row and first MCU.  That is t * 24576 for every t exactly when no tile is short -- a row-bound tile ends with
// its MCU row, a linear one with its image -- and the images are as far apart as their tiles are long; one image has no
// distance to the next.  4:4:4 only: the layout whose tile is 64 MCUs of three blocks (jb_kernels.hip).
int jb_flat_front_geometry(int hs, int vs, int linear, int32_t mcus_x, int32_t mcus_y, int32_t n_images, int64_t coef_image_stride) {
  if (hs != 1 || vs != 1 || mcus_x < 1 || mcus_y < 1 || n_images < 1) return 0;
  constexpr int64_t kTileMcus = 64, kTileBytes = kTileMcus * 3 * 128;
  const int64_t mcus = (int64_t)mcus_x * mcus_y;
  if (linear ? mcus % kTileMcus != 0 : mcus_x % kTileMcus != 0) return 0;
  return n_images == 1 || coef_image_stride == mcus / kTileMcus * kTileBytes;
}

int jb_scaled_size(int32_t width, int32_t height, int denom, int32_t *out_w, int32_t *out_h) {
  if (!out_w || !out_h) return JB_ERR_NULL;
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return JB_ERR_GEOMETRY;
  if (width < 1 || height < 1 || width > 65535 || height > 65535) return JB_ERR_GEOMETRY;
  *out_w = (width + denom - 1) / denom;
  *out_h = (height + denom - 1) / denom;
  return JB_OK;
}

// "draft decode": jdmaster.c's block sizes and what is left to jdsample.c
int jb_draft_geometry_of(const jb_image_desc *d, int denom, jb_draft_geometry *out) {
  if (!d || !out) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc) return rc;
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return JB_ERR_GEOMETRY;
  memset(out, 0, sizeof *out);
  const int s = 8 / denom;
  int sc = s;
  while (sc < 8 && (d->hs * s) % (2 * sc) == 0 && (d->vs * s) % (2 * sc) == 0) sc *= 2;
  out->width = (d->width + denom - 1) / denom;
  out->height = (d->height + denom - 1) / denom;
  out->luma_block = s, out->chroma_block = sc;
  out->up_h = d->hs * s / sc, out->up_v = d->vs * s / sc;
  out->fancy = s > 1 ? 1 : 0;
  return JB_OK;
}

// bytes per element of an output format (0: not a format)
static int jb_format_esize_(int format) {
  return format == JB_FMT_RGB_U8_HWC || format == JB_FMT_RGB_U8_CHW ? 1 : format == JB_FMT_RGB_F32_CHW ? 4 : format == JB_FMT_RGB_F16_CHW ? 2 : 0;
}

int jb_output_bytes(int32_t width, int32_t height, int format, int64_t *bytes) {
  if (!bytes) return JB_ERR_NULL;
  jb_image_desc d;
  jb_output_spec s;
  memset(&d, 0, sizeof d);
  memset(&s, 0, sizeof s);
  d.width = width, d.height = height;
  s.format = format;
  const JbOutPlan plan = jb_out_plan_(&d, 1, &s);  // an unknown format or a size outside 1..65535: JB_ERR_GEOMETRY
  if (plan.status != JB_OK) return plan.status;
  *bytes = plan.image_bytes;
  return JB_OK;
}

int jb_output_spec_check(const jb_output_spec *s, int32_t height, int64_t row_stride) {
  if (!s) return JB_ERR_NULL;
  if (jb_format_esize_(s->format) == 0 || s->reserved != 0) return JB_ERR_GEOMETRY;
  if (s->format == JB_FMT_RGB_U8_HWC) return JB_OK;  // (the other fields are not looked at)
  if (height < 1 || height > 65535 || row_stride < 1) return JB_ERR_GEOMETRY;
  if (s->plane_stride != 0 && s->plane_stride < row_stride * (int64_t)height) return JB_ERR_GEOMETRY;
  if (s->format != JB_FMT_RGB_U8_CHW)
    for (int c = 0; c < 3; c++) {
      // finite: the exponent field is not all ones (tested on the bits)
      uint32_t a, b;
      memcpy(&a, &s->scale[c], 4);
      memcpy(&b, &s->bias[c], 4);
      if ((a & 0x7f800000u) == 0x7f800000u || (b & 0x7f800000u) == 0x7f800000u) return JB_ERR_GEOMETRY;
    }
  return JB_OK;
}

// does the rectangle lie in a W x H image?  (64-bit sums: x = INT32_MAX is refused, not wrapped)
static bool jb_roi_fits_(const jb_roi *r, int32_t width, int32_t height) {
  return r->x >= 0 && r->y >= 0 && r->width >= 1 && r->height >= 1 && (int64_t)r->x + r->width <= width &&
         (int64_t)r->y + r->height <= height;
}

int jb_roi_check(const jb_image_desc *d, const jb_roi *roi) {
  if (!d || !roi) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  return jb_roi_fits_(roi, d->width, d->height) ? JB_OK : JB_ERR_GEOMETRY;
}

int jb_resize_check(const jb_image_desc *d, const jb_roi *roi, int32_t out_w, int32_t out_h) {
  if (!d) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  const JbTarget t = {out_w, out_h};
  return jb_out_plan_(d, 1, nullptr, roi, &t).status;  // the rectangle first, then the target
}

int jb_crops_check(const jb_image_desc *d, const jb_roi *rois, int n, int32_t out_w, int32_t out_h, int *bad_index) {
  if (bad_index) *bad_index = -1;
  if (!d || (!rois && n > 0)) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  if (n < 0) return JB_ERR_GEOMETRY;
  const JbTarget t = {out_w, out_h};
  static const jb_roi none = {0, 0, 0, 0};
  const JbOutPlan plan = jb_out_plan_(d, 1, nullptr, nullptr, &t, rois ? rois : &none, n);  // the rectangles first, then the target
  if (bad_index) *bad_index = plan.bad_crop;
  return plan.status;
}

int jb_views_check(const jb_image_desc *d, const jb_view *views, int n_images, int views_per_image, const jb_resize *rs, int *bad_index) {
  if (bad_index) *bad_index = -1;
  if (!d || !rs || (!views && n_images > 0 && views_per_image > 0)) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  const JbOutPlan plan = jb_views_plan_(d, nullptr, views, n_images, views_per_image, rs);
  if (bad_index) *bad_index = plan.bad_crop;
  return plan.status;
}

int jb_view_groups_check(const jb_image_desc *d, const jb_view *views, int n_images, const jb_view_group *groups, int n_groups, int *bad_index) {
  if (bad_index) *bad_index = -1;
  if (!d || !groups || (!views && n_images > 0)) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  const JbOutPlan plan = jb_view_groups_plan_(d, nullptr, views, n_images, groups, n_groups);
  if (bad_index) *bad_index = plan.bad_crop;
  return plan.status;
}

int jb_view_groups_bytes(const jb_view_group *groups, int n_groups, int format, int64_t *group_offsets, int64_t *image_bytes) {
  if (!groups || !image_bytes) return JB_ERR_NULL;
  if (n_groups < 1 || n_groups > JB_VIEW_GROUPS_MAX) return JB_ERR_GEOMETRY;
  int64_t at = 0, k = 0;
  for (int g = 0; g < n_groups; g++) {
    if (groups[g].n_views < 1 || groups[g].reserved != 0) return JB_ERR_GEOMETRY;
    k += groups[g].n_views;
  }
  if (k > JB_VIEWS_MAX) return JB_ERR_GEOMETRY;
  int64_t offsets[JB_VIEW_GROUPS_MAX];
  for (int g = 0; g < n_groups; g++) {
    int64_t one = 0;
    const int rc = jb_output_bytes(groups[g].rs.out_w, groups[g].rs.out_h, format, &one);
    if (rc != JB_OK) return rc;
    offsets[g] = at;
    at += one * groups[g].n_views;
  }
  if (group_offsets) memcpy(group_offsets, offsets, sizeof(int64_t) * (size_t)n_groups);
  *image_bytes = at;
  return JB_OK;
}

int jb_filter_check(const jb_image_desc *d, const jb_roi *roi, const jb_resize *rs) {
  if (!d || !rs) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  const JbTarget t = {rs->out_w, rs->out_h, rs->filter, rs->reserved};
  return jb_out_plan_(d, 1, nullptr, roi, &t).status;  // the rectangle, the target, then the filter
}

int jb_filter_window(const jb_image_desc *d, const jb_roi *roi, const jb_resize *rs, jb_roi *window) {
  if (!window) return JB_ERR_NULL;
  const int rc = jb_filter_check(d, roi, rs);
  if (rc != JB_OK) return rc;
  const jb_roi whole = {0, 0, d->width, d->height};
  *window = rs->filter == JB_FILTER_AREA ? (roi ? *roi : whole) : jb_filter_window_of_(d, roi, rs->out_w, rs->out_h, rs->filter);
  return JB_OK;
}

int jb_fit_check(const jb_image_desc *d, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit, jb_fit_geometry *out) {
  if (!d || !rs) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  const JbTarget t = {rs->out_w, rs->out_h, rs->filter, rs->reserved};
  const JbOutPlan plan = jb_out_plan_(d, 1, nullptr, roi, &t, nullptr, 0, 1, fit);  // the rectangle, the target, the filter, then the fit
  if (plan.status != JB_OK) return plan.status;
  if (out) {
    const jb_roi whole = {0, 0, d->width, d->height};
    out->src = plan.has_roi ? plan.roi : whole;
    out->inner = plan.inner;
  }
  return JB_OK;
}

int jb_oriented_size(int32_t w, int32_t h, int o, int32_t *ow, int32_t *oh) {
  if (!ow || !oh) return JB_ERR_NULL;
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || o < 1 || o > 8) return JB_ERR_GEOMETRY;
  const bool swap = jb_orient_bits(o).transpose != 0;
  *ow = swap ? h : w, *oh = swap ? w : h;
  return JB_OK;
}

int jb_orient_map_roi(int32_t w, int32_t h, int o, const jb_roi *r, jb_roi *stored) {
  if (!r || !stored) return JB_ERR_NULL;
  int32_t ow, oh;
  const int rc = jb_oriented_size(w, h, o, &ow, &oh);
  if (rc != JB_OK) return rc;
  if (!jb_roi_fits_(r, ow, oh)) return JB_ERR_GEOMETRY;
  // jb_orient.h: u runs along the stored rows' index (y), v along the stored columns' (x)
  const JbOrientBits b = jb_orient_bits(o);
  const int32_t u0 = b.transpose ? r->x : r->y, ul = b.transpose ? r->width : r->height;
  const int32_t v0 = b.transpose ? r->y : r->x, vl = b.transpose ? r->height : r->width;
  *stored = jb_roi{b.flip_x ? w - v0 - vl : v0, b.flip_y ? h - u0 - ul : u0, vl, ul};
  return JB_OK;
}

int jb_orient_check(const jb_image_desc *d, int orientation, int scale, const jb_roi *roi) {
  if (!d) return JB_ERR_NULL;
  jb_geometry g;
  const int rc = jb_geometry_of(d, &g);
  if (rc != JB_OK) return rc;
  return jb_out_plan_(d, scale, nullptr, roi, nullptr, nullptr, 0, orientation).status;
}

int jb_resolve_qtabs(const jb_image_desc *d, const uint16_t *qtabs, int32_t *out192) {
  if (!d || !qtabs || !out192) return JB_ERR_NULL;
  for (int c = 0; c < 3; c++) {
    if (d->qtab_id[c] < 0 || d->qtab_id[c] > 3) return JB_ERR_QTAB;
    // the table each component names (reference jpeg.cpp:584), natural order
    for (int i = 0; i < 64; i++) out192[c * 64 + i] = qtabs[d->qtab_id[c] * 64 + i];
  }
  return JB_OK;
}

}  // extern "C"

jb_image_desc jb_draft_desc_(const jb_image_desc *d, int denom) {
  jb_image_desc draft = *d;
  if (denom == 2 || denom == 4 || denom == 8) {
    draft.width = (d->width + denom - 1) / denom;
    draft.height = (d->height + denom - 1) / denom;
  }
  return draft;
}

const char *jb_draft_refusal_(int draft, int arith, int scale, int orientation) {
  if (draft == 1) return nullptr;
  if (arith != JB_ARITH_LIBJPEG) return kJbDraftArithText;
  if (scale != 1) return kJbDraftScaleText;
  if (orientation != JB_ORIENT_STORED) return kJbDraftOrientText;
  return nullptr;
}

jb_roi jb_filter_window_of_(const jb_image_desc *d, const jb_roi *roi, int32_t out_w, int32_t out_h, int filter) {
  const jb_roi whole = {0, 0, d->width, d->height};
  const jb_roi &r = roi ? *roi : whole;
  int x0, x1, y0, y1;
  jb_filter_span(jb_filter_axis(filter, d->width, r.x, r.x + r.width, out_w), out_w, &x0, &x1);
  jb_filter_span(jb_filter_axis(filter, d->height, r.y, r.y + r.height, out_h), out_h, &y0, &y1);
  return jb_roi{x0, y0, x1 - x0, y1 - y0};
}

// "fit" (include/jpegblk.h): PAD is Pillow's ImageOps.pad / contain on doubles, operation for operation (the build keeps
// every operation separate: -ffp-contract=off; rint rounds halves to even, as Python's round); COVER is integers only
jb_fit_geometry jb_fit_geometry_of_(const jb_roi &s, int32_t w, int32_t h, const jb_fit *fit) {
  jb_fit_geometry g = {s, jb_roi{0, 0, w, h}};
  const int mode = fit ? fit->mode : JB_FIT_STRETCH, anchor = fit ? fit->anchor : JB_FIT_CENTER;
  const auto offset = [anchor](int64_t d, bool halves_even) -> int32_t {
    if (anchor == JB_FIT_START) return 0;
    if (anchor == JB_FIT_END) return (int32_t)d;
    return halves_even ? (int32_t)std::rint((double)d * 0.5) : (int32_t)(d / 2);
  };
  const auto clamp = [](int64_t v, int64_t hi) { return (int32_t)(v < 1 ? 1 : v > hi ? hi : v); };
  if (mode == JB_FIT_PAD) {
    const double sw = (double)s.width, sh = (double)s.height;
    const double ir = sw / sh, dr = (double)w / (double)h;
    if (ir == dr) return g;
    if (ir > dr) {
      const int32_t dh = clamp((int64_t)std::rint(sh / sw * (double)w), h);
      g.inner = jb_roi{0, offset(h - dh, true), w, dh};
    } else {
      const int32_t dw = clamp((int64_t)std::rint(sw / sh * (double)h), w);
      g.inner = jb_roi{offset(w - dw, true), 0, dw, h};
    }
  } else if (mode == JB_FIT_COVER) {
    const int64_t sw = s.width, sh = s.height, a = sw * h, b = sh * w;
    if (a > b) {
      const int32_t cw = clamp((2 * sh * w + h) / (2 * (int64_t)h), sw);
      g.src = jb_roi{s.x + offset(sw - cw, false), s.y, cw, s.height};
    } else if (a < b) {
      const int32_t ch = clamp((2 * sw * h + w) / (2 * (int64_t)w), sh);
      g.src = jb_roi{s.x, s.y + offset(sh - ch, false), s.width, ch};
    }
  }
  return g;
}

JbOutPlan jb_views_plan_(const jb_image_desc *d, const jb_output_spec *spec, const jb_view *views, int n_images, int k, const jb_resize *rs,
                         int orientation) {
  JbOutPlan p;
  memset(&p, 0, sizeof p);
  p.bad_crop = -1;
  p.orient = 1;
  auto refuse = [&p](int status, const char *why, int bad = -1) {
    memset(&p, 0, sizeof p);
    p.orient = 1;
    p.status = status, p.why = why, p.bad_crop = bad;
    return p;
  };
  if (!d || !rs) return refuse(JB_ERR_NULL, "null descriptor or jb_resize");
  if (n_images < 0) return refuse(JB_ERR_GEOMETRY, "negative count");
  if (k < 1 || k > JB_VIEWS_MAX) return refuse(JB_ERR_GEOMETRY, "views_per_image is outside 1..16");
  const int64_t n = (int64_t)n_images * k;
  if (n > 0 && !views) return refuse(JB_ERR_NULL, "views is NULL");
  if (n > 0x7fffffffLL) return refuse(JB_ERR_CAPACITY, "too many views");
  static thread_local char text[224];
  std::vector<jb_roi> rects((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const jb_view &v = views[i];
    if ((v.flags & ~JB_VIEW_MIRROR) != 0 || v.reserved != 0) {
      snprintf(text, sizeof text, "image %d, view %d: unknown flag bits (or reserved is not 0)", (int)(i / k), (int)(i % k));
      return refuse(JB_ERR_GEOMETRY, text, (int)i);
    }
    rects[(size_t)i] = jb_roi{v.x, v.y, v.width, v.height};
  }
  // the rectangles, the target and the filter: exactly the checks of per-image rectangles, in their order
  static const jb_roi none = {0, 0, 0, 0};
  const bool no_target = rs->out_w == 0 && rs->out_h == 0;
  // ("no target size" is JB_ERR_STATE whatever the filter: a filter of 1 makes the plan say so where the target is checked)
  const JbTarget t = {rs->out_w, rs->out_h, no_target && rs->filter == JB_FILTER_AREA ? JB_FILTER_BILINEAR : rs->filter, rs->reserved};
  p = jb_out_plan_(d, 1, spec, nullptr, &t, n > 0 ? rects.data() : &none, (int)n, orientation);
  if (p.status != JB_OK) {
    const int bad = p.bad_crop;
    if (bad >= 0 && p.status == JB_ERR_GEOMETRY) {
      const jb_view &v = views[bad];
      const bool swap = jb_orient_bits(orientation).transpose != 0;
      snprintf(text, sizeof text, "image %d, view %d: the rectangle %d x %d at (%d, %d) does not lie in the %d x %d image", bad / k, bad % k,
               v.width, v.height, v.x, v.y, swap ? d->height : d->width, swap ? d->width : d->height);
      return refuse(JB_ERR_GEOMETRY, text, bad);
    }
    return refuse(p.status, p.why, bad);
  }
  p.crops = nullptr, p.n_crops = 0;  // (rects ends here: the launch reads the views)
  p.views = views, p.views_per_image = k, p.n_views = (int32_t)n;
  p.view_bytes = p.image_bytes;
  p.image_bytes = p.view_bytes * k;
  return p;
}

JbOutPlan jb_view_groups_plan_(const jb_image_desc *d, const jb_output_spec *spec, const jb_view *views, int n_images, const jb_view_group *groups,
                               int n_groups, int orientation) {
  JbOutPlan p;
  auto refuse = [&p](int status, const char *why, int bad = -1) {
    memset(&p, 0, sizeof p);
    p.orient = 1;
    p.status = status, p.why = why, p.bad_crop = bad;
    return p;
  };
  if (!d || !groups) return refuse(JB_ERR_NULL, "null descriptor or groups");
  if (n_images < 0) return refuse(JB_ERR_GEOMETRY, "negative count");
  if (n_groups < 1 || n_groups > JB_VIEW_GROUPS_MAX) return refuse(JB_ERR_GEOMETRY, "n_groups is outside 1..4");
  int64_t k = 0;
  for (int g = 0; g < n_groups; g++) {
    if (groups[g].n_views < 1 || groups[g].reserved != 0) return refuse(JB_ERR_GEOMETRY, "a group's n_views is below 1 (or its reserved is not 0)");
    k += groups[g].n_views;
  }
  if (k > JB_VIEWS_MAX) return refuse(JB_ERR_GEOMETRY, "the groups' views per image add up to more than 16");
  // every view in flat order -- flags and reserved, then the rectangles: the views' plan under a target nothing refuses
  const jb_resize any = {1, 1, JB_FILTER_AREA, 0};
  p = jb_views_plan_(d, spec, views, n_images, (int)k, &any, orientation);
  if (p.status != JB_OK) return p;
  JbOutPlan out = p;
  std::vector<jb_view> mine;
  int32_t first = 0;
  int64_t offset = 0;
  for (int g = 0; g < n_groups; g++) {
    const int kg = groups[g].n_views;
    mine.resize((size_t)n_images * (size_t)kg);
    for (int64_t i = 0; i < n_images; i++)
      for (int v = 0; v < kg; v++) mine[(size_t)(i * kg + v)] = views[i * k + first + v];
    p = jb_views_plan_(d, spec, mine.data(), n_images, kg, &groups[g].rs, orientation);
    if (p.status != JB_OK) return refuse(p.status, p.why, p.bad_crop < 0 ? -1 : (int)((p.bad_crop / kg) * k + first + p.bad_crop % kg));
    if (g == 0) {
      out = p;
      out.views = views, out.views_per_image = (int32_t)k, out.n_views = (int32_t)(n_images * k);
    }
    out.groups[g] = JbOutPlan::Group{first, kg, p.out_w, p.out_h, p.filter, p.row_stride, p.view_bytes, offset};
    first += kg;
    offset += p.view_bytes * kg;
  }
  out.n_groups = n_groups;
  out.image_bytes = offset;
  return out;
}

JbOutPlan jb_view_group_plan_(const JbOutPlan &plan, int g) {
  JbOutPlan p = plan;
  const JbOutPlan::Group &q = plan.groups[g];
  p.n_groups = 0;
  memset(p.groups, 0, sizeof p.groups);
  p.views = nullptr;
  p.views_per_image = q.n_views;
  p.n_views = plan.views_per_image > 0 ? plan.n_views / plan.views_per_image * q.n_views : 0;
  p.out_w = q.out_w, p.out_h = q.out_h, p.filter = q.filter;
  p.inner = jb_roi{0, 0, q.out_w, q.out_h};
  p.row_stride = q.row_stride;
  p.view_bytes = q.view_bytes;
  p.image_bytes = q.view_bytes * q.n_views;
  return p;
}

// jb_plan.h: the only place that turns (frame, scale, spec, rectangle, target) into the output's sizes and strides
JbOutPlan jb_out_plan_(const jb_image_desc *d, int scale, const jb_output_spec *spec, const jb_roi *roi, const JbTarget *target,
                       const jb_roi *crops, int n_crops, int orientation, const jb_fit *fit) {
  JbOutPlan p;
  memset(&p, 0, sizeof p);
  p.bad_crop = -1;
  p.orient = 1;
  auto refuse = [&p](int status, const char *why) {
    p.status = status, p.why = why;
    return p;
  };
  if (!d) return refuse(JB_ERR_NULL, "null descriptor");
  // "fit": a fit that is none is refused behind everything else, and is a stretch until then
  const bool fit_bad = fit && (fit->mode < JB_FIT_STRETCH || fit->mode > JB_FIT_COVER || fit->anchor < JB_FIT_CENTER || fit->anchor > JB_FIT_END ||
                               fit->reserved8 != 0 || fit->reserved != 0);
  const int fit_mode = fit && !fit_bad ? fit->mode : JB_FIT_STRETCH;
  jb_roi inner = {0, 0, 0, 0}, cover = {0, 0, 0, 0};
  int32_t out_w = 0, out_h = 0;
  if (jb_scaled_size(d->width, d->height, scale, &out_w, &out_h) != JB_OK)
    return refuse(JB_ERR_GEOMETRY, "scale is not 1, 2, 4 or 8 (or the image size is outside 1..65535)");
  // "orientation": everything below sees the oriented frame
  if (orientation < 0 || orientation > 8) return refuse(JB_ERR_GEOMETRY, "orientation is outside 0..8");
  if (orientation > 1 && scale != 1) return refuse(JB_ERR_UNSUPPORTED, kJbOrientScaleText);  // (0: JB_ERR_STATE at the launch, or the file decides)
  jb_image_desc oriented;
  if (jb_orient_bits(orientation).transpose) {
    oriented = *d;
    oriented.width = d->height, oriented.height = d->width;
    d = &oriented;
    const int32_t t = out_w;
    out_w = out_h, out_h = t;
  }
  if (spec && spec->format == JB_FMT_RGB_U8_HWC) {
    if (spec->reserved != 0) return refuse(JB_ERR_GEOMETRY, "output spec: reserved must be 0");
    spec = nullptr;  // (the other fields are not looked at)
  }
  const int esize = spec ? jb_format_esize_(spec->format) : 1;
  if (esize == 0) return refuse(JB_ERR_GEOMETRY, "unknown output format");
  if (spec && scale != 1) return refuse(JB_ERR_UNSUPPORTED, "a planar output format cannot be combined with a scale");
  if (roi) {
    if (!jb_roi_fits_(roi, d->width, d->height)) {
      static thread_local char text[160];
      snprintf(text, sizeof text, "the rectangle %d x %d at (%d, %d) does not lie in the %d x %d image", roi->width, roi->height,
               roi->x, roi->y, d->width, d->height);
      return refuse(JB_ERR_GEOMETRY, text);
    }
    if (scale != 1) return refuse(JB_ERR_UNSUPPORTED, "a rectangle cannot be combined with a scale");
    out_w = roi->width, out_h = roi->height;
    p.has_roi = true, p.roi = *roi;
  }
  if (crops) {
    // two rectangles for one image is a mistake, not a composition; and only a target makes the outputs one size
    if (roi) {
      p.has_roi = false, p.roi = jb_roi{};
      return refuse(JB_ERR_STATE, "per-image rectangles cannot be combined with a rectangle for every image");
    }
    if (!target) return refuse(JB_ERR_STATE, "per-image rectangles want a target size");
    for (int i = 0; i < n_crops; i++)
      if (!jb_roi_fits_(&crops[i], d->width, d->height)) {
        static thread_local char text[192];
        snprintf(text, sizeof text, "image %d: the rectangle %d x %d at (%d, %d) does not lie in the %d x %d image", i, crops[i].width,
                 crops[i].height, crops[i].x, crops[i].y, d->width, d->height);
        p.bad_crop = i;
        return refuse(JB_ERR_GEOMETRY, text);
      }
    if (scale != 1) return refuse(JB_ERR_UNSUPPORTED, "a rectangle cannot be combined with a scale");
    out_w = out_h = 0;  // (the source size is per image)
  }
  if (target) {
    auto refuse_target = [&](int status, const char *why) {
      p.has_roi = false, p.roi = jb_roi{};
      return refuse(status, why);
    };
    // "a filter and no target size", "a fit and no target size"
    const bool no_target = target->w == 0 && target->h == 0 && (target->filter != 0 || fit_mode != JB_FIT_STRETCH);
    if (!no_target && (target->w < 1 || target->h < 1 || target->w > 65535 || target->h > 65535))
      return refuse_target(JB_ERR_GEOMETRY, "the target size is outside 1..65535");
    if (scale != 1) return refuse_target(JB_ERR_UNSUPPORTED, "a target size cannot be combined with a scale");
    if (target->filter < JB_FILTER_AREA || target->filter > JB_FILTER_BICUBIC || target->reserved != 0)
      return refuse_target(JB_ERR_GEOMETRY, "unknown resampling filter (or reserved is not 0)");
    if (no_target)
      return refuse_target(JB_ERR_STATE, target->filter != 0 ? "a resampling filter wants a target size" : "a fit other than JB_FIT_STRETCH wants a target size");
    // "fit": what is resampled is src -> the inner size (with per-image rectangles the fit is refused below)
    inner = jb_roi{0, 0, target->w, target->h};
    if (fit_mode != JB_FIT_STRETCH && !crops) {
      const jb_roi whole = {0, 0, d->width, d->height};
      const jb_fit_geometry fg = jb_fit_geometry_of_(roi ? *roi : whole, target->w, target->h, fit);
      inner = fg.inner;
      if (fit_mode == JB_FIT_COVER) {  // an ordinary plan of the derived rectangle
        cover = fg.src;
        roi = &cover;
        p.has_roi = true, p.roi = cover;
        out_w = cover.width, out_h = cover.height;
      }
    }
    if (target->filter != JB_FILTER_AREA) {
      // the taps of both axes against the kernel's cap, for the one rectangle or for every image's
      const jb_roi whole = {0, 0, d->width, d->height};
      const jb_roi *rects = crops ? crops : roi ? roi : &whole;
      const int n_rects = crops ? n_crops : 1;
      for (int i = 0; i < n_rects; i++) {
        const jb_roi &r = rects[i];
        const int tx = jb_filter_taps(jb_filter_axis(target->filter, d->width, r.x, r.x + r.width, inner.width));
        const int ty = jb_filter_taps(jb_filter_axis(target->filter, d->height, r.y, r.y + r.height, inner.height));
        if (tx > kJbFilterMaxTaps || ty > kJbFilterMaxTaps) {
          static thread_local char text[192];
          snprintf(text, sizeof text, "the reduction of the %d x %d rectangle to %d x %d wants %d x %d filter taps: more than the cap of %d per axis",
                   r.width, r.height, inner.width, inner.height, tx, ty, kJbFilterMaxTaps);
          if (crops) p.bad_crop = i;
          return refuse_target(JB_ERR_UNSUPPORTED, text);
        }
      }
      p.filter = target->filter;
    }
    p.has_resize = true;
    if (crops) p.crops = crops, p.n_crops = n_crops;
    if (p.filter != JB_FILTER_AREA && !crops) {
      p.window = jb_filter_window_of_(d, roi, inner.width, inner.height, p.filter);
      out_w = p.window.width, out_h = p.window.height;
    }
    p.src_w = out_w, p.src_h = out_h;
    p.tmp_image_bytes = 3LL * out_w * out_h;
    out_w = target->w, out_h = target->h;
  }
  if (fit_bad || (fit_mode != JB_FIT_STRETCH && (!target || crops))) {
    memset(&p, 0, sizeof p);
    p.bad_crop = -1;
    p.orient = 1;
    if (fit_bad) return refuse(JB_ERR_GEOMETRY, "fit: unknown mode or anchor (or a reserved field is not 0)");
    if (!target) return refuse(JB_ERR_STATE, "a fit other than JB_FIT_STRETCH wants a target size");
    return refuse(JB_ERR_UNSUPPORTED, "a fit other than JB_FIT_STRETCH cannot be combined with per-image rectangles or views");
  }
  p.fit_mode = fit_mode;
  p.inner = target ? inner : jb_roi{0, 0, out_w, out_h};
  if (fit_mode == JB_FIT_PAD) memcpy(p.fill, fit->fill, 3);
  p.why = "";
  p.orient = orientation;
  p.scale = scale;
  p.out_w = out_w, p.out_h = out_h;
  p.esize = esize;
  p.planar = spec != nullptr;
  if (spec) p.format = spec->format, p.spec = *spec;
  p.row_stride = p.planar ? (int64_t)out_w * esize : 3LL * out_w;
  p.image_bytes = 3LL * out_w * out_h * esize;  // at most 3 * 65535^2 * 4 < 2^36
  return p;
}
