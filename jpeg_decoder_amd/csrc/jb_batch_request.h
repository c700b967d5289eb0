// jb_batch_request.h -- what a batch decoder is asked for: the output request of the decoder (OutputRequest), what a run
// has per file next to its path (PerFile), and their rules, each ONCE: which requests can be had, which plan function a
// file or a group gets, what a run checks in front of its first file.  Host-only and header-only, without a decoder or
// a thread in it: jb_batch.cpp and jb_batch_run.cpp include it, and tools/fuzz/batch_request_check.cpp walks the rules
// on the CPU.  A new per-file option is a field of PerFile, a line of PerFile::plan / check, a builder and a vector of
// PerFileOwned -- all in this file.
#pragma once
#include <string>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_internal.h"
#include "jb_plan.h"

// a status and the text that goes with it (JB_OK: none)
struct JbVerdict {
  int status;
  const char *why;
};

// What a decoder has been asked to deliver (jb_batch_decoder_set_scale, jb_batch_decoder_set_output_format,
// jb_batch_decoder_set_roi, jb_batch_decoder_set_resize): ONE value on the decoder, copied to its parts, its twin and every
// run.  Never a format other than 0, a rectangle or a target size with a scale other than 1.
struct OutputRequest {
  int scale = 1;
  jb_output_spec spec = {};  // format 0: interleaved uint8
  bool has_roi = false;      // one rectangle for every image
  jb_roi roi = {};
  const jb_roi *roi_ptr() const { return has_roi ? &roi : nullptr; }
  bool has_resize = false;   // one output size for every image
  JbTarget target = {};      // (target.filter: always the decoder's filter, with or without a target size)
  const JbTarget *target_ptr() const { return has_resize ? &target : nullptr; }
  int arith = JB_ARITH_REFERENCE;  // "decoder arithmetic": what the decoder's contexts compute in (never LIBJPEG with a scale)
  int orient = JB_ORIENT_STORED;   // "orientation": JB_ORIENT_* or 2..8 (never another value than 1 with a scale)
  int draft = 1;                   // "draft decode": 1, 2, 4, 8 (never another value than 1 without LIBJPEG, with a scale or an orientation)
  jb_fit fit = {};                 // "fit": a valid one; JB_FIT_STRETCH: none.  Kept, like the filter, while no target size is set
  const jb_fit *fit_ptr() const { return fit.mode != JB_FIT_STRETCH ? &fit : nullptr; }
  // THE rule: can this request be had, and why not?  First the pairs that no plan sees, in a fixed order (a setter
  // changes one field of a request that could be had, so only pairs with that field can fire), then the plan function
  // (jb_plan.h), here for an image of one pixel -- with a rectangle, for the largest frame there is (JB_ERR_GEOMETRY: no
  // frame holds the rectangle).  combined / other: the caller's own words for the plan's JB_ERR_UNSUPPORTED (something
  // with a scale) and for its other refusals; null: the plan's.
  JbVerdict verdict(const char *combined = nullptr, const char *other = nullptr) const {
    if (scale != 1 && arith == JB_ARITH_LIBJPEG) return {JB_ERR_UNSUPPORTED, kJbArithScaleText};
    if (scale != 1 && orient != JB_ORIENT_STORED) return {JB_ERR_UNSUPPORTED, kJbOrientScaleText};
    if (const char *why = jb_draft_refusal_(draft, arith, scale, orient)) return {JB_ERR_UNSUPPORTED, why};  // arithmetic, scale, orientation
    const int32_t n = has_roi ? 65535 : 1;
    const jb_image_desc one = {n, n, 1, 1, {0, 0, 0}, 0};
    JbTarget sized = target;  // (without the filter: its tap cap is a matter of every file's own frame)
    sized.filter = 0;
    const JbOutPlan plan = jb_out_plan_(&one, scale, &spec, roi_ptr(), has_resize ? &sized : nullptr);
    if (plan.status == JB_ERR_UNSUPPORTED && combined) return {plan.status, combined};
    if (plan.status != JB_OK && other) return {plan.status, other};
    return {plan.status, plan.why};
  }
};

// what a run has per FILE next to its path: a rectangle ("per-image rectangles": rois[i]), or k views ("views":
// views[i * k + v]); neither: a plain run
struct PerFile {
  const jb_roi *rois = nullptr;
  const jb_view *views = nullptr;
  int k = 0;
  // "view groups" (_run_view_groups): the k views of a file fall into n_groups groups, each with its own target and filter
  // (by value: the same for every file, every part of a multi-device decoder and both sides of submit / collect); 0: none
  jb_view_group groups[JB_VIEW_GROUPS_MAX] = {};
  int n_groups = 0;
  const jb_roi *roi_of(int i) const { return rois ? &rois[i] : nullptr; }
  const jb_view *views_of(int i) const { return views ? &views[(size_t)i * (size_t)k] : nullptr; }
  // "colour chains" (the _color entry points): colors[i * k + v] goes with views[i * k + v]; null: none
  const jb_color_chain *colors = nullptr;
  const jb_color_chain *colors_of(int i) const { return colors ? &colors[(size_t)i * (size_t)k] : nullptr; }
  // what the builder below refuses of the caller's arguments (reported by the call, in front of everything else)
  JbVerdict bad = {JB_OK, nullptr};

  // ---- the four shapes an entry point passes: PerFile{} (plain) and ----
  static PerFile of_crops(const jb_roi *rois) {
    PerFile per;
    per.rois = rois;
    if (!rois) per.bad = {JB_ERR_NULL, "NULL pointer"};
    return per;
  }
  static PerFile of_views(const jb_view *views, int views_per_image, const jb_color_chain *colors = nullptr) {
    PerFile per;
    per.views = views, per.k = views_per_image, per.colors = colors;
    if (!views) per.bad = {JB_ERR_NULL, "NULL pointer"};
    return per;
  }
  // "view groups": k is the groups' sum (JB_ERR_GEOMETRY: what jb_view_groups_check refuses of the counts)
  static PerFile of_groups(const jb_view *views, const jb_view_group *groups, int n_groups, const jb_color_chain *colors = nullptr) {
    PerFile per;
    if (!views || !groups) per.bad = {JB_ERR_NULL, "NULL pointer"};
    else if (n_groups < 1 || n_groups > JB_VIEW_GROUPS_MAX) per.bad = {JB_ERR_GEOMETRY, "n_groups is outside 1..4"};
    for (int g = 0; g < n_groups && per.bad.status == JB_OK; g++) {
      if (groups[g].n_views < 1 || groups[g].n_views > JB_VIEWS_MAX || groups[g].reserved != 0)
        per.bad = {JB_ERR_GEOMETRY, "a group's n_views is outside 1..16 (or its reserved is not 0)"};
      per.groups[g] = groups[g];
      per.k += groups[g].n_views;
    }
    if (per.bad.status != JB_OK) return per;
    per.views = views, per.n_groups = n_groups, per.colors = colors;
    return per;
  }

  // THE plan choice: the output plan of n files of one frame (the draft frame) under the decoder's request.  A file on
  // its own (parse_one: n = 1) is planned as a batch of one -- v: its k views; one: its rectangle, in the place of the
  // decoder's -- so that plan.image_bytes is the FILE's (its k outputs, its block) and the file stays the unit of every
  // size downstream.  A group (submit_group) brings its members' views (v: n * k, in the group's order) or rectangles
  // (each: n) next to one geometry and one target.  The arrays are read before the submission returns.
  JbOutPlan plan(const OutputRequest &out, const jb_image_desc &frame, int orient, int n, const jb_view *v, const jb_roi *one,
                 const jb_roi *each = nullptr) const {
    if (v && n_groups > 0) return jb_view_groups_plan_(&frame, &out.spec, v, n, groups, n_groups, orient);
    if (v) {
      const jb_resize rs = {out.target.w, out.target.h, out.target.filter, out.target.reserved};
      return jb_views_plan_(&frame, &out.spec, v, n, k, &rs, orient);
    }
    if (each) return jb_out_plan_(&frame, out.scale, &out.spec, nullptr, out.target_ptr(), each, n, orient);
    return jb_out_plan_(&frame, out.scale, &out.spec, one ? one : out.roi_ptr(), out.target_ptr(), nullptr, 0, orient, out.fit_ptr());
  }

  // what a run or a submission of n_paths files checks of the decoder's request in front of its first file (fn: the name
  // the refusal carries); JB_OK, or the refusal through jb_fail_
  int check(const OutputRequest &out, int n_paths, const char *fn) const {
    const std::string name = std::string(fn) + ": ";
    auto fail = [&name](int status, const std::string &why) { return jb_fail_(nullptr, status, (name + why).c_str()); };
    if (rois) {
      // per-image rectangles want a target size and no decoder-wide rectangle (the plan function says so: jb_plan.h)
      static const jb_roi one = {0, 0, 1, 1};
      const jb_image_desc frame = {65535, 65535, 1, 1, {0, 0, 0}, 0};
      const JbOutPlan p = jb_out_plan_(&frame, out.scale, &out.spec, out.roi_ptr(), out.target_ptr(), &one, 1, 1, out.fit_ptr());
      if (p.status != JB_OK) return fail(p.status, p.why);
    }
    if (!views) return JB_OK;
    // "views": no scale, no decoder-wide rectangle (JB_ERR_UNSUPPORTED), a target size (JB_ERR_STATE), k in 1..16
    // ("view groups" bring their own targets; k is the groups' sum)
    if (out.scale != 1) return fail(JB_ERR_UNSUPPORTED, "views cannot be combined with a scale other than 1");
    if (out.has_roi) return fail(JB_ERR_UNSUPPORTED, "views cannot be combined with a rectangle for every image");
    if (!out.has_resize && n_groups == 0) return fail(JB_ERR_STATE, "views want a target size");
    if (k < 1 || k > JB_VIEWS_MAX) return fail(JB_ERR_GEOMETRY, "views_per_image is outside 1..16");
    if (out.fit_ptr()) return fail(JB_ERR_UNSUPPORTED, "a fit other than JB_FIT_STRETCH is set: views cannot be combined with it");
    // "colour chains": a bad chain refuses the whole call, behind the call's own refusals
    if (!colors) return JB_OK;
    if ((int64_t)n_paths * k > 0x7fffffffLL) return fail(JB_ERR_CAPACITY, "too many chains");
    const int rc = jb_color_check(colors, n_paths * k, nullptr);
    if (rc != JB_OK) return fail(rc, std::string(jb_last_error(nullptr)));
    // the refusals of the geometric operations that depend on the views' size: view v of a file has its group's target, or the decoder's
    for (int i = 0; i < n_paths; i++) {
      int v0 = 0;
      for (int g = 0; g < (n_groups > 0 ? n_groups : 1); g++) {
        const int n = n_groups > 0 ? groups[g].n_views : k;
        const int32_t w = n_groups > 0 ? groups[g].rs.out_w : out.target.w, h = n_groups > 0 ? groups[g].rs.out_h : out.target.h;
        int64_t bad = 0;
        const char *why = nullptr;
        // (a target outside 1..65535 is every file's own refusal, by its plan)
        const bool sized = w >= 1 && h >= 1 && w <= 65535 && h <= 65535;
        const int rs = sized ? jb_color_check_size_(colors + (size_t)i * (size_t)k + v0, n, w, h, &bad, &why) : JB_OK;
        if (rs != JB_OK) return fail(rs, "colour chain " + std::to_string((int64_t)i * k + v0 + bad) + ": " + why);
        v0 += n;
      }
    }
    return JB_OK;
  }
};

// The owning companion of PerFile: the per-file arrays of some files of a run, copied -- a part's share of a multi-device
// run (file i goes where path i goes), a submitted batch (the caller's arrays need not outlive submit) -- with the
// by-value part (k, the groups) next to them.
struct PerFileOwned {
  PerFile asked;  // (its pointers only say which arrays there are)
  std::vector<jb_roi> rois;
  std::vector<jb_view> views;
  std::vector<jb_color_chain> colors;
  // files first, first + step, ... (< n_files) of `from`; (0, 1): all of them
  void copy(const PerFile &from, int n_files, int first = 0, int step = 1) {
    asked = from;
    rois.clear(), views.clear(), colors.clear();
    const size_t k = (size_t)from.k;
    for (int i = first; i < n_files; i += step) {
      if (from.rois) rois.push_back(from.rois[i]);
      if (from.views) views.insert(views.end(), from.views_of(i), from.views_of(i) + k);
      if (from.colors) colors.insert(colors.end(), from.colors_of(i), from.colors_of(i) + k);
    }
  }
  // the copied files as a PerFile that points into this object
  PerFile get() const {
    PerFile per = asked;
    per.rois = asked.rois ? rois.data() : nullptr, per.views = asked.views ? views.data() : nullptr;
    per.colors = asked.colors ? colors.data() : nullptr;
    return per;
  }
};
