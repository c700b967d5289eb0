// batch_request_check -- the rules of the batch decoder's request (jpeg_decoder_amd/csrc/jb_batch_request.h) walked
// without a decoder: every request of tests/batch_refusal_cases.py that can be had, every setter's edit of it through
// OutputRequest::verdict, and every entry point's arguments through PerFile's builders and PerFile::check, printed as
//   <case name> TAB <code> TAB <text>
// under the names of that table, for tests/test_batch_request_cpu.py to compare with tests/golden/batch_refusals.json.
// The edits and the setters' own words are restated here; the rules are the header's.  A stand-alone program, built
// with ASan + UBSan (tools/fuzz/Makefile).
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../jpeg_decoder_amd/csrc/jb_batch_request.h"

// ---- the error channel of the library, which needs a context there ----
static std::string g_err;
int jb_fail_(jb_ctx *, int code, const char *msg) {
  g_err = msg ? msg : "";
  return code;
}
extern "C" const char *jb_last_error(const jb_ctx *) { return g_err.c_str(); }

static int g_rows = 0;
static void row(const std::string &name, int code, const std::string &text) {
  printf("%s\t%d\t%s\n", name.c_str(), code, code == JB_OK ? "" : text.c_str());
  g_rows++;
}

static const jb_roi kRect = {2, 2, 8, 8};
static const int kPlanar = JB_FMT_RGB_F32_CHW;

struct State {
  int scale, arith, orient, draft, fmt, roi, target, fit;
  std::string name() const {
    char b[64];
    snprintf(b, sizeof b, "s%da%do%dd%df%dr%dt%dc%d", scale, arith, orient, draft, fmt, roi, target, fit);
    return b;
  }
  OutputRequest request() const {
    OutputRequest q;
    q.scale = scale, q.arith = arith, q.orient = orient, q.draft = draft;
    q.spec.format = fmt;
    for (int c = 0; c < 3 && fmt; c++) q.spec.scale[c] = 1.0f;
    q.has_roi = roi != 0;
    if (roi) q.roi = kRect;
    q.has_resize = target != 0;
    if (target) q.target = JbTarget{8, 8, 0, 0};
    q.fit.mode = fit;
    return q;
  }
};

// one setter with one argument that passes the setter's own check: the edit, and the setter's own words
struct Setter {
  const char *name, *arg;
  void (*edit)(OutputRequest &);
  const char *combined, *other;
};
static const Setter kSetters[] = {
    {"scale", "1", [](OutputRequest &q) { q.scale = 1; }, "a planar output format, a rectangle or a target size is set: it cannot be combined with a scale", nullptr},
    {"scale", "2", [](OutputRequest &q) { q.scale = 2; }, "a planar output format, a rectangle or a target size is set: it cannot be combined with a scale", nullptr},
    {"output_format", "fmt0", [](OutputRequest &q) { q.spec = jb_output_spec{}; }, "the decoder's scale is not 1: a planar output format cannot be combined with it", nullptr},
    {"output_format", "planar", [](OutputRequest &q) { q.spec = State{1, 0, 1, 1, kPlanar, 0, 0, 0}.request().spec; },
     "the decoder's scale is not 1: a planar output format cannot be combined with it", nullptr},
    {"roi", "null", [](OutputRequest &q) { q.has_roi = false, q.roi = jb_roi{}; }, "the decoder's scale is not 1: a rectangle cannot be combined with it", "no frame can hold this rectangle"},
    {"roi", "rect", [](OutputRequest &q) { q.has_roi = true, q.roi = kRect; }, "the decoder's scale is not 1: a rectangle cannot be combined with it", "no frame can hold this rectangle"},
    {"roi", "bad", [](OutputRequest &q) { q.has_roi = true, q.roi = jb_roi{0, 0, 0, 8}; }, "the decoder's scale is not 1: a rectangle cannot be combined with it", "no frame can hold this rectangle"},
    {"resize", "0x0", [](OutputRequest &q) { q.has_resize = false, q.target = JbTarget{0, 0, q.target.filter, 0}; },
     "the decoder's scale is not 1: a target size cannot be combined with it", "the target size is outside 1..65535"},
    {"resize", "8x8", [](OutputRequest &q) { q.has_resize = true, q.target = JbTarget{8, 8, q.target.filter, 0}; },
     "the decoder's scale is not 1: a target size cannot be combined with it", "the target size is outside 1..65535"},
    {"resize", "70000x8", [](OutputRequest &q) { q.has_resize = true, q.target = JbTarget{70000, 8, q.target.filter, 0}; },
     "the decoder's scale is not 1: a target size cannot be combined with it", "the target size is outside 1..65535"},
    {"filter", "1", [](OutputRequest &q) { q.target.filter = 1; }, nullptr, nullptr},
    {"fit", "null", [](OutputRequest &q) { q.fit = jb_fit{}; }, nullptr, nullptr},
    {"fit", "cover", [](OutputRequest &q) { q.fit = jb_fit{}, q.fit.mode = JB_FIT_COVER; }, nullptr, nullptr},
    {"arithmetic", "0", [](OutputRequest &q) { q.arith = 0; }, nullptr, nullptr},
    {"arithmetic", "1", [](OutputRequest &q) { q.arith = 1; }, nullptr, nullptr},
    {"orientation", "1", [](OutputRequest &q) { q.orient = 1; }, nullptr, nullptr},
    {"orientation", "6", [](OutputRequest &q) { q.orient = 6; }, nullptr, nullptr},
    {"orientation", "0", [](OutputRequest &q) { q.orient = 0; }, nullptr, nullptr},
    {"draft", "1", [](OutputRequest &q) { q.draft = 1; }, nullptr, nullptr},
    {"draft", "2", [](OutputRequest &q) { q.draft = 2; }, nullptr, nullptr},
};

static void setters() {
  static const int two[2] = {1, 2}, bit[2] = {0, 1}, orients[3] = {1, 0, 6}, fmts[2] = {0, kPlanar}, fits[2] = {0, JB_FIT_COVER};
  for (int scale : two) for (int arith : bit) for (int orient : orients) for (int draft : two) for (int fmt : fmts)
    for (int roi : bit) for (int target : bit) for (int fit : fits) {
      const State s = {scale, arith, orient, draft, fmt, roi, target, fit};
      if (scale != 1 && (arith == 1 || orient != 1 || draft != 1 || fmt || roi || target)) continue;
      if (draft != 1 && (arith != 1 || orient != 1)) continue;
      if (s.request().verdict().status != JB_OK) {  // (the table's requests are those that can be had)
        fprintf(stderr, "%s: %s\n", s.name().c_str(), s.request().verdict().why);
        exit(1);
      }
      for (const Setter &t : kSetters) {
        OutputRequest q = s.request();
        t.edit(q);
        const JbVerdict v = q.verdict(t.combined, t.other);
        row("set:" + s.name() + ":idle:" + t.name + "(" + t.arg + ")", v.status,
            v.status == JB_OK ? "" : std::string("jb_batch_decoder_set_") + t.name + ": " + v.why);
      }
    }
}

// an entry point with the arguments of the table's variant, on a decoder holding `out` with nothing in flight
static void call(const char *state, const OutputRequest &out, bool submit, const std::string &entry, const std::string &variant) {
  static jb_view views[34];
  jb_view_group groups[5];
  jb_color_chain colors[34] = {};
  for (jb_view &v : views) v = jb_view{0, 0, 8, 8, 0, 0};
  for (jb_view_group &g : groups) g = jb_view_group{jb_resize{8, 8, 0, 0}, 1, 0};
  if (variant == "n_views0") groups[0].n_views = 0;
  if (variant == "reserved1") groups[1].reserved = 1;
  if (variant == "bad_chain") colors[1].n_ops = 1, colors[1].ops[0].op = 99;
  const int k = variant == "k0" ? 0 : variant == "k17" ? 17 : 2;
  const int n_groups = variant == "n_groups0" ? 0 : variant == "n_groups5" ? 5 : 2;
  const int n_paths = variant == "bad_chain" ? 1 : 0;
  static const jb_roi one = {0, 0, 8, 8};
  const jb_view *const v = variant == "null_views" ? nullptr : views;
  const jb_color_chain *const c = entry.find("_color") == std::string::npos || variant == "null_colors" ? nullptr : colors;
  PerFile per;
  if (entry == "_crops") per = PerFile::of_crops(variant == "null_rois" ? nullptr : &one);
  else if (entry.find("_view_groups") == 0) per = PerFile::of_groups(v, variant == "null_groups" ? nullptr : groups, n_groups, c);
  else if (entry.find("_views") == 0) per = PerFile::of_views(v, k, c);
  const std::string kind = submit ? "submit" : "run";
  const std::string fn = "jb_batch_decoder_" + kind + entry;
  const std::string name = std::string("call:") + state + ":" + kind + entry + ":" + variant;
  if (per.bad.status != JB_OK) return row(name, per.bad.status, fn + ": " + per.bad.why);
  // (a submission's refusals of the per-file arrays carry the name of the entry point without its _color)
  const std::string checked = !submit ? fn : per.rois ? "jb_batch_decoder_submit_crops" : per.n_groups > 0 ? "jb_batch_decoder_submit_view_groups" : "jb_batch_decoder_submit_views";
  const int rc = per.check(out, n_paths, checked.c_str());
  row(name, rc, g_err);
}

static void calls() {
  const struct {
    const char *name;
    State s;
  } states[] = {{"plain", {1, 0, 1, 1, 0, 0, 0, 0}}, {"target", {1, 0, 1, 1, 0, 0, 1, 0}}, {"scale2", {2, 0, 1, 1, 0, 0, 0, 0}},
                {"rect", {1, 0, 1, 1, 0, 1, 0, 0}}, {"fit", {1, 0, 1, 1, 0, 0, 1, JB_FIT_COVER}}};
  const char *entries[] = {"", "_crops", "_views", "_views_color", "_view_groups", "_view_groups_color"};
  for (const auto &st : states)
    for (int submit = 0; submit < 2; submit++)
      for (const std::string entry : entries) {
        std::vector<std::string> variants = {"ok"};
        if (entry == "_crops") variants.push_back("null_rois");
        if (entry.find("_views") == 0) variants.insert(variants.end(), {"null_views", "k0", "k17"});
        if (entry.find("_view_groups") == 0) variants.insert(variants.end(), {"null_views", "null_groups", "n_groups0", "n_groups5", "n_views0", "reserved1"});
        if (entry.find("_color") != std::string::npos) variants.insert(variants.end(), {"null_colors", "bad_chain"});
        for (const std::string &variant : variants) call(st.name, st.s.request(), submit != 0, entry, variant);
      }
}

int main() {
  setters();
  calls();
  fprintf(stderr, "%d rows\n", g_rows);
  return 0;
}
