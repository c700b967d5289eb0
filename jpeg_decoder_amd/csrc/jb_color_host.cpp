// jb_color_host.cpp -- "colour chains" (include/jpegblk.h), the host half: the ONE place that checks chains
// (jb_color_check) and the CPU statement of the kernels' arithmetic (jb_color_host), through the jb_color_core.h the
// kernels compile.  Host-only, like jb_geometry.cpp.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jb_color_core.h"
#include "jb_internal.h"

namespace {

// why a chain cannot be had (null: it can); *status: JB_ERR_GEOMETRY or JB_ERR_UNSUPPORTED
const char *chain_refusal(const jb_color_chain &c, int *status) {
  *status = JB_ERR_GEOMETRY;
  if (c.n_ops < 0 || c.n_ops > JB_COLOR_OPS_MAX) return "n_ops is outside 0..8";
  if (c.reserved != 0) return "reserved is not 0";
  int contrasts = 0, blurs = 0, stats = 0, nbhds = 0, warps = 0;
  bool box_too_large = false, contrast_behind_blur = false, stat_behind_nbhd = false, warp_behind_nbhd = false;
  for (int i = 0; i < c.n_ops; i++) {
    const float v = c.ops[i].value;
    const int op = c.ops[i].op;
    if (jbc_is_stat(op)) {
      stats++;
      if (nbhds) stat_behind_nbhd = true;
    }
    switch (op) {
      case JB_COLOR_CONTRAST:
        contrasts++;
        if (blurs) contrast_behind_blur = true;
        [[fallthrough]];
      case JB_COLOR_BRIGHTNESS:
      case JB_COLOR_SATURATION:
        if (!std::isfinite(v) || v < 0.0f) return "a factor is not finite or below 0";
        break;
      case JB_COLOR_HUE:
        if (!(v >= 0.0f && v <= 255.0f) || v != std::floor(v)) return "a hue shift is outside 0..255 or not integral";
        break;
      case JB_COLOR_SOLARIZE:
        if (!(v >= 0.0f && v <= 256.0f) || v != std::floor(v)) return "a solarize threshold is outside 0..256 or not integral";
        break;
      case JB_COLOR_GRAYSCALE:
        if (v != 0.0f) return "the value of JB_COLOR_GRAYSCALE is not 0";
        break;
      case JB_COLOR_POSTERIZE:
        if (!(v >= 0.0f && v <= 8.0f) || v != std::floor(v)) return "posterize bits are outside 0..8 or not integral";
        break;
      case JB_COLOR_INVERT:
      case JB_COLOR_AUTOCONTRAST:
      case JB_COLOR_EQUALIZE:
        if (v != 0.0f) return "the value of JB_COLOR_INVERT / _AUTOCONTRAST / _EQUALIZE is not 0";
        break;
      case JB_COLOR_SHARPNESS:
        if (!std::isfinite(v) || v < 0.0f) return "a sharpness factor is not finite or below 0";
        nbhds++;
        break;
      case JB_COLOR_BLUR: {
        JbBlurWeights k;
        bool geometry;
        if (!jbc_blur_weights(v, &k, &geometry)) {
          if (geometry) return "a blur radius is not finite or below 0";
          box_too_large = true;
        }
        blurs++, nbhds++;
        break;
      }
      case JB_COLOR_SHEAR_X:
      case JB_COLOR_SHEAR_Y:
      case JB_COLOR_ROTATE:
        if (!std::isfinite(v)) return "the value of a geometric operation is not finite";
        warps++;
        if (nbhds) warp_behind_nbhd = true;
        break;
      case JB_COLOR_TRANSLATE_X:
      case JB_COLOR_TRANSLATE_Y:
        if (!std::isfinite(v) || v != std::floor(v) || v < -65535.0f || v > 65535.0f)
          return "a translation is not finite, not integral or its absolute value is above 65535";
        warps++;
        if (nbhds) warp_behind_nbhd = true;
        break;
      default: return "unknown op";
    }
  }
  *status = JB_ERR_UNSUPPORTED;
  if (contrasts > 1) return "more than one JB_COLOR_CONTRAST in a chain (each costs a reduction pass)";
  if (stats > JB_COLOR_STATS_MAX) return "more than JB_COLOR_STATS_MAX (2) statistics operations in a chain (each costs a reduction pass)";
  if (box_too_large) return "a blur radius whose box radius is above JB_COLOR_BLUR_BOX_MAX (7: Gaussian radii up to about 8.4)";
  if (blurs > 1) return "more than one JB_COLOR_BLUR in a chain (each costs a tile pass)";
  if (nbhds > 1) return "more than one neighbourhood operation (blur, sharpness) in a chain (each costs a tile pass)";
  if (contrast_behind_blur) return "a JB_COLOR_CONTRAST behind a JB_COLOR_BLUR (its mean would be the blurred view's)";
  if (stat_behind_nbhd) return "a statistics operation behind a neighbourhood operation (it would want the filtered view's statistics)";
  if (warps > JB_COLOR_WARPS_MAX) return "more than JB_COLOR_WARPS_MAX (2) geometric operations in a chain";
  if (warp_behind_nbhd) return "a geometric operation behind a neighbourhood operation (it would want the filter at a gathered position)";
  *status = JB_OK;
  return nullptr;
}

}  // namespace

// what jb_color_check cannot know: the geometric operations of CHECKED chains on views of w x h (jb_warp_params' refusals that
// depend on the size).  JB_OK, or the status with *bad (may be null) the first such chain's index and *why the reason.
int jb_color_check_size_(const jb_color_chain *chains, int64_t n, int32_t w, int32_t h, int64_t *bad, const char **why) {
  for (int64_t i = 0; i < n; i++)
    for (int k = 0; k < chains[i].n_ops && k < JB_COLOR_OPS_MAX; k++) {
      if (!jbc_is_warp(chains[i].ops[k].op)) continue;
      JbWarp unused;
      const int rc = jbc_warp_params(chains[i].ops[k].op, chains[i].ops[k].value, w, h, &unused, why);
      if (rc != JB_OK) {
        if (bad) *bad = i;
        return rc;
      }
    }
  return JB_OK;
}

extern "C" int jb_color_check(const jb_color_chain *chains, int n, int *bad_index) {
  if (bad_index) *bad_index = -1;
  if (n < 0) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_check: negative count");
  if (!chains && n > 0) return jb_fail_(nullptr, JB_ERR_NULL, "jb_color_check: chains is NULL");
  for (int i = 0; i < n; i++) {
    int status;
    if (const char *why = chain_refusal(chains[i], &status)) {
      if (bad_index) *bad_index = i;
      return jb_fail_(nullptr, status, ("colour chain " + std::to_string(i) + ": " + why).c_str());
    }
  }
  return JB_OK;
}

extern "C" int jb_blur_params(float radius, int32_t *r, uint32_t *ww, uint32_t *fw) {
  if (!r || !ww || !fw) return jb_fail_(nullptr, JB_ERR_NULL, "jb_blur_params: NULL pointer");
  JbBlurWeights k;
  bool geometry;
  if (!jbc_blur_weights(radius, &k, &geometry))
    return geometry ? jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_blur_params: the radius is not finite or below 0")
                    : jb_fail_(nullptr, JB_ERR_UNSUPPORTED, "jb_blur_params: the box radius is above JB_COLOR_BLUR_BOX_MAX (7)");
  *r = k.r, *ww = k.ww, *fw = k.fw;
  return JB_OK;
}

extern "C" int jb_warp_params(int op, float value, int32_t w, int32_t h, int32_t *mode, int32_t coef[6]) {
  if (!mode || !coef) return jb_fail_(nullptr, JB_ERR_NULL, "jb_warp_params: NULL pointer");
  JbWarp k;
  const char *why;
  const int rc = jbc_warp_params(op, value, w, h, &k, &why);
  if (rc != JB_OK) return jb_fail_(nullptr, rc, (std::string("jb_warp_params: ") + why).c_str());
  *mode = k.mode;
  for (int i = 0; i < 6; i++) coef[i] = k.coef[i];
  return JB_OK;
}

extern "C" int jb_color_host(const uint8_t *in, int64_t in_row_stride, int32_t w, int32_t h, const jb_color_chain *chain, uint8_t *out,
                             int64_t out_row_stride) {
  if (!in || !chain || !out) return jb_fail_(nullptr, JB_ERR_NULL, "jb_color_host: NULL pointer");
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_host: size outside 1..65535");
  if (in_row_stride < 3LL * w || out_row_stride < 3LL * w) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_host: row stride < 3*width");
  const int rc = jb_color_check(chain, 1, nullptr);
  if (rc != JB_OK) return rc;
  {
    const char *why;
    const int rs = jb_color_check_size_(chain, 1, w, h, nullptr, &why);
    if (rs != JB_OK) return jb_fail_(nullptr, rs, (std::string("jb_color_host: colour chain 0: ") + why).c_str());
  }
  // The kernels' order on one tight copy of the view: the view as it stands in front of a statistics operation, then its
  // statistic (the luma sum, or the three histograms and their tables); the view in front of the neighbourhood operation, then
  // its filter between two buffers (in == out is allowed); then the rest, pointwise (no geometric operation stands behind a
  // neighbourhood operation).  A chain WITHOUT a geometric operation goes forwards on the copy, ops [done, last) at a time, as
  // it did before there were any; one with a geometric operation computes every such view pixel by pixel through jbc_gather
  // (the text the kernels compile) from a second copy, the input's.
  const JbcShape shape = jbc_shape(*chain);
  const JbcWarpShape ws = jbc_warp_shape(*chain);
  JbWarp wk[JB_COLOR_WARPS_MAX] = {};
  for (int k = 0; k < JB_COLOR_WARPS_MAX; k++) {
    const int at = k == 0 ? ws.warp0 : ws.warp1;
    const char *why;
    if (at >= 0 && jbc_warp_params(chain->ops[at].op, chain->ops[at].value, w, h, &wk[k], &why) != JB_OK)
      return jb_fail_(nullptr, JB_ERR_UNSUPPORTED, "jb_color_host: geometric operation");  // (checked above: not reached)
  }
  const int64_t row = 3LL * w;
  std::vector<uint8_t> orig, a, b2;
  const bool warped = ws.warp0 >= 0;
  try {
    if (warped) orig.resize((size_t)(row * h));
    a.resize((size_t)(row * h));
    if (shape.nbhd >= 0) b2.resize((size_t)(row * h));
  } catch (const std::bad_alloc &) {
    return jb_fail_(nullptr, JB_ERR_CAPACITY, "jb_color_host: no memory for the view's working copies");
  }
  for (int y = 0; y < h; y++) memcpy((warped ? orig : a).data() + y * row, in + y * in_row_stride, (size_t)row);
  uint8_t lut[JB_COLOR_STATS_MAX][768];
  JbcCtx s;
  s.mean = 0, s.at1 = shape.stat1, s.lut[0] = lut[0], s.lut[1] = lut[1];
  // ops [first, last) on `a`, pointwise
  const auto run = [&](int first, int last) {
    if (last > first)
      for (uint8_t *p = a.data(), *end = p + row * h; p < end; p += 3) {
        int r = p[0], g = p[1], b = p[2];
        jbc_apply_ops<true>(*chain, first, last, s, &r, &g, &b);
        p[0] = (uint8_t)r, p[1] = (uint8_t)g, p[2] = (uint8_t)b;
      }
  };
  int done = 0;  // without a geometric operation: ops [0, done) are applied to `a`
  // `a` = the view as it stands in front of op `last`
  const auto view_before = [&](int last) {
    if (!warped) {
      run(done, last);
      done = last;
      return;
    }
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        int r, g, b;
        jbc_gather<true>(*chain, ws, last, s, wk, orig.data(), row, w, h, x, y, &r, &g, &b);
        uint8_t *const p = a.data() + y * row + 3 * x;
        p[0] = (uint8_t)r, p[1] = (uint8_t)g, p[2] = (uint8_t)b;
      }
  };
  for (int k = 0; k < shape.n_stats; k++) {
    const int at = jbc_stat_at(shape, k);
    view_before(at);
    if (chain->ops[at].op == JB_COLOR_CONTRAST) {
      uint64_t sum = 0;
      for (const uint8_t *p = a.data(), *end = p + row * h; p < end; p += 3) sum += (uint64_t)jbc_luma(p[0], p[1], p[2]);
      s.mean = jbc_contrast_mean(sum, (uint64_t)w * (uint64_t)h);
    } else {
      std::vector<uint32_t> counts(768, 0);
      for (const uint8_t *p = a.data(), *end = p + row * h; p < end; p += 3) counts[p[0]]++, counts[256 + p[1]]++, counts[512 + p[2]]++;
      for (int c = 0; c < 3; c++) jbc_lut_from_counts(chain->ops[at].op, counts.data() + 256 * c, lut[k] + 256 * c);
    }
  }
  if (shape.nbhd >= 0) {
    view_before(shape.nbhd);
    uint8_t *src = a.data(), *dst = b2.data();
    if (chain->ops[shape.nbhd].op == JB_COLOR_BLUR) {
      JbBlurWeights k;
      bool geometry;
      if (!jbc_blur_weights(chain->ops[shape.nbhd].value, &k, &geometry)) return jb_fail_(nullptr, JB_ERR_UNSUPPORTED, "jb_color_host: blur radius");
      for (int pass = 0; pass < 6; pass++) {
        if (pass < 3) {
          for (int y = 0; y < h; y++)
            for (int c = 0; c < 3; c++) jbc_blur_line(src + y * row + c, dst + y * row + c, (int64_t)3, 0, w, 0, w - 1, k);
        } else {
          for (int64_t xc = 0; xc < row; xc++) jbc_blur_line(src + xc, dst + xc, row, 0, h, 0, h - 1, k);
        }
        std::swap(src, dst);
      }
    } else {
      // ImageEnhance.Sharpness: the blend against SMOOTH; the outermost rows and columns are SMOOTH's copies of the input
      const float f = chain->ops[shape.nbhd].value;
      for (int y = 0; y < h; y++)
        for (int64_t xc = 0; xc < row; xc++) {
          const uint8_t *const p = src + y * row + xc;
          int sm = p[0];
          if (y > 0 && y < h - 1 && xc >= 3 && xc < row - 3)
            sm = jbc_smooth(p[row - 3], p[row], p[row + 3], p[-3], p[0], p[3], p[-row - 3], p[-row], p[-row + 3]);
          dst[y * row + xc] = (uint8_t)jbc_blend(sm, p[0], f);
        }
      std::swap(src, dst);
    }
    if (src != a.data()) a.swap(b2);
    run(shape.nbhd + 1, chain->n_ops);
  } else {
    view_before(chain->n_ops);
  }
  for (int y = 0; y < h; y++) memcpy(out + y * out_row_stride, a.data() + y * row, (size_t)row);
  return JB_OK;
}

extern "C" int jb_color_lut(int op, const uint32_t *counts, uint8_t *lut) {
  if (!counts || !lut) return jb_fail_(nullptr, JB_ERR_NULL, "jb_color_lut: NULL pointer");
  if (!jbc_is_hist(op)) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_lut: op is neither JB_COLOR_AUTOCONTRAST nor JB_COLOR_EQUALIZE");
  jbc_lut_from_counts(op, counts, lut);
  return JB_OK;
}
