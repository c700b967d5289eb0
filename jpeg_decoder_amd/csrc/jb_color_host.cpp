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
  int contrasts = 0, blurs = 0, stats = 0, nbhds = 0;
  bool box_too_large = false, contrast_behind_blur = false, stat_behind_nbhd = false;
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
  *status = JB_OK;
  return nullptr;
}

}  // namespace

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

extern "C" int jb_color_host(const uint8_t *in, int64_t in_row_stride, int32_t w, int32_t h, const jb_color_chain *chain, uint8_t *out,
                             int64_t out_row_stride) {
  if (!in || !chain || !out) return jb_fail_(nullptr, JB_ERR_NULL, "jb_color_host: NULL pointer");
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_host: size outside 1..65535");
  if (in_row_stride < 3LL * w || out_row_stride < 3LL * w) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_host: row stride < 3*width");
  const int rc = jb_color_check(chain, 1, nullptr);
  if (rc != JB_OK) return rc;
  // The kernels' order on one tight copy of the view: the ops in front of a statistics operation, then its statistic of the view
  // as it stands (the luma sum, or the three histograms and their tables); the ops in front of the neighbourhood operation,
  // then its filter between two buffers (in == out is allowed); then the rest.
  const JbcShape shape = jbc_shape(*chain);
  const int64_t row = 3LL * w;
  std::vector<uint8_t> a, b2;
  try {
    a.resize((size_t)(row * h));
    if (shape.nbhd >= 0) b2.resize((size_t)(row * h));
  } catch (const std::bad_alloc &) {
    return jb_fail_(nullptr, JB_ERR_CAPACITY, "jb_color_host: no memory for the view's working copies");
  }
  for (int y = 0; y < h; y++) memcpy(a.data() + y * row, in + y * in_row_stride, (size_t)row);
  uint8_t lut[JB_COLOR_STATS_MAX][768];
  JbcCtx s;
  s.mean = 0, s.at1 = shape.stat1, s.lut[0] = lut[0], s.lut[1] = lut[1];
  int done = 0;  // ops [0, done) are applied to `a`
  const auto run = [&](int last) {
    if (last > done)
      for (uint8_t *p = a.data(), *end = p + row * h; p < end; p += 3) {
        int r = p[0], g = p[1], b = p[2];
        jbc_apply_ops<true>(*chain, done, last, s, &r, &g, &b);
        p[0] = (uint8_t)r, p[1] = (uint8_t)g, p[2] = (uint8_t)b;
      }
    done = last;
  };
  for (int k = 0; k < shape.n_stats; k++) {
    const int at = jbc_stat_at(shape, k);
    run(at);
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
    run(shape.nbhd);
    done = shape.nbhd + 1;
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
  }
  run(chain->n_ops);
  for (int y = 0; y < h; y++) memcpy(out + y * out_row_stride, a.data() + y * row, (size_t)row);
  return JB_OK;
}

extern "C" int jb_color_lut(int op, const uint32_t *counts, uint8_t *lut) {
  if (!counts || !lut) return jb_fail_(nullptr, JB_ERR_NULL, "jb_color_lut: NULL pointer");
  if (!jbc_is_hist(op)) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_color_lut: op is neither JB_COLOR_AUTOCONTRAST nor JB_COLOR_EQUALIZE");
  jbc_lut_from_counts(op, counts, lut);
  return JB_OK;
}
