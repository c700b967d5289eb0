// jb_color_host.cpp -- "colour chains" (include/jpegblk.h), the host half: the ONE place that checks chains
// (jb_color_check) and the CPU statement of the kernels' arithmetic (jb_color_host), through the jb_color_core.h the
// kernels compile.  Host-only, like jb_geometry.cpp.
#include <cmath>
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
  int contrasts = 0, blurs = 0;
  bool box_too_large = false, contrast_behind_blur = false;
  for (int i = 0; i < c.n_ops; i++) {
    const float v = c.ops[i].value;
    switch (c.ops[i].op) {
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
      case JB_COLOR_BLUR: {
        JbBlurWeights k;
        bool geometry;
        if (!jbc_blur_weights(v, &k, &geometry)) {
          if (geometry) return "a blur radius is not finite or below 0";
          box_too_large = true;
        }
        blurs++;
        break;
      }
      default: return "unknown op";
    }
  }
  *status = JB_ERR_UNSUPPORTED;
  if (contrasts > 1) return "more than one JB_COLOR_CONTRAST in a chain (each costs a reduction pass)";
  if (box_too_large) return "a blur radius whose box radius is above JB_COLOR_BLUR_BOX_MAX (7: Gaussian radii up to about 8.4)";
  if (blurs > 1) return "more than one JB_COLOR_BLUR in a chain (each costs a tile pass)";
  if (contrast_behind_blur) return "a JB_COLOR_CONTRAST behind a JB_COLOR_BLUR (its mean would be the blurred view's)";
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
  // the kernels' two passes: the ops in front of the contrast and the luma sum, then the whole chain with the mean
  const int at = jbc_contrast_at(*chain);
  int mean = 0;
  if (at >= 0) {
    uint64_t sum = 0;
    for (int y = 0; y < h; y++) {
      const uint8_t *p = in + y * in_row_stride;
      for (int x = 0; x < w; x++, p += 3) {
        int r = p[0], g = p[1], b = p[2];
        jbc_apply_ops(*chain, 0, at, 0, &r, &g, &b);
        sum += (uint64_t)jbc_luma(r, g, b);
      }
    }
    mean = jbc_contrast_mean(sum, (uint64_t)w * (uint64_t)h);
  }
  const int blur = jbc_blur_at(*chain);
  if (blur < 0) {
    for (int y = 0; y < h; y++) {
      const uint8_t *p = in + y * in_row_stride;
      uint8_t *q = out + y * out_row_stride;
      for (int x = 0; x < w; x++, p += 3, q += 3) {
        int r = p[0], g = p[1], b = p[2];
        jbc_apply_ops(*chain, 0, chain->n_ops, mean, &r, &g, &b);
        q[0] = (uint8_t)r, q[1] = (uint8_t)g, q[2] = (uint8_t)b;
      }
    }
    return JB_OK;
  }
  // the blur kernel's order: the ops in front of the blur, six passes between two buffers of its own (in == out is
  // allowed), the ops behind it
  JbBlurWeights k;
  bool geometry;
  if (!jbc_blur_weights(chain->ops[blur].value, &k, &geometry)) return jb_fail_(nullptr, JB_ERR_UNSUPPORTED, "jb_color_host: blur radius");
  const int64_t row = 3LL * w;
  std::vector<uint8_t> a, b2;
  try {
    a.resize((size_t)(row * h)), b2.resize((size_t)(row * h));
  } catch (const std::bad_alloc &) {
    return jb_fail_(nullptr, JB_ERR_CAPACITY, "jb_color_host: no memory for the blur's two buffers");
  }
  for (int y = 0; y < h; y++) {
    const uint8_t *p = in + y * in_row_stride;
    uint8_t *q = a.data() + y * row;
    for (int x = 0; x < w; x++, p += 3, q += 3) {
      int r = p[0], g = p[1], b = p[2];
      jbc_apply_ops(*chain, 0, blur, mean, &r, &g, &b);
      q[0] = (uint8_t)r, q[1] = (uint8_t)g, q[2] = (uint8_t)b;
    }
  }
  uint8_t *src = a.data(), *dst = b2.data();
  for (int pass = 0; pass < 6; pass++) {
    if (pass < 3) {
      for (int y = 0; y < h; y++)
        for (int c = 0; c < 3; c++) jbc_blur_line(src + y * row + c, dst + y * row + c, (int64_t)3, 0, w, 0, w - 1, k);
    } else {
      for (int64_t xc = 0; xc < row; xc++) jbc_blur_line(src + xc, dst + xc, row, 0, h, 0, h - 1, k);
    }
    std::swap(src, dst);
  }
  for (int y = 0; y < h; y++) {
    const uint8_t *p = src + y * row;
    uint8_t *q = out + y * out_row_stride;
    for (int x = 0; x < w; x++, p += 3, q += 3) {
      int r = p[0], g = p[1], b = p[2];
      jbc_apply_ops(*chain, blur + 1, chain->n_ops, 0, &r, &g, &b);
      q[0] = (uint8_t)r, q[1] = (uint8_t)g, q[2] = (uint8_t)b;
    }
  }
  return JB_OK;
}
