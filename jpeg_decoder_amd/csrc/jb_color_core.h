// jb_color_core.h -- "colour chains" (include/jpegblk.h): the per-pixel arithmetic of every colour operation, in one
// place: jb_color.hip compiles it for gfx950, jb_color_host (jb_color.hip's host half) and the CPU tests the same text for
// the host.  It is Pillow's, operation for operation -- ImageEnhance.Brightness / Contrast / Color are Image.blend against
// a degenerate image, the hue shift is convert("HSV") and back, grayscale is convert("L"), solarize is ImageOps.solarize.
// JB_COLOR_BLUR is ImageFilter.GaussianBlur: BoxBlur.c's weights and its one pass along a line, at the end of this file.
// Posterize / invert / autocontrast / equalize are ImageOps', JB_COLOR_SHARPNESS is ImageEnhance.Sharpness: a blend against
// ImageFilter.SMOOTH.
//
// Every float step is written as ONE operation per statement and the file is built with -ffp-contract=off and without
// fast-math: a product and the sum behind it stay two roundings, and f32 / f64 divisions are correctly rounded.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/jpegblk.h"

#if defined(__HIPCC__)
#define JBC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define JBC_FN inline
#endif

// convert("L"): ITU-R 601-2 luma in 16-bit fixed point, rounded
JBC_FN int jbc_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// Image.blend(degenerate, image, a) of one sample: d, v in 0..255.  float32, product and sum rounded separately.
JBC_FN int jbc_blend(int d, int v, float a) {
  const float prod = a * (float)(v - d);
  const float t = (float)d + prod;
  if (a >= 0.0f && a <= 1.0f) return (int)t;  // (t lies between d and v: truncation alone)
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (int)t;
}

JBC_FN int jbc_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ImageEnhance.Contrast's int(mean + 0.5) of the view's luma sum S over N pixels, in integers
JBC_FN int jbc_contrast_mean(uint64_t sum, uint64_t n) { return (int)((2 * sum + n) / (2 * n)); }

// convert("HSV") of one pixel.  s, rc, gc, bc are float32; the hue's sum is taken in double FROM the float values and
// lands in a float variable; so does the fmod.
JBC_FN void jbc_rgb_to_hsv(int r, int g, int b, int *ph, int *ps, int *pv) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  *pv = maxc;
  if (minc == maxc) {
    *ph = 0, *ps = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr;
  const float gc = (float)(maxc - g) / cr;
  const float bc = (float)(maxc - b) / cr;
  double hd;
  if (r == maxc) {
    hd = (double)bc - (double)gc;
  } else if (g == maxc) {
    hd = 2.0 + (double)rc;
    hd = hd - (double)bc;
  } else {
    hd = 4.0 + (double)gc;
    hd = hd - (double)rc;
  }
  const float h = (float)hd;
  double x = (double)h / 6.0;
  x = x + 1.0;                    // in [5/6, 11/6]
  x = x - floor(x);               // fmod(x, 1.0): exact
  const float h2 = (float)x;
  const double hs = (double)h2 * 255.0;
  const float ss = s * 255.0f;
  *ph = jbc_clip8((int)hs);
  *ps = jbc_clip8((int)ss);
}

// round half away from zero (x >= 0 here), clipped to 0..255: Pillow's round() and CLIP8
JBC_FN int jbc_rnd8(float x) { return jbc_clip8((int)floor((double)x + 0.5)); }

// convert("RGB") of one HSV pixel, in float32
JBC_FN void jbc_hsv_to_rgb(int h, int s, int v, int *pr, int *pg, int *pb) {
  if (s == 0) {
    *pr = *pg = *pb = v;
    return;
  }
  const float h6 = (float)h * 6.0f;
  const float hh = h6 / 255.0f;
  const float fi = floorf(hh);
  const float f = hh - fi;
  const float fs = (float)s / 255.0f;
  const float fv = (float)v;
  const float a = 1.0f - fs;
  const float fsf = fs * f;
  const float bq = 1.0f - fsf;
  const float g1 = 1.0f - f;
  const float fsg = fs * g1;
  const float ct = 1.0f - fsg;
  const float xp = fv * a, xq = fv * bq, xt = fv * ct;
  const int p = jbc_rnd8(xp), q = jbc_rnd8(xq), t = jbc_rnd8(xt);
  switch ((int)fi % 6) {
    case 0: *pr = v, *pg = t, *pb = p; break;
    case 1: *pr = q, *pg = v, *pb = p; break;
    case 2: *pr = p, *pg = v, *pb = t; break;
    case 3: *pr = p, *pg = q, *pb = v; break;
    case 4: *pr = t, *pg = p, *pb = v; break;
    default: *pr = v, *pg = p, *pb = q; break;
  }
}

// ---- statistics operations: JB_COLOR_CONTRAST (one number, the mean), JB_COLOR_AUTOCONTRAST and JB_COLOR_EQUALIZE (a table of
// 256 bytes per channel from the channel's histogram) ----
JBC_FN bool jbc_is_hist(int op) { return op == JB_COLOR_AUTOCONTRAST || op == JB_COLOR_EQUALIZE; }
JBC_FN bool jbc_is_stat(int op) { return op == JB_COLOR_CONTRAST || jbc_is_hist(op); }
JBC_FN bool jbc_is_nbhd(int op) { return op == JB_COLOR_BLUR || op == JB_COLOR_SHARPNESS; }

// where a chain's statistics operations stand (in order; jb_color_check allows JB_COLOR_STATS_MAX, one of them a contrast) and
// where its neighbourhood operation stands (one, no statistics operation behind it); -1: none
// Two plain members, not an array: an index that is not a constant (a kernel's `round`) would make the compiler keep every
// thread's JbcShape in LDS.
struct JbcShape {
  int stat0, stat1;  // the first and the second statistics operation (JB_COLOR_STATS_MAX = 2)
  int n_stats, contrast, nbhd;
};
static_assert(JB_COLOR_STATS_MAX == 2, "JbcShape names its statistics operations");
// the index of statistics operation k (0, 1) of the chain
JBC_FN int jbc_stat_at(const JbcShape &s, int k) { return k == 0 ? s.stat0 : s.stat1; }
JBC_FN JbcShape jbc_shape(const jb_color_chain &c) {
  JbcShape s;
  s.stat0 = s.stat1 = -1, s.n_stats = 0, s.contrast = -1, s.nbhd = -1;
  for (int i = 0; i < c.n_ops && i < JB_COLOR_OPS_MAX; i++) {
    const int op = c.ops[i].op;
    if (jbc_is_stat(op)) {
      if (s.n_stats == 0) s.stat0 = i;
      if (s.n_stats == 1) s.stat1 = i;
      s.n_stats++;
      if (op == JB_COLOR_CONTRAST && s.contrast < 0) s.contrast = i;
    } else if (jbc_is_nbhd(op) && s.nbhd < 0) {
      s.nbhd = i;
    }
  }
  return s;
}

// What the operations of a chain read beside the pixel: the contrast's mean, and the tables (3 x 256 bytes, R then G then B) of
// the chain's histogram operations -- lut[0] is the table of the FIRST statistics operation (when it has one), lut[1] of the
// second, which stands at index at1 (-1: the chain has no second one).  Only finished statistics are read: whoever applies
// ops [first, last) has the results of every statistics operation in that range.
struct JbcCtx {
  int mean, at1;
  const uint8_t *lut[JB_COLOR_STATS_MAX];
};

// ImageOps.autocontrast (cutoff 0): entry ix of a channel whose first / last non-empty bins are lo / hi.  fp64, one operation
// per statement; Python's int() truncates toward zero, then the clamp.
JBC_FN int jbc_autocontrast_entry(int lo, int hi, int ix) {
  if (hi <= lo) return ix;
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = (double)(-lo) * scale;
  double t = (double)ix * scale;
  t = t + offset;
  return t <= 0.0 ? 0 : t >= 255.0 ? 255 : (int)t;
}
// ImageOps.equalize: entry i of a channel; before = h[0] + .. + h[i - 1], step = (N - h[last non-empty bin]) div 255, or 0 for
// a channel with fewer than two non-empty bins.  step / 2 + before can pass 2^32: 64-bit.  The min is Pillow's.
JBC_FN int jbc_equalize_entry(uint32_t step, uint32_t before, int i) {
  if (step == 0) return i;
  const uint64_t q = ((uint64_t)(step >> 1) + (uint64_t)before) / (uint64_t)step;
  return q > 255 ? 255 : (int)q;
}
// the table of one channel from its 256 counts, one entry after the other (the host; the device's table kernel finds lo, hi
// and the prefix sums in parallel and calls the two functions above)
JBC_FN void jbc_lut_from_counts(int op, const uint32_t *h, uint8_t *lut) {
  int lo = 256, hi = -1;
  uint64_t n = 0;
  for (int i = 0; i < 256; i++) {
    if (h[i]) lo = lo == 256 ? i : lo, hi = i;
    n += h[i];
  }
  if (hi < 0) lo = hi = 0;
  const uint32_t step = hi > lo ? (uint32_t)((n - h[hi]) / 255u) : 0u;
  uint32_t before = 0;
  for (int i = 0; i < 256; i++) {
    lut[i] = (uint8_t)(op == JB_COLOR_EQUALIZE ? jbc_equalize_entry(step, before, i) : jbc_autocontrast_entry(lo, hi, i));
    before += h[i];
  }
}

// ImageFilter.SMOOTH (Filter.c's 3 x 3, kernel (1 1 1, 1 5 1, 1 1 1) / 13) of one sample: a = the three samples of the row
// below, b = of the sample's own row, c = of the row above.  float32; every product and every sum rounded separately.
JBC_FN float jbc_smooth_row(int p0, int p1, int p2, float k0, float k1, float k2) {
  const float m0 = (float)p0 * k0;
  const float m1 = (float)p1 * k1;
  const float m2 = (float)p2 * k2;
  const float s = m0 + m1;
  return s + m2;
}
JBC_FN int jbc_smooth(int a0, int a1, int a2, int b0, int b1, int b2, int c0, int c1, int c2) {
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float acc = 0.5f;
  acc = acc + jbc_smooth_row(a0, a1, a2, k1, k1, k1);
  acc = acc + jbc_smooth_row(b0, b1, b2, k1, k5, k1);
  acc = acc + jbc_smooth_row(c0, c1, c2, k1, k1, k1);
  return acc <= 0.0f ? 0 : acc >= 255.0f ? 255 : (int)acc;
}

// operation i of a chain on one pixel; s: the chain's context (JB_COLOR_CONTRAST reads the mean, the two table operations
// their table).  op is uniform over a view -- on the device over a wave -- so the switch does not diverge.
// NEW_OPS = false compiles the operations numbered from 10 out (their case labels fall into the default): the switch is then
// the one over the six operations that it was before there were more, with no memory access in it.  The kernels run such
// instantiations for the launches whose chains hold none of those operations.
template <bool NEW_OPS>
JBC_FN void jbc_apply_op(int op, float value, const JbcCtx &s, int i, int *r, int *g, int *b) {
  switch (op) {
    case JB_COLOR_BRIGHTNESS:
      *r = jbc_blend(0, *r, value), *g = jbc_blend(0, *g, value), *b = jbc_blend(0, *b, value);
      break;
    case JB_COLOR_CONTRAST:
      *r = jbc_blend(s.mean, *r, value), *g = jbc_blend(s.mean, *g, value), *b = jbc_blend(s.mean, *b, value);
      break;
    case JB_COLOR_SATURATION: {
      const int l = jbc_luma(*r, *g, *b);
      *r = jbc_blend(l, *r, value), *g = jbc_blend(l, *g, value), *b = jbc_blend(l, *b, value);
      break;
    }
    case JB_COLOR_HUE: {
      int h, sat, v;
      jbc_rgb_to_hsv(*r, *g, *b, &h, &sat, &v);
      h = (h + (int)value) & 255;
      jbc_hsv_to_rgb(h, sat, v, r, g, b);
      break;
    }
    case JB_COLOR_GRAYSCALE:
      *r = *g = *b = jbc_luma(*r, *g, *b);
      break;
    case JB_COLOR_SOLARIZE: {
      const int t = (int)value;
      *r = *r < t ? *r : 255 - *r, *g = *g < t ? *g : 255 - *g, *b = *b < t ? *b : 255 - *b;
      break;
    }
    case JB_COLOR_POSTERIZE:
      if constexpr (NEW_OPS) {
        const int keep = ~((1 << (8 - (int)value)) - 1);
        *r &= keep, *g &= keep, *b &= keep;
      }
      break;
    case JB_COLOR_INVERT:
      if constexpr (NEW_OPS) *r = 255 - *r, *g = 255 - *g, *b = 255 - *b;
      break;
    case JB_COLOR_AUTOCONTRAST:
    case JB_COLOR_EQUALIZE:
      if constexpr (NEW_OPS) {
        const uint8_t *const t = i == s.at1 ? s.lut[1] : s.lut[0];
        *r = t[*r], *g = t[256 + *g], *b = t[512 + *b];
      }
      break;
    default: break;
  }
}

// ops [first, last) of a chain on one pixel
template <bool NEW_OPS>
JBC_FN void jbc_apply_ops(const jb_color_chain &c, int first, int last, const JbcCtx &s, int *r, int *g, int *b) {
  for (int i = first; i < last; i++) jbc_apply_op<NEW_OPS>(c.ops[i].op, c.ops[i].value, s, i, r, g, b);
}
// does the chain hold a pointwise or table operation numbered from 10?
JBC_FN bool jbc_has_new_ops(const jb_color_chain &c) {
  for (int i = 0; i < c.n_ops && i < JB_COLOR_OPS_MAX; i++)
    if (c.ops[i].op >= JB_COLOR_POSTERIZE && c.ops[i].op <= JB_COLOR_EQUALIZE) return true;
  return false;
}

// ---- geometric operations (JB_COLOR_SHEAR_X .. JB_COLOR_ROTATE): Pillow's nearest-neighbour affine transform ----
JBC_FN bool jbc_is_warp(int op) { return op >= JB_COLOR_SHEAR_X && op <= JB_COLOR_ROTATE; }

// where a chain's geometric operations stand (in order; jb_color_check allows JB_COLOR_WARPS_MAX); -1: none.  Beside JbcShape,
// not in it: the kernels of the launches without a geometric operation never ask.
struct JbcWarpShape {
  int warp0, warp1;
};
static_assert(JB_COLOR_WARPS_MAX == 2, "JbcWarpShape names its geometric operations");
JBC_FN JbcWarpShape jbc_warp_shape(const jb_color_chain &c) {
  JbcWarpShape s;
  s.warp0 = s.warp1 = -1;
  for (int i = 0; i < c.n_ops && i < JB_COLOR_OPS_MAX; i++)
    if (jbc_is_warp(c.ops[i].op)) {
      if (s.warp0 < 0) s.warp0 = i;
      else if (s.warp1 < 0) s.warp1 = i;
    }
  return s;
}

// one geometric operation as the kernels get it: Pillow's path and its six integers (jb_warp_params); 32 bytes
struct JbWarp {
  int32_t mode, coef[6], pad;
};

// (x, y) of the view behind the operation -> the position it reads in the view in front; false: outside the view.  The sums
// wrap like Pillow's int additions: jb_warp_params takes the fixed path only where the corners' positions fit 16.16.
JBC_FN bool jbc_warp_back(const JbWarp &k, int w, int h, int *x, int *y) {
  int xin, yin;
  if (k.mode == JB_WARP_SHIFT) {
    xin = *x + k.coef[2], yin = *y + k.coef[5];
  } else {
    const uint32_t ux = (uint32_t)*x, uy = (uint32_t)*y;
    xin = (int32_t)((uint32_t)k.coef[2] + uy * (uint32_t)k.coef[1] + ux * (uint32_t)k.coef[0]) >> 16;
    yin = (int32_t)((uint32_t)k.coef[5] + uy * (uint32_t)k.coef[4] + ux * (uint32_t)k.coef[3]) >> 16;
  }
  *x = xin, *y = yin;
  return xin >= 0 && xin < w && yin >= 0 && yin < h;
}

// Pixel (x, y) of the view AS IT STANDS in front of op `last` of a chain with geometric operations, from the w x h source
// at src (rows `stride` bytes apart): (x, y) backwards through the geometric operations in front of `last` -- wk[0] is
// ws.warp0's, wk[1] ws.warp1's --, three byte loads there, then ops [0, last) forwards, a geometric operation setting the
// pixel to black where ITS position fell outside.  A position outside is replaced by (0, 0): every load lies inside the view.
// The chain is uniform over a view; only the two selects are per pixel.
template <bool NEW_OPS>
JBC_FN void jbc_gather(const jb_color_chain &c, const JbcWarpShape &ws, int last, const JbcCtx &s, const JbWarp *wk, const uint8_t *src,
                       int64_t stride, int w, int h, int x, int y, int *r, int *g, int *b) {
  bool out0 = false, out1 = false;
  if (ws.warp1 >= 0 && ws.warp1 < last) {
    out1 = !jbc_warp_back(wk[1], w, h, &x, &y);
    if (out1) x = 0, y = 0;
  }
  if (ws.warp0 >= 0 && ws.warp0 < last) {
    out0 = !jbc_warp_back(wk[0], w, h, &x, &y);
    if (out0) x = 0, y = 0;
  }
  const uint8_t *const from = src + (int64_t)y * stride + 3 * (int64_t)x;
  *r = from[0], *g = from[1], *b = from[2];
  for (int i = 0; i < last; i++) {
    if (i == ws.warp0) {
      if (out0) *r = 0, *g = 0, *b = 0;
    } else if (i == ws.warp1) {
      if (out1) *r = 0, *g = 0, *b = 0;
    } else {
      jbc_apply_op<NEW_OPS>(c.ops[i].op, c.ops[i].value, s, i, r, g, b);
    }
  }
}

// Python's round(x, 15): the correctly rounded decimal with 15 places, read back (host only)
inline double jbc_round15(double x) {
  char text[64];
  snprintf(text, sizeof text, "%.15f", x);
  return strtod(text, nullptr);
}

// The ONE text of a geometric operation's coefficients (include/jpegblk.h states it): the inverse matrix in doubles, one
// operation per statement (built with -ffp-contract=off), then Pillow's choice of path.  Host only: the kernels get the integers.
// JB_OK, JB_ERR_GEOMETRY (the value, the size or the op) or JB_ERR_UNSUPPORTED (Pillow's scaling or float path); *why says which.
inline int jbc_warp_params(int op, float value, int32_t w, int32_t h, JbWarp *o, const char **why) {
  *why = "the op is not geometric";
  if (!jbc_is_warp(op)) return JB_ERR_GEOMETRY;
  *why = "the size is outside 1..65535";
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return JB_ERR_GEOMETRY;
  *why = "the value of a geometric operation is not finite";
  if (!(value >= -3.402823466e38f && value <= 3.402823466e38f)) return JB_ERR_GEOMETRY;
  const double v = (double)value;
  const double pi = 3.141592653589793;
  double m[6];
  if (op == JB_COLOR_ROTATE) {
    double deg = fmod(v, 360.0);  // Python's %: the result takes the divisor's sign
    if (deg != 0.0) {
      if (deg < 0.0) deg = deg + 360.0;
    } else {
      deg = 0.0;
    }
    const double rad = deg * (pi / 180.0);
    const double g = -rad;
    const double cg = cos(g), sg = sin(g);
    // (two conversions, not four: a correctly rounded conversion is odd, round15(-s) = -round15(s))
    const double rc = jbc_round15(cg), rs = jbc_round15(sg);
    m[0] = rc, m[1] = rs, m[2] = 0.0;
    m[3] = -rs, m[4] = rc, m[5] = 0.0;
    const double cx = (double)w / 2.0, cy = (double)h / 2.0;
    const double nx = -cx, ny = -cy;
    const double p0 = m[0] * nx, p1 = m[1] * ny;
    const double s01 = p0 + p1;
    const double q0 = m[3] * nx, q1 = m[4] * ny;
    const double s34 = q0 + q1;
    m[2] = s01 + m[2];
    m[5] = s34 + m[5];
    m[2] = m[2] + cx;
    m[5] = m[5] + cy;
  } else {
    double sx = 0.0, sy = 0.0, cx = 0.0, cy = 0.0, tx = 0.0, ty = 0.0;
    if (op == JB_COLOR_SHEAR_X || op == JB_COLOR_SHEAR_Y) {
      const double at = atan(v);
      const double deg = at * (180.0 / pi);
      const double rad = deg * (pi / 180.0);
      if (op == JB_COLOR_SHEAR_X) sx = rad;
      else sy = rad;
    } else {
      *why = "a translation is not integral or its absolute value is above 65535";
      if (v != floor(v) || v < -65535.0 || v > 65535.0) return JB_ERR_GEOMETRY;
      cx = (double)w * 0.5, cy = (double)h * 0.5;
      if (op == JB_COLOR_TRANSLATE_X) tx = v;
      else ty = v;
    }
    const double rot = 0.0;
    const double rs = rot - sy;
    const double crs = cos(rs), srs = sin(rs), csy = cos(sy), tsx = tan(sx), srot = sin(rot), crot = cos(rot);
    const double A = crs / csy;
    const double b0 = -crs;
    const double b1 = b0 * tsx;
    const double b2 = b1 / csy;
    const double B = b2 - srot;
    const double C = srs / csy;
    const double d0 = -srs;
    const double d1 = d0 * tsx;
    const double d2 = d1 / csy;
    const double D = d2 + crot;
    m[0] = D, m[1] = -B, m[2] = 0.0, m[3] = -C, m[4] = A, m[5] = 0.0;
    const double ex = -cx - tx, ey = -cy - ty;
    const double p0 = m[0] * ex, p1 = m[1] * ey;
    const double s01 = p0 + p1;
    const double q0 = m[3] * ex, q1 = m[4] * ey;
    const double s34 = q0 + q1;
    m[2] = m[2] + s01;
    m[5] = m[5] + s34;
    m[2] = m[2] + cx;
    m[5] = m[5] + cy;
  }
  JbWarp k;
  k.pad = 0;
  if (m[1] == 0.0 && m[3] == 0.0) {
    *why = "a matrix of Pillow's scaling path (a rotation by 180 degrees is one)";
    if (m[0] != 1.0 || m[4] != 1.0 || m[2] != floor(m[2]) || m[5] != floor(m[5])) return JB_ERR_UNSUPPORTED;
    k.mode = JB_WARP_SHIFT;
    k.coef[0] = k.coef[1] = k.coef[3] = k.coef[4] = 0;
    k.coef[2] = (int32_t)m[2], k.coef[5] = (int32_t)m[5];
  } else {
    *why = "a matrix of Pillow's float path (a corner's position does not fit 16.16 fixed point)";
    const double xs[4] = {0.0, (double)w, 0.0, (double)w}, ys[4] = {0.0, 0.0, (double)h, (double)h};
    for (int i = 0; i < 4; i++) {
      const double a0 = xs[i] * m[0], a1 = ys[i] * m[1];
      const double a01 = a0 + a1;
      const double ax = a01 + m[2];
      const double c0 = xs[i] * m[3], c1 = ys[i] * m[4];
      const double c01 = c0 + c1;
      const double ay = c01 + m[5];
      if (!(fabs(ax) < 32768.0) || !(fabs(ay) < 32768.0)) return JB_ERR_UNSUPPORTED;
    }
    const auto fix = [](double t) {
      const double s = t * 65536.0;
      const double u = s + 0.5;
      return u < 0.0 ? (int32_t)floor(u) : (int32_t)u;
    };
    const double h0 = m[0] * 0.5, h1 = m[1] * 0.5, h3 = m[3] * 0.5, h4 = m[4] * 0.5;
    const double e2 = m[2] + h0, e5 = m[5] + h3;
    const double f2 = e2 + h1, f5 = e5 + h4;
    const double all[6] = {m[0], m[1], f2, m[3], m[4], f5};
    // (FIX must fit int32; with the corners inside +-32768 the five operations' matrices always do: not reached)
    for (int i = 0; i < 6; i++)
      if (!(fabs(all[i]) * 65536.0 + 0.5 < 2147483648.0)) return JB_ERR_UNSUPPORTED;
    k.mode = JB_WARP_FIXED;
    for (int i = 0; i < 6; i++) k.coef[i] = fix(all[i]);
  }
  *o = k;
  *why = nullptr;
  return JB_OK;
}

// ---- JB_COLOR_BLUR: Pillow's ImageFilter.GaussianBlur, three extended box blur passes along the rows, then three along
// the columns, each rounded to uint8 (BoxBlur.c) ----
// The weights of one pass: box radius r, 8.24 weights ww (the 2 r + 1 samples of the box) and fw (the two samples beside it).
struct JbBlurWeights {
  int32_t r;
  uint32_t ww, fw;
};

// Pillow's _gaussian_blur_radius and ImagingLineBoxBlur's weights.  Only the HOST evaluates this (jb_blur_params): the double
// sqrt and the float32 steps decide bits, and the weights travel to the kernel as three integers.  One operation per statement.
// false: the radius is negative or not finite (*geometry = true), or r > JB_COLOR_BLUR_BOX_MAX (*geometry = false).
JBC_FN bool jbc_blur_weights(float radius, JbBlurWeights *o, bool *geometry) {
  *geometry = true;
  if (!(radius >= 0.0f) || !(radius <= 3.402823466e38f)) return false;
  *geometry = false;
  const float rr = radius * radius;
  const float sigma2 = rr / 3.0f;
  const double l12 = 12.0 * (double)sigma2;
  const double l121 = l12 + 1.0;
  const float L = (float)sqrt(l121);
  const double lm1 = (double)L - 1.0;
  const float l = (float)floor(lm1 / 2.0);
  if (!(l <= (float)JB_COLOR_BLUR_BOX_MAX)) return false;  // (a radius whose square is not finite too)
  const float l2 = 2.0f * l;
  const float l21 = l2 + 1.0f;
  const float lp1 = l + 1.0f;
  const float llp1 = l * lp1;
  const float s3 = 3.0f * sigma2;
  const float d1 = llp1 - s3;
  const float num = l21 * d1;
  const float sq = lp1 * lp1;
  const float d2 = sigma2 - sq;
  const float den = 6.0f * d2;
  const float a = num / den;
  const float fr = l + a;
  if (!(fr < (float)(JB_COLOR_BLUR_BOX_MAX + 1))) return false;
  const int32_t r = (int32_t)fr;
  const float f2 = fr * 2.0f;
  const float f21 = f2 + 1.0f;
  const float wq = 16777216.0f / f21;
  const uint32_t ww = (uint32_t)wq;
  o->r = r;
  o->ww = ww;
  o->fw = (16777216u - (uint32_t)(2 * r + 1) * ww) / 2u;
  return true;
}

// one sample of one pass: box = the sum of the 2 r + 1 samples of the box, sides = the sum of the two samples beside it.
// Exact in uint32: ww (2 r + 1) + 2 fw <= 2^24.
JBC_FN uint32_t jbc_blur_sample(uint32_t ww, uint32_t fw, uint32_t box, uint32_t sides) { return (ww * box + fw * sides + (1u << 23)) >> 24; }

// one pass along one line: samples first..last-1 of `out` from `in`, both addressed in[i * stride]; a read of position i goes to
// min(max(i, lo), hi), the view's two edge samples on this line.  The box sum runs along the line: two reads a sample, whatever r.
// STRIDE: int for the kernel's tile, int64_t for the host's whole image.
// in and out never overlap, and the reads of a sample do not depend on the sums in front of it: eight samples' reads are
// issued together (on the device one wait for sixteen LDS loads, not eight waits for two), then the running sum goes along.
template <typename STRIDE>
JBC_FN void jbc_blur_line(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, STRIDE stride, int first, int last, int lo, int hi,
                          const JbBlurWeights &k) {
  if (first >= last) return;
  const int r = k.r;
#define JBC_AT(i) ((uint32_t)in[((i) < lo ? lo : (i) > hi ? hi : (i)) * stride])
  uint32_t box = 0;
  for (int j = -r; j <= r; j++) box += JBC_AT(first + j);
  uint32_t left = JBC_AT(first - r - 1);
  int x = first;
  for (; x + 8 <= last; x += 8) {
    uint32_t right[8], leave[8];
#pragma unroll
    for (int j = 0; j < 8; j++) right[j] = JBC_AT(x + j + r + 1), leave[j] = JBC_AT(x + j - r);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      out[(x + j) * stride] = (uint8_t)jbc_blur_sample(k.ww, k.fw, box, left + right[j]);
      left = leave[j];
      box = box + right[j] - left;
    }
  }
  for (; x < last; x++) {
    const uint32_t right = JBC_AT(x + r + 1);
    out[x * stride] = (uint8_t)jbc_blur_sample(k.ww, k.fw, box, left + right);
    left = JBC_AT(x - r);  // (the left neighbour of the box of x + 1: the sample that leaves the box)
    box = box + right - left;
  }
#undef JBC_AT
}
