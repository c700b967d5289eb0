// jb_color_core.h -- "colour chains" (include/jpegblk.h): the per-pixel arithmetic of every colour operation, in one
// place: jb_color.hip compiles it for gfx950, jb_color_host (jb_color.hip's host half) and the CPU tests the same text for
// the host.  It is Pillow's, operation for operation -- ImageEnhance.Brightness / Contrast / Color are Image.blend against
// a degenerate image, the hue shift is convert("HSV") and back, grayscale is convert("L"), solarize is ImageOps.solarize.
//
// Every float step is written as ONE operation per statement and the file is built with -ffp-contract=off and without
// fast-math: a product and the sum behind it stay two roundings, and f32 / f64 divisions are correctly rounded.
#pragma once
#include <math.h>
#include <stdint.h>

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

// one operation on one pixel; mean: the view's jbc_contrast_mean (JB_COLOR_CONTRAST alone reads it).  op is uniform over
// a view -- on the device over a wave -- so the switch does not diverge.
JBC_FN void jbc_apply_op(int op, float value, int mean, int *r, int *g, int *b) {
  switch (op) {
    case JB_COLOR_BRIGHTNESS:
      *r = jbc_blend(0, *r, value), *g = jbc_blend(0, *g, value), *b = jbc_blend(0, *b, value);
      break;
    case JB_COLOR_CONTRAST:
      *r = jbc_blend(mean, *r, value), *g = jbc_blend(mean, *g, value), *b = jbc_blend(mean, *b, value);
      break;
    case JB_COLOR_SATURATION: {
      const int l = jbc_luma(*r, *g, *b);
      *r = jbc_blend(l, *r, value), *g = jbc_blend(l, *g, value), *b = jbc_blend(l, *b, value);
      break;
    }
    case JB_COLOR_HUE: {
      int h, s, v;
      jbc_rgb_to_hsv(*r, *g, *b, &h, &s, &v);
      h = (h + (int)value) & 255;
      jbc_hsv_to_rgb(h, s, v, r, g, b);
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
    default: break;
  }
}

// ops [first, last) of a chain on one pixel
JBC_FN void jbc_apply_ops(const jb_color_chain &c, int first, int last, int mean, int *r, int *g, int *b) {
  for (int i = first; i < last; i++) jbc_apply_op(c.ops[i].op, c.ops[i].value, mean, r, g, b);
}

// the index of the chain's JB_COLOR_CONTRAST (jb_color_check allows one); -1: none
JBC_FN int jbc_contrast_at(const jb_color_chain &c) {
  for (int i = 0; i < c.n_ops && i < JB_COLOR_OPS_MAX; i++)
    if (c.ops[i].op == JB_COLOR_CONTRAST) return i;
  return -1;
}
