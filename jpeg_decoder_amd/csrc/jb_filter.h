// jb_filter.h -- "resampling filters" (include/jpegblk.h): the weight arithmetic of one axis, operation for operation
// as the header states it, in ONE place for the host (jb_geometry.cpp: the source window and the tap cap) and the device
// (jb_resample.hip: the weight tables).  Only + - * /, compares and truncating conversions on IEEE doubles, never
// contracted (the build uses -ffp-contract=off), so both sides get the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JB_HD __host__ __device__ inline
#else
#define JB_HD inline
#endif

// The cap on the taps of one axis (include/jpegblk.h names it): what the kernel's weight table in LDS is sized for.
// A 32x bicubic reduction counts 2 * 2 * 32 + 2 = 130.
constexpr int kJbFilterMaxTaps = 160;

// one axis of a filtered resize: frame extent in_size, rectangle [in0, in1), n outputs
struct JbFilterAxis {
  double scale, sup, inv;
  int32_t in0, in_size;
  int32_t filter;  // JB_FILTER_BILINEAR (1) or JB_FILTER_BICUBIC (2)
};

JB_HD JbFilterAxis jb_filter_axis(int filter, int in_size, int in0, int in1, int n) {
  JbFilterAxis a;
  a.scale = (double)(in1 - in0) / (double)n;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.sup = (filter == 2 ? 2.0 : 1.0) * fs;
  a.inv = 1.0 / fs;
  a.in0 = in0, a.in_size = in_size, a.filter = filter;
  return a;
}

// output j reads source samples [*lo, *hi); *center for jb_filter_weight
JB_HD void jb_filter_bounds(const JbFilterAxis &a, int j, double *center, int *lo, int *hi) {
  const double c = (double)a.in0 + ((double)j + 0.5) * a.scale;
  int l = (int)(c - a.sup + 0.5);
  if (l < 0) l = 0;
  int h = (int)(c + a.sup + 0.5);
  if (h > a.in_size) h = a.in_size;
  *center = c, *lo = l, *hi = h;
}

// the filter's value for tap t of an output with bounds [lo, ...) and `center`, before the normalisation
JB_HD double jb_filter_weight(const JbFilterAxis &a, int lo, double center, int t) {
  double x = ((double)(t + lo) - center + 0.5) * a.inv;
  if (x < 0.0) x = -x;
  if (a.filter == 2) {
    const double k = -0.5;
    if (x < 1.0) return ((k + 2.0) * x - (k + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * k;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;
}

// a normalised weight in 22-bit fixed point, rounded half away from zero
JB_HD int32_t jb_filter_fixed(double w) { return w < 0.0 ? (int32_t)(w * 4194304.0 - 0.5) : (int32_t)(w * 4194304.0 + 0.5); }

// The taps of an axis as the cap counts them: floor(2 * sup) + 2, an upper bound of hi - lo for every output (two
// truncations 2 * sup apart differ by at most floor(2 * sup) + 1; one more for the roundings of center -+ sup + 0.5).
JB_HD int jb_filter_taps(const JbFilterAxis &a) { return (int)(2.0 * a.sup) + 2; }

// the samples the axis reads at all: centers grow with j, so the union of [lo, hi) is [lo of output 0, hi of output n - 1)
JB_HD void jb_filter_span(const JbFilterAxis &a, int n, int *lo, int *hi) {
  double c;
  int other;
  jb_filter_bounds(a, 0, &c, lo, &other);
  jb_filter_bounds(a, n - 1, &c, &other, hi);
}
