// filter_plan_check.cpp -- the pure host code of "resampling filters" (csrc/jb_geometry.cpp: the plan's refusals,
// jb_filter_check, jb_filter_window; csrc/jb_filter.h) under AddressSanitizer + UBSan: random descriptors, rectangles,
// targets and filters -- valid, on the edges and out of range -- through the public entry points and through the plan
// with per-image rectangles.  Every accepted request's window must be the brute-force union of the outputs' bounds, hold
// the rectangle and lie in the frame; every answer must be a status.  Usage: filter_plan_check [iterations] [seed]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/jpegblk.h"
#include "../../jpeg_decoder_amd/csrc/jb_filter.h"
#include "../../jpeg_decoder_amd/csrc/jb_plan.h"

static int fails = 0;
#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                                 \
  } while (0)

int main(int argc, char **argv) {
  const long iterations = argc > 1 ? atol(argv[1]) : 200000;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  auto pick = [&](int64_t lo, int64_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  const int32_t odd[] = {INT32_MIN, -1, 0, 1, 2, 65535, 65536, INT32_MAX};
  auto any = [&](int64_t lo, int64_t hi) { return rng() % 16 == 0 ? odd[rng() % 8] : pick(lo, hi); };
  long accepted = 0, capped = 0;
  for (long it = 0; it < iterations; it++) {
    jb_image_desc d = {any(1, rng() % 4 ? 300 : 65535), any(1, rng() % 4 ? 300 : 65535), 1 + (int)(rng() % 2), 1 + (int)(rng() % 2), {0, 1, 1}, 0};
    const bool whole = rng() % 4 == 0;
    jb_roi r = {any(0, 300), any(0, 300), any(1, 300), any(1, 300)};
    if (rng() % 2 && d.width > 0 && d.height > 0) {  // mostly inside the frame
      r.width = pick(1, d.width), r.height = pick(1, d.height);
      r.x = pick(0, d.width - r.width), r.y = pick(0, d.height - r.height);
    }
    jb_resize rs = {any(1, rng() % 4 ? 64 : 65535), any(1, rng() % 4 ? 64 : 65535), rng() % 8 ? 1 + (int)(rng() % 2) : any(-1, 3), rng() % 32 ? 0 : 1};
    jb_roi win = {-7, -7, -7, -7};
    const int rc = jb_filter_window(&d, whole ? nullptr : &r, &rs, &win);
    EXPECT(rc == jb_filter_check(&d, whole ? nullptr : &r, &rs));
    EXPECT(rc <= 0 && rc >= JB_ERR_UNSUPPORTED);
    if (rc == JB_ERR_UNSUPPORTED) capped++;
    // the plan with the same rectangle as a batch of three per-image rectangles answers alike (a rectangle's refusal names it)
    if (!whole) {
      const jb_roi three[3] = {r, r, r};
      const JbTarget t = {rs.out_w, rs.out_h, rs.filter, rs.reserved};
      const JbOutPlan plan = jb_out_plan_(&d, 1, nullptr, nullptr, &t, three, 3);
      jb_geometry g;
      if (jb_geometry_of(&d, &g) == JB_OK) EXPECT(plan.status == rc);
      if (plan.status == JB_ERR_UNSUPPORTED) EXPECT(plan.bad_crop == 0);
    }
    if (rc != JB_OK) {
      EXPECT(win.x == -7);
      continue;
    }
    accepted++;
    const jb_roi q = whole ? jb_roi{0, 0, d.width, d.height} : r;
    if (rs.filter == JB_FILTER_AREA) {
      EXPECT(win.x == q.x && win.y == q.y && win.width == q.width && win.height == q.height);
      continue;
    }
    for (int axis = 0; axis < 2; axis++) {
      const int in_size = axis ? d.height : d.width, in0 = axis ? q.y : q.x, len = axis ? q.height : q.width, n = axis ? rs.out_h : rs.out_w;
      const int w0 = axis ? win.y : win.x, w1 = w0 + (axis ? win.height : win.width);
      const JbFilterAxis a = jb_filter_axis(rs.filter, in_size, in0, in0 + len, n);
      EXPECT(jb_filter_taps(a) <= kJbFilterMaxTaps);
      int lo_min = in_size, hi_max = 0;
      const int step = n > 4096 ? n / 2048 : 1;  // (every output of a small axis, a sample and both ends of a large one)
      for (int j = 0; j < n; j = (j + step < n || j == n - 1) ? j + step : n - 1) {
        double c;
        int lo, hi;
        jb_filter_bounds(a, j, &c, &lo, &hi);
        EXPECT(hi > lo && hi - lo <= jb_filter_taps(a) && lo >= 0 && hi <= in_size);
        if (lo < lo_min) lo_min = lo;
        if (hi > hi_max) hi_max = hi;
        double ww = 0.0;
        for (int t = 0; t < hi - lo; t++) ww += jb_filter_weight(a, lo, c, t);
        long long sum = 0;
        for (int t = 0; t < hi - lo; t++) sum += jb_filter_fixed(ww != 0.0 ? jb_filter_weight(a, lo, c, t) / ww : jb_filter_weight(a, lo, c, t));
        EXPECT(sum > 4194304 - 2 * (hi - lo) && sum < 4194304 + 2 * (hi - lo));  // the weights of an output sum to one
      }
      EXPECT(w0 == lo_min && w1 == hi_max);
      EXPECT(w0 >= 0 && w1 <= in_size && w0 <= in0 && w1 >= in0 + len);
    }
  }
  printf("filter_plan_check: %ld requests, %ld accepted, %ld over the tap cap, %d failed expectations\n", iterations, accepted, capped, fails);
  return fails ? 1 : 0;
}
