// tools/frontend_host_bench.cpp -- host time of the front end without a device: jb_entropy_decode on one thread,
// jb_huff_prepare_, and jb_decode_memory's host route with the device half stubbed (parse, scan decode, no pixels).
// Built from a csrc directory's front-end sources, so that two commits can be built side by side and run in turns:
//   g++ -O3 -std=c++17 -pthread -I<csrc> -o bench tools/frontend_host_bench.cpp <csrc>/jb_frontend.cpp <csrc>/jb_frontend_ext.cpp
//       <csrc>/jb_geometry.cpp <csrc>/jb_exif.cpp <csrc>/jb_huff_pack.cpp <csrc>/jb_hostutil.cpp
//   ./bench file.jpg [repeats]      -> "<file> decode_us prepare_us decode_memory_host_us" (the median of the repeats)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/jpegblk.h"
#include "jb_internal.h"

static std::string g_err;
static JbKnobs g_knobs;
int jb_fail_(jb_ctx *, int code, const char *msg) {
  g_err = msg ? msg : "";
  return code;
}
void jb_ctx_set_last_desc_(jb_ctx *, const jb_image_desc *) {}
const JbKnobs *jb_ctx_knobs_(const jb_ctx *) { return &g_knobs; }
int jb_decode_job_(jb_ctx *, const JbHuffJob *, uint8_t *, const JbOutPlan &) { return JB_OK; }
int jb_blocks_to_rgb_plan_(jb_ctx *, const jb_image_desc *, const int16_t *, const uint16_t *, uint8_t *, const JbOutPlan &) { return JB_OK; }
extern "C" {
const char *jb_last_error(const jb_ctx *) { return g_err.c_str(); }
void *jb_pinned_alloc(size_t n) { return malloc(n); }
void *jb_pinned_alloc_on(int, size_t n) { return malloc(n); }
int jb_ctx_reserve(jb_ctx *, size_t, size_t) { return JB_OK; }
int jb_ctx_device(const jb_ctx *) { return 0; }
int jb_ctx_orientation(const jb_ctx *) { return JB_ORIENT_STORED; }
int jb_ctx_arithmetic(const jb_ctx *) { return JB_ARITH_REFERENCE; }
int jb_ctx_draft(const jb_ctx *) { return 1; }
void jb_pinned_free(void *p) { free(p); }
int jb_device_numa_node(int) { return JB_ERR_STATE; }
}

template <class F> static double median_us(int repeats, F f) {
  std::vector<double> t;
  for (int i = 0; i < repeats; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::vector<uint8_t> f;
  if (!jb_read_file_(argv[1], f)) return 2;
  const int repeats = argc > 2 ? atoi(argv[2]) : 21;
  jb_image_desc d;
  uint16_t q[256];
  if (jb_entropy_decode(f.data(), f.size(), &d, q, nullptr, 0) != JB_OK) return 1;
  jb_geometry g;
  jb_geometry_of(&d, &g);
  std::vector<int16_t> coef((size_t)g.coef_bytes / 2);
  static JbHuffJob job;
  static int dummy;
  g_knobs.gpu_huffman = 0;  // jb_decode_memory: the host route
  int bad = 0;
  const double decode = median_us(repeats, [&] { bad |= jb_entropy_decode(f.data(), f.size(), &d, q, coef.data(), (size_t)g.coef_bytes); });
  const double prepare = median_us(repeats, [&] { bad |= jb_huff_prepare_(f.data(), f.size(), &job, nullptr); });
  const double memory = median_us(repeats, [&] {
    uint8_t *rgb = nullptr;
    int32_t w, h;
    bad |= jb_decode_memory((jb_ctx *)&dummy, f.data(), f.size(), &rgb, &w, &h);
    free(rgb);
  });
  printf("%s %.1f %.1f %.1f\n", argv[1], decode, prepare, memory);
  return bad ? 1 : 0;
}
