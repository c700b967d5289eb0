// lj_kernel_check -- jb_lj_block_kernel and jb_lj_pixel_kernel (csrc/jb_libjpeg.hip) and their two launchers compiled for
// the CPU: the built-ins are stubbed and a launch is a loop over block and thread index (the kernels have no barrier and no
// LDS).  Built with AddressSanitizer + UBSan; coefficients, planes and outputs are heap blocks of exactly the bytes the
// launch may touch, so a load or store outside them, or a misaligned wide store, is a report.  The cases come from a file
// that tools/fuzz/lj_kernel_cases.py writes: every file of the decode and draft known-answer sets at draft 1, 2, 4, 8 -- the
// whole frame through jbk_lj_launch, rectangles through jbk_lj_launch (roi) and jbk_lj_launch_crops -- with the bytes
// Pillow gives (draft 1: the decode KAT's; else the draft KAT's) as the expectation.
//   python3 lj_kernel_cases.py cases.bin && ./lj_kernel_check cases.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define JB_KERNELS_HOST
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
struct HostIdx {
  unsigned x;
};
static HostIdx threadIdx, blockIdx;
struct dim3 {
  unsigned x;
  explicit dim3(unsigned x_) : x(x_) {}
};
struct u32x4_t {
  uint32_t x, y, z, w;
};
struct alignas(8) uint2 {
  uint32_t x, y;
};
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
// v_mul_i32_i24: the product of the operands' low 24 bits, sign-extended; the low 32 bits of it
static inline int __mul24(int a, int b) {
  const int64_t x = (int64_t)((int32_t)((uint32_t)a << 8) >> 8), y = (int64_t)((int32_t)((uint32_t)b << 8) >> 8);
  return (int)(uint32_t)(uint64_t)(x * y);
}
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
static inline int hipGetLastError() { return hipSuccess; }
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                  \
  do {                                                                                               \
    for (unsigned b_ = 0; b_ < (grid).x; b_++)                                                      \
      for (unsigned t_ = 0; t_ < (block).x; t_++) {                                                 \
        blockIdx.x = b_, threadIdx.x = t_;                                                           \
        kernel(__VA_ARGS__);                                                                         \
      }                                                                                              \
  } while (0)
// binary16 where the host compiler has no _Float16: float -> half, round to nearest even (the device's one convert)
struct HostHalf {
  uint16_t bits;
  explicit HostHalf(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) bits = (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0));
    else if (mag >= 0x477ff000u) bits = (uint16_t)(sign | 0x7c00u);
    else if (mag < 0x33000001u) bits = (uint16_t)sign;
    else {
      const int e = (int)(mag >> 23) - 127;
      const uint32_t sig = (mag & 0x7fffffu) | 0x800000u;
      const int shift = e >= -14 ? 13 : 13 + (-14 - e);
      const uint32_t kept = sig >> shift, rest = sig & ((1u << shift) - 1), half = 1u << (shift - 1);
      uint32_t h = e >= -14 ? ((uint32_t)(e + 15) << 10) + (kept - 0x400u) : kept;
      if (rest > half || (rest == half && (h & 1))) h++;
      bits = (uint16_t)(sign | h);
    }
  }
};
#define _Float16 HostHalf
#include "../../jpeg_decoder_amd/csrc/jb_libjpeg.hip"

static const uint8_t kSent = 0xA5;
static long n_cases = 0;

// the exact bytes of a window's three planes (jbk_lj_window rounds them up to 256 for the next image's sake)
static int64_t exact_plane_bytes(const JbLjWindow &w, int hs, int vs, int draft) {
  int s = 8 / draft, sc = s;
  while (sc < 8 && (hs * s) % (2 * sc) == 0 && (vs * s) % (2 * sc) == 0) sc *= 2;
  return (int64_t)w.nx * w.ny * (hs * vs * s * s + 2 * sc * sc);
}

struct Case {
  int32_t w, h, hs, vs, draft, mcus_x, mcus_y, n_rects;
  std::vector<int32_t> rects;  // n_rects x (x, y, w, h) of the draft frame; the first one is the whole frame
  std::vector<int32_t> q;      // [3][64]
  std::vector<int16_t> coef;
  std::vector<uint8_t> image;  // the draft frame [oh][ow][3]
};

static bool read_exact(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

static void fail(const Case &c, const char *what, const int32_t *r) {
  printf("FAIL: %dx%d %dx%d draft %d rect (%d, %d, %d, %d): %s\n", c.w, c.h, c.hs, c.vs, c.draft, r[0], r[1], r[2], r[3], what);
  exit(1);
}

static void run(const Case &c) {
  const int ow = (c.w + c.draft - 1) / c.draft, oh = (c.h + c.draft - 1) / c.draft;
  const int nb = c.hs * c.vs + 2;
  // exactly-sized heap copies: the coefficients of the coded MCUs, the tables
  int16_t *coef = (int16_t *)malloc(c.coef.size() * 2);
  int32_t *q = (int32_t *)malloc(192 * 4);
  memcpy(coef, c.coef.data(), c.coef.size() * 2);
  memcpy(q, c.q.data(), 192 * 4);
  if ((int64_t)c.coef.size() != (int64_t)c.mcus_x * c.mcus_y * nb * 64) fail(c, "coefficient count", c.rects.data());
  JbLaunch base;
  memset(&base, 0, sizeof base);
  base.coef = coef, base.qtabs = q;
  base.width = ow, base.height = oh, base.mcus_x = c.mcus_x, base.mcus_y = c.mcus_y;
  // 1. every rectangle alone through jbk_lj_launch (the first one as the whole frame, without the ROI fields)
  for (int k = 0; k < c.n_rects; k++) {
    const int32_t *r = &c.rects[(size_t)k * 4];
    const JbLjWindow win = jbk_lj_window(c.hs, c.vs, c.draft, c.mcus_x, c.mcus_y, r[0], r[1], r[2], r[3]);
    uint8_t *planes = (uint8_t *)malloc((size_t)exact_plane_bytes(win, c.hs, c.vs, c.draft));
    const size_t out_bytes = (size_t)3 * r[2] * r[3];
    uint8_t *out = (uint8_t *)malloc(out_bytes);
    memset(out, kSent, out_bytes);
    JbLaunch p = base;
    p.rgb = out, p.rgb_row_stride = 3LL * r[2];
    if (k > 0) p.roi = 1, p.roi_x = r[0], p.roi_y = r[1], p.roi_w = r[2], p.roi_h = r[3];
    p.tiles_per_image = jbk_lj_tiles(r[2], r[3]), p.n_tiles = p.tiles_per_image;
    if (jbk_lj_launch(p, c.hs, c.vs, c.draft, planes, nullptr) != hipSuccess) fail(c, "jbk_lj_launch refuses", r);
    for (int y = 0; y < r[3]; y++)
      if (memcmp(out + (size_t)y * 3 * r[2], &c.image[((size_t)(r[1] + y) * ow + r[0]) * 3], (size_t)3 * r[2]) != 0) fail(c, "pixels differ", r);
    free(planes), free(out);
    n_cases++;
  }
  // 2. all of them in one jbk_lj_launch_crops: an "image" per rectangle, every one the same coefficients
  if (c.n_rects > 1 && c.n_rects <= kJbCropsPerLaunch) {
    JbCropTable table;
    memset(&table, 0, sizeof table);
    int64_t at = 0, plane_bytes = 0;
    int32_t most = 0;
    for (int k = 0; k < c.n_rects; k++) {
      const int32_t *r = &c.rects[(size_t)k * 4];
      JbCrop &cr = table.c[k];
      cr.x = r[0], cr.y = r[1], cr.w = r[2], cr.h = r[3], cr.tmp_offset = at;
      at += 3LL * r[2] * r[3];
      const JbLjWindow win = jbk_lj_window(c.hs, c.vs, c.draft, c.mcus_x, c.mcus_y, r[0], r[1], r[2], r[3]);
      plane_bytes = k + 1 < c.n_rects ? plane_bytes + win.bytes : plane_bytes + exact_plane_bytes(win, c.hs, c.vs, c.draft);
      if (jbk_lj_tiles(r[2], r[3]) > most) most = jbk_lj_tiles(r[2], r[3]);
    }
    uint8_t *planes = (uint8_t *)malloc((size_t)plane_bytes), *out = (uint8_t *)malloc((size_t)at);
    memset(out, kSent, (size_t)at);
    JbLaunch p = base;
    p.rgb = out, p.roi = 2, p.tiles_per_image = most, p.n_tiles = c.n_rects * most;
    if (jbk_lj_launch_crops(p, table, c.hs, c.vs, c.draft, planes, nullptr) != hipSuccess) fail(c, "jbk_lj_launch_crops refuses", c.rects.data());
    for (int k = 0; k < c.n_rects; k++) {
      const int32_t *r = &c.rects[(size_t)k * 4];
      for (int y = 0; y < r[3]; y++)
        if (memcmp(out + table.c[k].tmp_offset + (size_t)y * 3 * r[2], &c.image[((size_t)(r[1] + y) * ow + r[0]) * 3], (size_t)3 * r[2]) != 0)
          fail(c, "pixels of the crops launch differ", r);
    }
    free(planes), free(out);
    n_cases++;
  }
  free(coef), free(q);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    printf("usage: %s cases.bin (written by lj_kernel_cases.py)\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  for (;;) {
    Case c;
    int32_t head[8];
    if (!read_exact(f, head, sizeof head)) break;
    c.w = head[0], c.h = head[1], c.hs = head[2], c.vs = head[3], c.draft = head[4], c.mcus_x = head[5], c.mcus_y = head[6], c.n_rects = head[7];
    const int ow = (c.w + c.draft - 1) / c.draft, oh = (c.h + c.draft - 1) / c.draft;
    c.rects.resize((size_t)c.n_rects * 4), c.q.resize(192), c.coef.resize((size_t)c.mcus_x * c.mcus_y * (c.hs * c.vs + 2) * 64);
    c.image.resize((size_t)ow * oh * 3);
    if (!read_exact(f, c.rects.data(), c.rects.size() * 4) || !read_exact(f, c.q.data(), 192 * 4) || !read_exact(f, c.coef.data(), c.coef.size() * 2) ||
        !read_exact(f, c.image.data(), c.image.size())) {
      printf("FAIL: %s is truncated\n", argv[1]);
      return 1;
    }
    run(c);
  }
  fclose(f);
  if (n_cases == 0) {
    printf("FAIL: no cases in %s\n", argv[1]);
    return 1;
  }
  printf("%ld libjpeg-arithmetic kernel launches ok\n", n_cases);
  return 0;
}
