// orient_kernel_check -- the body of jb_orient_kernel (csrc/jb_orient.hip) compiled for the CPU: the HIP built-ins it
// uses are stubbed below, a launch is a loop over the block index with, per block, every lane's load half and then every
// lane's store half (the barrier between them).  Built with AddressSanitizer + UBSan; source, destination and LDS are
// heap blocks of exactly the promised size, so any access outside them is a report.  Every orientation, all four
// formats, sizes around the tile, tight and padded strides, and the table variant, against T_o written out per value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define JB_ORIENT_HOST
#define __device__
#define __forceinline__ inline
struct HostRsrc {
  const uint8_t *base;
  int range;
};
typedef HostRsrc __amdgpu_buffer_rsrc_t;
static inline HostRsrc host_make_rsrc(uint8_t *p, int, int range, int) { return HostRsrc{p, range}; }
// a raw buffer load: 0 beyond the descriptor's range, else the bytes -- read for real, so that a range that promises
// more than the allocation holds is a sanitizer report
static inline uint32_t host_load_b32(HostRsrc r, int off, int, int) {
  if (off < 0 || off + 4 > r.range) return 0;
  uint32_t v;
  memcpy(&v, r.base + off, 4);
  return v;
}
// binary16 where the host compiler has no _Float16: float -> half, round to nearest even (the device's one convert)
struct HostHalf {
  uint16_t bits;
  explicit HostHalf(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) bits = (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0));  // inf, nan
    else if (mag >= 0x477ff000u) bits = (uint16_t)(sign | 0x7c00u);                                // rounds to inf
    else if (mag < 0x33000001u) bits = (uint16_t)sign;                                             // rounds to zero
    else {
      const int e = (int)(mag >> 23) - 127;
      // the 24-bit significand shifted so that its kept part is the half's (subnormal below 2^-14)
      const uint32_t sig = (mag & 0x7fffffu) | 0x800000u;
      const int shift = e >= -14 ? 13 : 13 + (-14 - e);
      const uint32_t kept = sig >> shift, rest = sig & ((1u << shift) - 1), half = 1u << (shift - 1);
      uint32_t h = e >= -14 ? ((uint32_t)(e + 15) << 10) + (kept - 0x400u) : kept;
      if (rest > half || (rest == half && (h & 1))) h++;  // (a carry walks into the exponent: still the right value)
      bits = (uint16_t)(sign | h);
    }
  }
};
#define _Float16 HostHalf
#define __builtin_amdgcn_make_buffer_rsrc host_make_rsrc
#define __builtin_amdgcn_raw_buffer_load_b32 host_load_b32
#include "../../jpeg_decoder_amd/csrc/jb_orient.hip"

static const uint8_t kSent = 0xA5;
static long n_cases = 0;

// T_o as include/jpegblk.h states it: the source pixel of output pixel (y, x)
static void source_of(int o, int w, int h, int y, int x, int *sy, int *sx) {
  switch (o) {
    case 1: *sy = y, *sx = x; break;
    case 2: *sy = y, *sx = w - 1 - x; break;
    case 3: *sy = h - 1 - y, *sx = w - 1 - x; break;
    case 4: *sy = h - 1 - y, *sx = x; break;
    case 5: *sy = x, *sx = y; break;
    case 6: *sy = h - 1 - x, *sx = y; break;
    case 7: *sy = h - 1 - x, *sx = w - 1 - y; break;
    default: *sy = x, *sx = w - 1 - y; break;
  }
}

template <int FORMAT, bool TABLE, typename... T>
static void launch(const JbOrient &p, long n_blocks, const T &...table) {
  for (long block = 0; block < n_blocks; block++) {
    OrientTile t;
    if (!orient_tile<TABLE>(p, (uint32_t)block, t, table...)) continue;
    std::vector<uint32_t> lds((size_t)kJbOrientTile * kOrientPitch, 0xDEADBEEFu);
    for (int th = 0; th < 256; th++) orient_load(t, th >> 6, th & 63, lds.data());
    for (int th = 0; th < 256; th++) orient_store<FORMAT>(p, t, th >> 6, th & 63, lds.data());
  }
}

static void fail(const char *what, int o, int fmt, int w, int h) {
  printf("FAIL %s: orientation %d format %d size %dx%d\n", what, o, fmt, w, h);
  exit(1);
}

static void one(int o, int fmt, int w, int h, int n, int pad_row, int pad_plane, int pad_img) {
  const int es = fmt == 2 ? 4 : fmt == 3 ? 2 : 1;
  const int ow = o >= 5 ? h : w, oh = o >= 5 ? w : h;
  const size_t src_img = (size_t)3 * w * h;
  uint8_t *src = (uint8_t *)malloc(src_img * n + 4);
  for (size_t i = 0; i < src_img * n + 4; i++) src[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + 1);
  const int64_t row = fmt == 0 ? 3LL * ow + pad_row : ((int64_t)ow + pad_row) * es;
  const int64_t plane = fmt == 0 ? 0 : row * oh + (int64_t)pad_plane * es;
  const int64_t img = fmt == 0 ? row * oh + pad_img : 3 * plane + (int64_t)pad_img * es;
  // exactly up to the last element of the last image
  const size_t dst_bytes = (size_t)((n - 1) * img + (fmt == 0 ? (oh - 1) * row + 3LL * ow : 2 * plane + (oh - 1) * row + (int64_t)ow * es));
  uint8_t *dst = (uint8_t *)malloc(dst_bytes), *want = (uint8_t *)malloc(dst_bytes);
  memset(dst, kSent, dst_bytes);
  memset(want, kSent, dst_bytes);
  JbOrient p;
  memset(&p, 0, sizeof p);
  p.src = src, p.dst = dst;
  p.src_image_stride = (int64_t)src_img;
  p.dst_image_stride = img, p.dst_row_stride = row, p.dst_plane_stride = plane;
  p.sw = w, p.sh = h, p.orientation = o, p.n_images = n;
  p.tiles_x = (w + kJbOrientTile - 1) / kJbOrientTile;
  p.tiles_per_image = p.tiles_x * ((h + kJbOrientTile - 1) / kJbOrientTile);
  const float scale[3] = {1.0f / (255.0f * 0.229f), 1.0f / 255.0f, 1.0f + 1.0f / 2048.0f}, bias[3] = {-0.485f / 0.229f, 0.0f, 0.25f};
  for (int c = 0; c < 3; c++) p.scale[c] = scale[c], p.bias[c] = bias[c];
  const long blocks = (long)p.tiles_per_image * n;
  if (fmt == 0) launch<0, false>(p, blocks);
  else if (fmt == 1) launch<1, false>(p, blocks);
  else if (fmt == 2) launch<2, false>(p, blocks);
  else launch<3, false>(p, blocks);
  for (int i = 0; i < n; i++)
    for (int y = 0; y < oh; y++)
      for (int x = 0; x < ow; x++) {
        int sy, sx;
        source_of(o, w, h, y, x, &sy, &sx);
        for (int c = 0; c < 3; c++) {
          const uint8_t u = src[i * src_img + ((size_t)sy * w + sx) * 3 + c];
          uint8_t *at = want + i * img + y * row + (fmt == 0 ? 3 * x + c : c * plane + (int64_t)x * es);
          volatile float prod = (float)u * scale[c];  // (one multiply, one add: no contraction)
          const float f = prod + bias[c];
          if (es == 1) *at = u;
          else if (es == 4) memcpy(at, &f, 4);
          else {
            const _Float16 hf = (_Float16)f;
            memcpy(at, &hf, 2);
          }
        }
      }
  if (memcmp(dst, want, dst_bytes) != 0) fail("launch", o, fmt, w, h);
  free(src), free(dst), free(want);
  n_cases++;
}

// the table variant: images of different sizes back to back, tight on both sides
static void table_case(int o, const int (*sizes)[2], int n) {
  JbOrientTable table;
  memset(&table, 0, sizeof table);
  int64_t at = 0;
  int most = 0;
  for (int i = 0; i < n; i++) {
    table.r[i] = JbOrientRow{sizes[i][0], sizes[i][1], at, at};
    at += 3LL * sizes[i][0] * sizes[i][1];
    const int tiles = ((sizes[i][0] + kJbOrientTile - 1) / kJbOrientTile) * ((sizes[i][1] + kJbOrientTile - 1) / kJbOrientTile);
    if (tiles > most) most = tiles;
  }
  uint8_t *src = (uint8_t *)malloc((size_t)at + 4), *dst = (uint8_t *)malloc((size_t)at), *want = (uint8_t *)malloc((size_t)at);
  for (int64_t i = 0; i < at + 4; i++) src[i] = (uint8_t)(i * 37 + (i >> 7) + 3);
  memset(dst, kSent, (size_t)at);
  JbOrient p;
  memset(&p, 0, sizeof p);
  p.src = src, p.dst = dst, p.orientation = o, p.n_images = n, p.tiles_per_image = most;
  launch<0, true>(p, (long)most * n, table);
  for (int i = 0; i < n; i++) {
    const int w = sizes[i][0], h = sizes[i][1], ow = o >= 5 ? h : w, oh = o >= 5 ? w : h;
    for (int y = 0; y < oh; y++)
      for (int x = 0; x < ow; x++) {
        int sy, sx;
        source_of(o, w, h, y, x, &sy, &sx);
        memcpy(want + table.r[i].dst_offset + ((size_t)y * ow + x) * 3, src + table.r[i].src_offset + ((size_t)sy * w + sx) * 3, 3);
      }
  }
  if (memcmp(dst, want, (size_t)at) != 0) fail("table", o, 0, sizes[0][0], sizes[0][1]);
  free(src), free(dst), free(want);
  n_cases++;
}

int main() {
  const int T = kJbOrientTile;
  const int sizes[][3] = {{1, 1, 1},     {1, T + 3, 1},     {T + 3, 1, 1}, {T - 1, T + 1, 1}, {2 * T + 5, T + 9, 3},
                          {T, T, 2},     {2 * T, T, 1},     {T + 1, 2 * T + 1, 1}, {3, 200, 1}};
  for (int o = 1; o <= 8; o++)
    for (int fmt = 0; fmt < 4; fmt++)
      for (const auto &s : sizes) {
        one(o, fmt, s[0], s[1], s[2], 0, 0, 0);
        one(o, fmt, s[0], s[1], s[2], 1, 5, 7);
      }
  const int mixed[][2] = {{T + 9, 2 * T + 5}, {1, 1}, {T, T}, {5, T + 1}, {2 * T + 1, 3}};
  for (int o = 1; o <= 8; o++) table_case(o, mixed, 5);
  printf("%ld orient kernel cases ok\n", n_cases);
  return 0;
}
