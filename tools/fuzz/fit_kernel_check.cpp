// fit_kernel_check -- the body of jb_fit_fill_kernel (csrc/jb_fit.hip) compiled for the CPU: a launch is a loop over the
// block and thread indices (the kernel has no barrier and no LDS).  Built with AddressSanitizer + UBSan; the destination
// is a heap block of exactly the bytes the strides promise, sentinel-filled, with odd strides, so a store outside it is a
// report and a store outside the border is a mismatch.  Expected: every border element holds the converted fill, every
// other byte -- the inner rectangle, the gaps between rows, planes and images -- the sentinel.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define JB_KERNELS_HOST
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
struct HostIdx {
  unsigned x;
};
static HostIdx threadIdx, blockIdx;
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
#include "../../jpeg_decoder_amd/csrc/jb_fit.hip"

static const uint8_t kSent = 0xA5;
static long n_cases = 0;
static const float kScale[3] = {1.0f / (255.0f * 0.229f), 1.0f / 255.0f, 1.0f + 1.0f / 2048.0f}, kBias[3] = {-0.485f / 0.229f, 0.0f, 0.25f};
static const uint8_t kFill[3] = {124, 116, 104};

template <int FORMAT>
static void launch(const JbFitFill &p, int64_t n_wgs) {
  for (int64_t b = 0; b < n_wgs; b++)
    for (unsigned t = 0; t < (unsigned)kFitFillLanes; t++) {
      blockIdx.x = (unsigned)b, threadIdx.x = t;
      jb_fit_fill_kernel<FORMAT>(p);
    }
}

// one case: n images of ow x oh whose inner rectangle is iw x ih at (ix, iy); the pads are in elements
static void one(int fmt, int n, int ow, int oh, int ix, int iy, int iw, int ih, int pad_row, int pad_plane, int pad_img) {
  const int es = fmt == 2 ? 4 : fmt == 3 ? 2 : 1;
  const int64_t row = fmt == 0 ? 3LL * ow + pad_row : ((int64_t)ow + pad_row) * es;
  const int64_t plane = fmt == 0 ? 0 : row * oh + (int64_t)pad_plane * es;
  const int64_t img = fmt == 0 ? row * oh + pad_img : 3 * plane + (int64_t)pad_img * es;
  const size_t bytes = (size_t)((n - 1) * img + (fmt == 0 ? (oh - 1) * row + 3LL * ow : 2 * plane + (oh - 1) * row + (int64_t)ow * es));
  uint8_t *dst = (uint8_t *)malloc(bytes), *want = (uint8_t *)malloc(bytes);
  memset(dst, kSent, bytes);
  memset(want, kSent, bytes);

  JbFitFill p;
  memset(&p, 0, sizeof p);
  p.dst = dst;
  p.dst_image_stride = n > 1 ? img : 0, p.dst_row_stride = row, p.dst_plane_stride = plane;
  p.ow = ow, p.oh = oh, p.n_images = n;
  if (iw < ow) {  // left and right
    p.bx[0] = 0, p.bw[0] = ix, p.bx[1] = ix + iw, p.bw[1] = ow - ix - iw;
    p.by[0] = p.by[1] = 0, p.bh[0] = p.bh[1] = oh;
  } else {  // top and bottom (none when ih == oh)
    p.by[0] = 0, p.bh[0] = iy, p.by[1] = iy + ih, p.bh[1] = oh - iy - ih;
    p.bx[0] = p.bx[1] = 0, p.bw[0] = p.bw[1] = ow;
  }
  for (int c = 0; c < 3; c++) p.scale[c] = kScale[c], p.bias[c] = kBias[c], p.fill[c] = kFill[c];
  int64_t n_wgs = -1;
  if (!fit_fill_grid(p, fmt, &n_wgs)) {
    printf("FAIL: fit_fill_grid refuses format %d target %dx%d inner %dx%d at (%d, %d)\n", fmt, ow, oh, iw, ih, ix, iy);
    exit(1);
  }
  const int64_t border = (int64_t)ow * oh - (int64_t)iw * ih;
  if ((border == 0) != (n_wgs == 0)) {
    printf("FAIL: %lld workgroups for a border of %lld elements\n", (long long)n_wgs, (long long)border);
    exit(1);
  }
  switch (fmt) {
    case 0: launch<0>(p, n_wgs); break;
    case 1: launch<1>(p, n_wgs); break;
    case 2: launch<2>(p, n_wgs); break;
    default: launch<3>(p, n_wgs); break;
  }

  for (int i = 0; i < n; i++)
    for (int y = 0; y < oh; y++)
      for (int x = 0; x < ow; x++) {
        if (x >= ix && x < ix + iw && y >= iy && y < iy + ih) continue;  // the inner rectangle: not the fill kernel's
        for (int c = 0; c < 3; c++) {
          uint8_t *at = want + i * img + y * row + (fmt == 0 ? 3 * x + c : c * plane + (int64_t)x * es);
          volatile float prod = (float)kFill[c] * kScale[c];
          const float f = prod + kBias[c];
          if (es == 1) *at = kFill[c];
          else if (es == 4) memcpy(at, &f, 4);
          else {
            const _Float16 hf = (_Float16)f;
            memcpy(at, &hf, 2);
          }
        }
      }
  if (memcmp(dst, want, bytes) != 0) {
    size_t at = 0;
    while (dst[at] == want[at]) at++;
    printf("FAIL: format %d, %d images of %dx%d, inner %dx%d at (%d, %d): byte %zu of %zu is %d, want %d\n", fmt, n, ow, oh, iw, ih, ix, iy, at,
           bytes, dst[at], want[at]);
    exit(1);
  }
  free(dst), free(want);
  n_cases++;
}

int main() {
  // {ow, oh, ix, iy, iw, ih}: top and bottom, left and right, bands one element wide, a band on one side only (the anchors
  // START and END), a band of more than one workgroup whose last one is ragged, and no border at all
  const int shapes[][6] = {{16, 16, 0, 3, 16, 10}, {16, 16, 3, 0, 10, 16}, {15, 16, 0, 1, 15, 14}, {16, 13, 1, 0, 14, 13}, {16, 16, 0, 0, 16, 10},
                           {16, 16, 6, 0, 10, 16}, {70, 23, 0, 9, 70, 1}, {9, 300, 4, 0, 1, 300}, {224, 224, 0, 49, 224, 126}, {16, 16, 0, 0, 16, 16},
                           {1, 1, 0, 0, 1, 1}, {3, 1, 1, 0, 1, 1}};
  for (int fmt = 0; fmt < 4; fmt++)
    for (const auto &s : shapes) {
      one(fmt, 1, s[0], s[1], s[2], s[3], s[4], s[5], 0, 0, 0);
      one(fmt, 3, s[0], s[1], s[2], s[3], s[4], s[5], 1, 5, 7);
    }
  // an argument outside its range is refused before anything runs
  JbFitFill bad;
  memset(&bad, 0, sizeof bad);
  bad.ow = 16, bad.oh = 16, bad.n_images = 1, bad.bw[0] = 16, bad.bh[0] = 4, bad.by[0] = 13;
  int64_t n_wgs = 0;
  if (fit_fill_grid(bad, 0, &n_wgs)) {
    printf("FAIL: a band that leaves the output is not refused\n");
    return 1;
  }
  bad.by[0] = 12;
  if (!fit_fill_grid(bad, 0, &n_wgs) || fit_fill_grid(bad, 4, &n_wgs)) {
    printf("FAIL: fit_fill_grid's range checks\n");
    return 1;
  }
  bad.ow = bad.oh = bad.bw[0] = bad.bh[0] = 65535, bad.by[0] = 0, bad.n_images = 1 << 8;
  if (fit_fill_grid(bad, 0, &n_wgs)) {  // 256 x 16.8 M workgroups: more than 2^31 - 1
    printf("FAIL: more than 2^31 - 1 workgroups are not refused\n");
    return 1;
  }
  printf("%ld fit fill kernel cases ok\n", n_cases);
  return 0;
}
