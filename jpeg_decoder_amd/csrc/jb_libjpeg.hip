// jb_libjpeg.hip -- the pixel kernels of JB_ARITH_LIBJPEG ("decoder arithmetic", include/jpegblk.h): dequantise,
// jidctint.c's "islow" inverse DCT, jdsample.c's "fancy" chroma upsampling and jdcolor.c's 16.16 fixed-point colour
// conversion, all in int32, so that the full-size decode has the bits libjpeg(-turbo) -- Pillow, torchvision, OpenCV
// -- gives for the same file.  The reference-arithmetic kernels (jb_kernels.hip) know nothing of this file.
//
// Two kernels per launch, in stream order, for every layout:
//   jb_lj_block_kernel   one lane = one coded 8x8 block of the launch's MCU WINDOW: 128 coefficient bytes -> registers,
//                        dequantise, columns pass, rows pass (v_mul_i32_i24: inside the contract's domain every
//                        multiplicand fits 24 bits), clamp(out + 128), and the block's 64 uint8 samples go into the
//                        image's Y, Cb or Cr PLANE in a scratch of the context (eight 8-byte stores).
//   jb_lj_pixel_kernel   one lane = 4 horizontally adjacent pixels of the OUTPUT rectangle: the luma samples, the chroma
//                        samples with their neighbours (every index clamped to the frame's chroma plane, which is the
//                        whole of libjpeg's edge handling), the triangle filter, the colour conversion, and the store
//                        in the launch's format.  No LDS, no barrier; a workgroup is 256 pixels x 4 rows of one image.
// The window is the MCUs the rectangle touches, grown by one MCU on every side where chroma is subsampled and clamped to
// the frame: the upsampler's neighbours are the true neighbouring samples also where they lie in MCUs the rectangle
// does not touch.  The planes cost traffic the fused reference kernel does not have (every sample is written and read
// once more: 2 bytes per pixel in 4:2:0, 3 in 4:4:4 ... on top of 6 and 9) -- see DESIGN.md section 5.13.
//
// Outside the contract's domain (an intermediate beyond int32, a pass input beyond int16) the arithmetic wraps: the
// output is deterministic and every access stays in bounds, and its bits are pinned to nothing.
//
// "Draft decode" (include/jpegblk.h): at draft K = 2, 4, 8 the block kernel runs jidctred.c's reduced IDCTs -- a luma block
// gives S = 8 / K samples per axis, a chroma block Sc (jdmaster.c) -- into planes of S- and Sc-sized blocks, and the pixel
// kernel reads them as planes of the DRAFT FRAME (p.width x p.height) whose upsampler is (eh, ev, fancy) in the place of
// (hs, vs, fancy).  The true hs, vs and p.mcus_x still address the coefficients.  Draft 1: S = Sc = 8, eh = hs, ev = vs.

// The kernels and their launchers also compile for the CPU (JB_KERNELS_HOST: tools/fuzz/lj_kernel_check.cpp stubs the
// built-ins and runs a launch as a loop over block and thread index).
#ifndef JB_KERNELS_HOST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "jb_kernels.h"

namespace {

typedef uint32_t u32_u __attribute__((aligned(1)));  // four bytes at any byte address
typedef uint32_t u32_h __attribute__((aligned(2)));
#ifndef JB_KERNELS_HOST
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
#endif

// what one image of a launch is: the rectangle, the window its planes hold, and where planes and output lie
struct LjView {
  int32_t x, y, w, h;          // the rectangle, in pixels of the frame (the draft frame)
  int32_t wmx, wmy, wnx, wny;  // the window: its first MCU, MCUs per row and per column
  int64_t plane_offset;        // bytes from the scratch's base to this image's Y plane (Cb, Cr follow)
  int64_t out_offset;          // bytes from p.rgb to this image's output
  int64_t out_row_stride;      // bytes between its rows (of a plane when planar)
};
struct LjTable {
  LjView v[kJbCropsPerLaunch];
};
struct LjArgs {
  uint8_t *planes;
  int64_t plane_image_stride;  // launch-wide view only: bytes between the images' planes
  int32_t hs, vs;
  int32_t block_wgs;           // workgroups per image of jb_lj_block_kernel
  int32_t sy, sc;              // "draft decode": samples per axis of a luma and of a chroma block (8: none)
  int32_t eh, ev, fancy;       // what the upsampler does: hs * sy / sc, vs * sy / sc; 0: plain replication (draft 8)
  LjView one;                  // the view of every image of a launch without a table (offsets of image 0)
};

__device__ __forceinline__ int shl13(int a) { return (int)((uint32_t)a << 13); }
__device__ __forceinline__ int clamp255(int a) { return min(max(a, 0), 255); }

// jidctint.c's 1-D network (CONST_BITS 13), outputs descaled by N with rounding
template <int N>
__device__ __forceinline__ void islow_1d(int in0, int in1, int in2, int in3, int in4, int in5, int in6, int in7, int &o0, int &o1,
                                         int &o2, int &o3, int &o4, int &o5, int &o6, int &o7) {
  // even part
  int z1 = __mul24(in2 + in6, 4433);
  const int tmp2 = z1 - __mul24(in6, 15137);
  const int tmp3 = z1 + __mul24(in2, 6270);
  const int tmp0 = shl13(in0 + in4);
  const int tmp1 = shl13(in0 - in4);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  int t0 = in7, t1 = in5, t2 = in3, t3 = in1;
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = __mul24(z3 + z4, 9633);
  t0 = __mul24(t0, 2446), t1 = __mul24(t1, 16819), t2 = __mul24(t2, 25172), t3 = __mul24(t3, 12299);
  z1 = __mul24(z1, -7373), z2 = __mul24(z2, -20995);
  z3 = __mul24(z3, -16069) + z5, z4 = __mul24(z4, -3196) + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  constexpr int R = 1 << (N - 1);
  o0 = (tmp10 + t3 + R) >> N, o7 = (tmp10 - t3 + R) >> N;
  o1 = (tmp11 + t2 + R) >> N, o6 = (tmp11 - t2 + R) >> N;
  o2 = (tmp12 + t1 + R) >> N, o5 = (tmp12 - t1 + R) >> N;
  o3 = (tmp13 + t0 + R) >> N, o4 = (tmp13 - t0 + R) >> N;
}

// the view of image `img`: its row of the table, or the launch's with the image's strides added
__device__ __forceinline__ LjView view_of(const JbLaunch &p, const LjArgs &a, int img) {
  LjView v = a.one;
  v.plane_offset += (int64_t)img * a.plane_image_stride;
  v.out_offset += (int64_t)img * p.rgb_image_stride;
  return v;
}

// jidctred.c's 4-point network (index 4 is never read), outputs descaled by N with rounding
template <int N>
__device__ __forceinline__ void red4_1d(int in0, int in1, int in2, int in3, int in5, int in6, int in7, int &o0, int &o1, int &o2, int &o3) {
  const int t0 = (int)((uint32_t)in0 << 14);
  const int t2 = __mul24(in2, 15137) + __mul24(in6, -6270);
  const int t10 = t0 + t2, t12 = t0 - t2;
  const int a = __mul24(in7, -1730) + __mul24(in5, 11893) + __mul24(in3, -17799) + __mul24(in1, 8697);
  const int b = __mul24(in7, -4176) + __mul24(in5, -4926) + __mul24(in3, 7373) + __mul24(in1, 20995);
  constexpr int R = 1 << (N - 1);
  o0 = (t10 + b + R) >> N, o1 = (t12 + a + R) >> N, o2 = (t12 - a + R) >> N, o3 = (t10 - b + R) >> N;
}
// ... and its 2-point network on in0, in1, in3, in5, in7
template <int N>
__device__ __forceinline__ void red2_1d(int in0, int in1, int in3, int in5, int in7, int &o0, int &o1) {
  const int t10 = (int)((uint32_t)in0 << 15);
  const int t = __mul24(in7, -5906) + __mul24(in5, 6967) + __mul24(in3, -10426) + __mul24(in1, 29692);
  constexpr int R = 1 << (N - 1);
  o0 = (t10 + t + R) >> N, o1 = (t10 - t + R) >> N;
}

// row k of a coded block (16 bytes), dequantised
__device__ __forceinline__ void lj_load_row(const u32x4_t *src, const int32_t *q, int k, int *c) {
  const u32x4_t t = src[k];
  const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int coef = (i & 1) ? ((int)w[i >> 1] >> 16) : (int)(short)(w[i >> 1] & 0xffffu);
    c[i] = __mul24(coef, q[k * 8 + i]);
  }
}

// one coded block -> its N x N samples at dst (N bytes per row: N-byte stores, dst and pitch are multiples of N)
template <int N>
__device__ __forceinline__ void lj_idct_store(const u32x4_t *src, const int32_t *q, uint8_t *dst, int pitch);

template <>
__device__ __forceinline__ void lj_idct_store<8>(const u32x4_t *src, const int32_t *q, uint8_t *dst, int pitch) {
  int c[64];
#pragma unroll
  for (int k = 0; k < 8; k++) lj_load_row(src, q, k, c + k * 8);
#pragma unroll
  for (int i = 0; i < 8; i++)  // columns pass (PASS1_BITS 2: descale by 13 - 2)
    islow_1d<11>(c[0 * 8 + i], c[1 * 8 + i], c[2 * 8 + i], c[3 * 8 + i], c[4 * 8 + i], c[5 * 8 + i], c[6 * 8 + i], c[7 * 8 + i],
                 c[0 * 8 + i], c[1 * 8 + i], c[2 * 8 + i], c[3 * 8 + i], c[4 * 8 + i], c[5 * 8 + i], c[6 * 8 + i], c[7 * 8 + i]);
#pragma unroll
  for (int k = 0; k < 8; k++) {  // rows pass (descale by 13 + 2 + 3), level shift, clamp
    int o[8];
    islow_1d<18>(c[k * 8 + 0], c[k * 8 + 1], c[k * 8 + 2], c[k * 8 + 3], c[k * 8 + 4], c[k * 8 + 5], c[k * 8 + 6], c[k * 8 + 7], o[0],
                 o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) lo |= (uint32_t)clamp255(o[i] + 128) << (8 * i), hi |= (uint32_t)clamp255(o[4 + i] + 128) << (8 * i);
    *(uint2 *)(dst + (int64_t)k * pitch) = make_uint2(lo, hi);
  }
}

template <>
__device__ __forceinline__ void lj_idct_store<4>(const u32x4_t *src, const int32_t *q, uint8_t *dst, int pitch) {
  int c[7][8];  // rows 0-3 and 5-7: row 4 is never read
#pragma unroll
  for (int k = 0; k < 7; k++) lj_load_row(src, q, k < 4 ? k : k + 1, c[k]);
  int ws[4][8];  // (column 4 stays unset and unread)
#pragma unroll
  for (int i = 0; i < 8; i++)  // columns pass (descale by 14 - 2)
    if (i != 4) red4_1d<12>(c[0][i], c[1][i], c[2][i], c[3][i], c[4][i], c[5][i], c[6][i], ws[0][i], ws[1][i], ws[2][i], ws[3][i]);
#pragma unroll
  for (int k = 0; k < 4; k++) {  // rows pass (descale by 14 + 2 + 3), level shift, clamp
    int o[4];
    red4_1d<19>(ws[k][0], ws[k][1], ws[k][2], ws[k][3], ws[k][5], ws[k][6], ws[k][7], o[0], o[1], o[2], o[3]);
    uint32_t px = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) px |= (uint32_t)clamp255(o[i] + 128) << (8 * i);
    *(uint32_t *)(dst + (int64_t)k * pitch) = px;
  }
}

template <>
__device__ __forceinline__ void lj_idct_store<2>(const u32x4_t *src, const int32_t *q, uint8_t *dst, int pitch) {
  int c[5][8];  // rows 0, 1, 3, 5, 7
#pragma unroll
  for (int k = 0; k < 5; k++) lj_load_row(src, q, k < 2 ? k : 2 * k - 1, c[k]);
  int ws[2][5];  // columns 0, 1, 3, 5, 7
#pragma unroll
  for (int j = 0; j < 5; j++) {  // columns pass (descale by 15 - 2)
    const int i = j < 2 ? j : 2 * j - 1;
    red2_1d<13>(c[0][i], c[1][i], c[2][i], c[3][i], c[4][i], ws[0][j], ws[1][j]);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {  // rows pass (descale by 15 + 2 + 3), level shift, clamp
    int o0, o1;
    red2_1d<20>(ws[k][0], ws[k][1], ws[k][2], ws[k][3], ws[k][4], o0, o1);
    *(uint16_t *)(dst + (int64_t)k * pitch) = (uint16_t)(clamp255(o0 + 128) | clamp255(o1 + 128) << 8);
  }
}

template <>
__device__ __forceinline__ void lj_idct_store<1>(const u32x4_t *src, const int32_t *q, uint8_t *dst, int) {
  const int dc = __mul24((int)(short)(src[0].x & 0xffffu), q[0]);
  *dst = (uint8_t)clamp255(((dc + 4) >> 3) + 128);
}

// ---- kernel 1: coded blocks -> uint8 planes ----
// SY, SC: samples per axis of a luma and of a chroma block ("draft decode"; 8, 8: the full-size decode)
template <int SY, int SC>
__device__ __forceinline__ void lj_block_body(const JbLaunch &p, const LjArgs &a, const LjView &v, int img, int idx) {
  const int hs = a.hs, vs = a.vs, ny = hs * vs, nb = ny + 2;
  const int n_mcus = v.wnx * v.wny;
  if (idx >= n_mcus * nb) return;
  // component-major: consecutive lanes are the same block of consecutive MCUs of a window row
  const int s = idx / n_mcus, r = idx - s * n_mcus;
  const int wy = r / v.wnx, wx = r - wy * v.wnx;
  const int comp = s < ny ? 0 : s - ny + 1;
  const int64_t mcu = (int64_t)(v.wmy + wy) * p.mcus_x + (v.wmx + wx);
  const u32x4_t *src = (const u32x4_t *)((const uint8_t *)p.coef + (int64_t)img * p.coef_image_stride + (mcu * nb + s) * 128);
  const int32_t *q = (const int32_t *)((const uint8_t *)p.qtabs + (int64_t)img * p.qtab_image_stride) + comp * 64;
  // where the block lands: luma block (bv, bh) of the MCU in the Y plane, a chroma block in its own plane
  const int ypitch = v.wnx * SY * hs, cpitch = v.wnx * SC;
  const int64_t ybytes = (int64_t)ypitch * (v.wny * SY * vs), cbytes = (int64_t)cpitch * (v.wny * SC);
  uint8_t *plane = a.planes + v.plane_offset;
  // (N-byte aligned stores: pitches, plane sizes and offsets are multiples of the block size that is stored there)
  if (comp == 0) {
    const int bv = s / hs, bh = s - bv * hs;
    lj_idct_store<SY>(src, q, plane + (int64_t)((wy * vs + bv) * SY) * ypitch + (wx * hs + bh) * SY, ypitch);
  } else {
    plane += ybytes + (comp - 1) * cbytes;
    lj_idct_store<SC>(src, q, plane + (int64_t)(wy * SC) * cpitch + wx * SC, cpitch);
  }
}

template <int SY, int SC>
__global__ __launch_bounds__(256) void jb_lj_block_kernel(const JbLaunch p, const LjArgs a) {
  const int img = blockIdx.x / a.block_wgs, wg = blockIdx.x - img * a.block_wgs;
  lj_block_body<SY, SC>(p, a, view_of(p, a, img), img, wg * 256 + threadIdx.x);
}
template <int SY, int SC>
__global__ __launch_bounds__(256) void jb_lj_block_kernel_crops(const JbLaunch p, const LjArgs a, const LjTable table) {
  const int img = blockIdx.x / a.block_wgs, wg = blockIdx.x - img * a.block_wgs;
  lj_block_body<SY, SC>(p, a, table.v[img], img, wg * 256 + threadIdx.x);
}

// ---- kernel 2: planes -> pixels ----
// the chroma of the lane's four pixels (frame columns x .. x + 3 of frame row y) from one chroma plane
__device__ __forceinline__ void lj_chroma4(const uint8_t *plane, int cpitch, int crows, int cx0, int cy0, int dw, int dh, int hs, int vs,
                                           bool plain, int x, int y, int (&out)[4]) {
  // the two source rows: the pixel's own and its vertical neighbour, clamped to the frame's plane (and, for memory
  // safety alone, to the window: inside the contract the window holds every sample that is asked for)
  const int cy = vs == 2 ? y >> 1 : y;
  const int nyr = min(max(cy + ((y & 1) ? 1 : -1), 0), dh - 1);
  const bool vfilter = vs == 2 && !plain;
  const uint8_t *r0 = plane + (int64_t)min(max(cy - cy0, 0), crows - 1) * cpitch;
  const uint8_t *r1 = plane + (int64_t)min(max(nyr - cy0, 0), crows - 1) * cpitch;
  // column c of the vertically filtered row: h2v2 keeps the sum 3a + b unscaled (jdsample.c's "thiscolsum")
  const auto col = [&](int c) {
    const int rel = min(max(min(max(c, 0), dw - 1) - cx0, 0), cpitch - 1);
    const int a = r0[rel];
    if (!vfilter) return a;
    const int s = 3 * a + r1[rel];
    return hs == 2 ? s : (s + ((y & 1) ? 2 : 1)) >> 2;
  };
  if (hs == 1) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = col(x + i);
    return;
  }
  // hs == 2: pixels x .. x + 3 and their horizontal neighbours lie in chroma columns c0 - 1 .. c0 + 2
  const int c0 = x >> 1, par = x & 1;
  int t[4];
#pragma unroll
  for (int k = 0; k < 4; k++) t[k] = col(c0 - 1 + k);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // pixel i: chroma column (i + par) >> 1 of the span, odd = (i + par) & 1; both parities with static indices
    const int e = i >> 1, o = (i + 1) >> 1;
    const int cur = par ? t[o + 1] : t[e + 1];
    const bool odd = ((i + par) & 1) != 0;
    const int nb = par ? (((i + 1) & 1) ? t[min(o + 2, 3)] : t[o]) : ((i & 1) ? t[e + 2] : t[e]);  // (o + 2 = 4 is never odd)
    if (plain) out[i] = cur;
    else if (vs == 2) out[i] = (3 * cur + nb + (odd ? 7 : 8)) >> 4;
    else out[i] = (3 * cur + nb + (odd ? 2 : 1)) >> 2;
  }
}

__device__ __forceinline__ void lj_pixel_body(const JbLaunch &p, const LjArgs &a, const LjView &v, int rem) {
  // (hs, vs: what the upsampler does -- the layout's factors, or what a draft's chroma IDCT has left of them)
  const int hs = a.eh, vs = a.ev;
  const int tiles_x = (v.w + 255) >> 8;
  const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int tid = threadIdx.x;
  const int ox = tx * 256 + (tid & 63) * 4, oy = ty * 4 + (tid >> 6);
  if (ox >= v.w || oy >= v.h) return;
  const int n = min(4, v.w - ox);
  const int x = v.x + ox, y = v.y + oy;
  const int mw = a.hs * a.sy, mh = a.vs * a.sy;  // an MCU in pixels of the frame
  const int ypitch = v.wnx * mw, yrows = v.wny * mh, cpitch = v.wnx * a.sc, crows = v.wny * a.sc;
  const uint8_t *yp = a.planes + v.plane_offset;
  const uint8_t *cbp = yp + (int64_t)ypitch * yrows, *crp = cbp + (int64_t)cpitch * crows;
  const uint8_t *yrow = yp + (int64_t)min(max(y - v.wmy * mh, 0), yrows - 1) * ypitch;
  const int xr = x - v.wmx * mw;
  int yy[4], cb[4], cr[4];
#pragma unroll
  for (int i = 0; i < 4; i++) yy[i] = yrow[min(max(xr + i, 0), ypitch - 1)];
  const int dw = (p.width + hs - 1) / hs, dh = (p.height + vs - 1) / vs;
  // libjpeg: no fancy upsampling for a chroma row of one or two samples, and none at all at draft 8
  const bool plain = (hs == 2 && dw <= 2) || !a.fancy;
  lj_chroma4(cbp, cpitch, crows, v.wmx * a.sc, v.wmy * a.sc, dw, dh, hs, vs, plain, x, y, cb);
  lj_chroma4(crp, cpitch, crows, v.wmx * a.sc, v.wmy * a.sc, dw, dh, hs, vs, plain, x, y, cr);
  uint32_t ch[3] = {0, 0, 0};  // ch[c]: the u8 samples of channel c, pixels 0..3
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int b = cb[i] - 128, r = cr[i] - 128;
    ch[0] |= (uint32_t)clamp255(yy[i] + ((__mul24(91881, r) + 32768) >> 16)) << (8 * i);
    ch[1] |= (uint32_t)clamp255(yy[i] + ((__mul24(-22554, b) + __mul24(-46802, r) + 32768) >> 16)) << (8 * i);
    ch[2] |= (uint32_t)clamp255(yy[i] + ((__mul24(116130, b) + 32768) >> 16)) << (8 * i);
  }
  uint8_t *row = p.rgb + v.out_offset + (int64_t)oy * v.out_row_stride;
  if (p.format == 0) {
    uint8_t *o = row + (int64_t)ox * 3;
    if (n == 4) {
      const uint32_t r = ch[0], g = ch[1], b = ch[2];
      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      const uint32_t w0 = (r & 0xffu) | (g & 0xffu) << 8 | (b & 0xffu) << 16 | (r & 0xff00u) << 16;
      const uint32_t w1 = ((g >> 8) & 0xffu) | ((b >> 8) & 0xffu) << 8 | ((r >> 16) & 0xffu) << 16 | ((g >> 16) & 0xffu) << 24;
      const uint32_t w2 = ((b >> 16) & 0xffu) | (r >> 24) << 8 | (g >> 24) << 16 | (b >> 24) << 24;
      ((u32_u *)o)[0] = w0, ((u32_u *)o)[1] = w1, ((u32_u *)o)[2] = w2;
    } else {
      for (int i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) o[i * 3 + c] = (uint8_t)(ch[c] >> (8 * i));
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint8_t *pl = row + (int64_t)c * p.rgb_plane_stride;
    if (p.format == 1) {
      uint8_t *o = pl + ox;
      if (n == 4) *(u32_u *)o = ch[c];
      else
        for (int i = 0; i < n; i++) o[i] = (uint8_t)(ch[c] >> (8 * i));
    } else {
      // value = (float)u8 * scale + bias: a multiply and an add, each rounded (this file is built with -ffp-contract=off)
      const float sc = p.scale[c], bi = p.bias[c];
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; i++) f[i] = (float)((ch[c] >> (8 * i)) & 0xffu) * sc + bi;
      if (p.format == 2) {
        float *o = (float *)pl + ox;
        for (int i = 0; i < n; i++) o[i] = f[i];
      } else {
        uint16_t hbits[4];
#pragma unroll
        for (int i = 0; i < 4; i++) hbits[i] = __builtin_bit_cast(uint16_t, (_Float16)f[i]);  // round to nearest even
        uint16_t *o = (uint16_t *)pl + ox;
        if (n == 4) ((u32_h *)o)[0] = hbits[0] | (uint32_t)hbits[1] << 16, ((u32_h *)o)[1] = hbits[2] | (uint32_t)hbits[3] << 16;
        else
          for (int i = 0; i < n; i++) o[i] = hbits[i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void jb_lj_pixel_kernel(const JbLaunch p, const LjArgs a) {
  const int img = blockIdx.x / p.tiles_per_image;
  lj_pixel_body(p, a, view_of(p, a, img), blockIdx.x - img * p.tiles_per_image);
}
__global__ __launch_bounds__(256) void jb_lj_pixel_kernel_crops(const JbLaunch p, const LjArgs a, const LjTable table) {
  const int img = blockIdx.x / p.tiles_per_image, rem = blockIdx.x - img * p.tiles_per_image;
  const LjView v = table.v[img];
  if (rem >= ((v.w + 255) >> 8) * ((v.h + 3) >> 2)) return;  // (the grid is sized for the launch's largest rectangle)
  lj_pixel_body(p, a, v, rem);
}

bool layout_ok(int hs, int vs) { return (hs == 1 || hs == 2) && (vs == 1 || vs == 2); }
bool draft_ok(int draft) { return draft == 1 || draft == 2 || draft == 4 || draft == 8; }

// "draft decode": the block sizes and the upsampler of a layout at a draft, into a (jb_draft_geometry_of's arithmetic)
void set_layout(LjArgs &a, int hs, int vs, int draft) {
  a.hs = hs, a.vs = vs;
  a.sy = a.sc = 8 / draft;
  while (a.sc < 8 && (hs * a.sy) % (2 * a.sc) == 0 && (vs * a.sy) % (2 * a.sc) == 0) a.sc *= 2;
  a.eh = hs * a.sy / a.sc, a.ev = vs * a.sy / a.sc;
  a.fancy = a.sy > 1 ? 1 : 0;
}

int32_t block_wgs_of(const JbLjWindow &w, int hs, int vs) { return (int32_t)(((int64_t)w.nx * w.ny * (hs * vs + 2) + 255) / 256); }

// the block launch of a's block sizes: one instantiation per (luma, chroma) pair that a layout and a draft can give
template <class... Table>
hipError_t launch_blocks(const LjArgs &a, uint32_t grid, hipStream_t stream, const JbLaunch &p, const Table &...table) {
#define JB_LJ_PAIR(SY, SC)                                                                                                  \
  if (a.sy == SY && a.sc == SC) {                                                                                           \
    if constexpr (sizeof...(Table) == 0) hipLaunchKernelGGL((jb_lj_block_kernel<SY, SC>), dim3(grid), dim3(256), 0, stream, p, a); \
    else hipLaunchKernelGGL((jb_lj_block_kernel_crops<SY, SC>), dim3(grid), dim3(256), 0, stream, p, a, table...);                 \
    return hipGetLastError();                                                                                               \
  }
  JB_LJ_PAIR(8, 8)
  JB_LJ_PAIR(4, 4)
  JB_LJ_PAIR(4, 8)
  JB_LJ_PAIR(2, 2)
  JB_LJ_PAIR(2, 4)
  JB_LJ_PAIR(1, 1)
  JB_LJ_PAIR(1, 2)
#undef JB_LJ_PAIR
  return hipErrorInvalidValue;
}

}  // namespace

JbLjWindow jbk_lj_window(int hs, int vs, int draft, int mcus_x, int mcus_y, int x, int y, int w, int h) {
  LjArgs a;
  memset(&a, 0, sizeof a);
  set_layout(a, hs, vs, draft_ok(draft) ? draft : 1);
  const int mw = hs * a.sy, mh = vs * a.sy;  // an MCU in pixels of the (draft) frame: never less than one
  int mx0 = x / mw, mx1 = (x + w - 1) / mw, my0 = y / mh, my1 = (y + h - 1) / mh;
  // one chroma sample of halo is one MCU at the most; only a direction the upsampler filters has neighbours to look at
  if (a.eh == 2 && a.fancy) mx0 -= 1, mx1 += 1;
  if (a.ev == 2 && a.fancy) my0 -= 1, my1 += 1;
  if (mx0 < 0) mx0 = 0;
  if (my0 < 0) my0 = 0;
  if (mx1 > mcus_x - 1) mx1 = mcus_x - 1;
  if (my1 > mcus_y - 1) my1 = mcus_y - 1;
  JbLjWindow win;
  win.mx = mx0, win.my = my0, win.nx = mx1 - mx0 + 1, win.ny = my1 - my0 + 1;
  win.bytes = (((int64_t)win.nx * win.ny * (hs * vs * a.sy * a.sy + 2 * a.sc * a.sc)) + 255) & ~(int64_t)255;
  return win;
}

int jbk_lj_tiles(int w, int h) {
  const int64_t t = (int64_t)((w + 255) / 256) * ((h + 3) / 4);
  return t > 0x7fffffffLL ? 0 : (int)t;
}

hipError_t jbk_lj_launch(const JbLaunch &p, int hs, int vs, int draft, void *planes, hipStream_t stream) {
  if (p.n_tiles <= 0) return hipSuccess;
  if (!layout_ok(hs, vs) || !draft_ok(draft) || !planes || p.roi > 1 || p.format < 0 || p.format > 3 || p.tiles_per_image < 1 ||
      p.n_tiles % p.tiles_per_image != 0)
    return hipErrorInvalidValue;
  LjArgs a;
  memset(&a, 0, sizeof a);
  LjView &v = a.one;
  if (p.roi) v.x = p.roi_x, v.y = p.roi_y, v.w = p.roi_w, v.h = p.roi_h;
  else v.x = 0, v.y = 0, v.w = p.width, v.h = p.height;
  if (v.x < 0 || v.y < 0 || v.w < 1 || v.h < 1 || v.x + (int64_t)v.w > p.width || v.y + (int64_t)v.h > p.height ||
      p.tiles_per_image != jbk_lj_tiles(v.w, v.h))
    return hipErrorInvalidValue;
  set_layout(a, hs, vs, draft);
  // (the frame the planes are read as must lie in the coded MCUs: the planes hold nothing else)
  if (p.width > (int64_t)p.mcus_x * hs * a.sy || p.height > (int64_t)p.mcus_y * vs * a.sy) return hipErrorInvalidValue;
  const JbLjWindow win = jbk_lj_window(hs, vs, draft, p.mcus_x, p.mcus_y, v.x, v.y, v.w, v.h);
  v.wmx = win.mx, v.wmy = win.my, v.wnx = win.nx, v.wny = win.ny;
  v.out_row_stride = p.rgb_row_stride;
  a.planes = (uint8_t *)planes;
  a.plane_image_stride = win.bytes;
  a.block_wgs = block_wgs_of(win, hs, vs);
  const int64_t n_images = p.n_tiles / p.tiles_per_image;
  if (n_images * a.block_wgs > 0x7fffffffLL) return hipErrorInvalidValue;
  (void)hipGetLastError();  // (the error reported below must be this launch's)
  hipError_t e = launch_blocks(a, (uint32_t)(n_images * a.block_wgs), stream, p);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jb_lj_pixel_kernel, dim3((uint32_t)p.n_tiles), dim3(256), 0, stream, p, a);
  return hipGetLastError();
}

hipError_t jbk_lj_launch_crops(const JbLaunch &p, const JbCropTable &table, int hs, int vs, int draft, void *planes, hipStream_t stream) {
  if (!layout_ok(hs, vs) || !draft_ok(draft) || !planes || p.roi != 2 || p.format != 0 || p.tiles_per_image < 1 || p.n_tiles < 1 ||
      p.n_tiles % p.tiles_per_image != 0 || p.n_tiles / p.tiles_per_image > kJbCropsPerLaunch)
    return hipErrorInvalidValue;
  const int n_images = p.n_tiles / p.tiles_per_image;
  LjArgs a;
  LjTable t;
  memset(&a, 0, sizeof a);
  memset(&t, 0, sizeof t);
  a.planes = (uint8_t *)planes;
  set_layout(a, hs, vs, draft);
  if (p.width > (int64_t)p.mcus_x * hs * a.sy || p.height > (int64_t)p.mcus_y * vs * a.sy) return hipErrorInvalidValue;
  int64_t at = 0;
  for (int i = 0; i < n_images; i++) {
    const JbCrop &c = table.c[i];
    LjView &v = t.v[i];
    if (c.x < 0 || c.y < 0 || c.w < 1 || c.h < 1 || c.x + (int64_t)c.w > p.width || c.y + (int64_t)c.h > p.height ||
        jbk_lj_tiles(c.w, c.h) < 1 || jbk_lj_tiles(c.w, c.h) > p.tiles_per_image)
      return hipErrorInvalidValue;
    const JbLjWindow win = jbk_lj_window(hs, vs, draft, p.mcus_x, p.mcus_y, c.x, c.y, c.w, c.h);
    v.x = c.x, v.y = c.y, v.w = c.w, v.h = c.h;
    v.wmx = win.mx, v.wmy = win.my, v.wnx = win.nx, v.wny = win.ny;
    v.plane_offset = at;
    v.out_offset = c.tmp_offset;
    v.out_row_stride = 3LL * c.w;
    at += win.bytes;
    const int32_t wgs = block_wgs_of(win, hs, vs);
    if (wgs > a.block_wgs) a.block_wgs = wgs;
  }
  (void)hipGetLastError();
  hipError_t e = launch_blocks(a, (uint32_t)n_images * (uint32_t)a.block_wgs, stream, p, t);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jb_lj_pixel_kernel_crops, dim3((uint32_t)p.n_tiles), dim3(256), 0, stream, p, a, t);
  return hipGetLastError();
}
