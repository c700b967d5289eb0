// jb_kernels.hip -- fused dequantize -> 8x8 inverse DCT -> YCbCr->RGB for gfx950 (MI355X).
//
// Replaces the three whole-image passes of the reference (dequantize(), inverseDCT(),
// YCbCrToRGB(): jpeg.cpp:572-590, 735-753, 544-561) with ONE kernel that reads every
// coefficient once and writes every pixel once.
//
// Work decomposition (wave64, no MFMA -- this is 8-point butterflies, not a GEMM):
//   * a workgroup owns one TILE = a run of consecutive MCUs (NB = hs*vs + 2 coded blocks per
//     MCU), sized so that every wave holds blocks of ONE kind (all luma or all chroma):
//       4:4:4  192 lanes = 64 MCUs (wave = Y | Cb | Cr)       24 KiB of coefficients, 24 KiB LDS
//       4:2:0  192 lanes = 32 MCUs (Y | Y | Cb+Cr)            24 KiB, 24 KiB
//       4:2:2, 4:4:0  256 lanes = 64 MCUs (Y | Y | Cb | Cr)   32 KiB, 32 KiB
//     always contiguous int16 coefficients in.
//     Two tilings, chosen by the host (jb_api.cpp) and compiled as separate instantiations:
//       row-bound (LINEAR=false): tiles never cross an MCU row; the last tile of a row is
//         partly empty unless mcus_x is a multiple of the tile length (4096/8192 px are);
//       linear (LINEAR=true): tiles cut the image's MCU stream every tile length regardless of
//         rows, so only the last tile of an image can be short; a colour segment may then
//         straddle one row end and is stored in two parts (1920 px: +4.2 %).
//     blockIdx -> tile is the identity (one compact advancing write window; XCD bands were slower).
//   * the front of every tile is kept short, because the kernel runs at the knee where its instruction stream just
//     stops hiding under the memory traffic (DESIGN_HISTORY.md section 4): tile -> (image, MCU row, first MCU) is two
//     multiply-and-shift pairs the launch computes (jb_divmagic.h), not two integer divisions; a full 4:4:4 tile issues
//     its eight LDS-DMA loads from two lane offsets and a scalar base that steps by 3072 bytes, with no vector
//     instruction between them (only a ragged tile clamps block numbers per load); and the wave's quantisation table is
//     fetched into SGPRs while the coefficients are on their way, not after they have arrived.
//   * stage 1+2, one lane = one coded 8x8 block.  Lanes take the tile's blocks sorted by
//     component, so the quantisation table is wave-uniform (scalar loads -> SGPRs) wherever
//     possible (4:4:4: wave w = component w).  The lane's 128 coefficient bytes reach 32 VGPRs
//     either straight from HBM (8 global_load_dwordx4 per lane; measured 6.4-6.5 TB/s although
//     every lane of an instruction touches a different line, tools/probe_load.hip) or, in 4:4:4
//     where it measured 4 % faster, through LDS-DMA (global_load_lds_dwordx4) into the wave's own
//     8 KiB of LDS with an XOR swizzle that makes the 128-B-strided ds_read_b128 conflict free.
//     Then dequantise and 16 1-D AAN passes run entirely in that lane's registers with static
//     indexing (no cross-lane traffic, no redundant arithmetic).
//   * stage 3, twice (rows 0-3 / rows 4-7 of every block): the lanes write the integer-valued
//     f32 samples of that half into planar strips in LDS (Y, Cb, Cr: 24 KiB; the other half waits
//     in registers), XOR-swizzled per 16-B chunk so ds_write_b128 is conflict free; then one lane =
//     4 horizontally adjacent pixels: ds_read_b128 of Y, the (replicated) chroma samples, the
//     colour transform, a 12-byte pack under round-toward-zero mode, and ONE
//     buffer_store_dwordx3 whose descriptor range check drops lanes past the image edge.
//     Consecutive lanes are consecutive in the image row: a wave-instruction writes 768
//     contiguous bytes (six whole 128-B lines).  All per-iteration addressing is scalar.
//     Two phases keep a workgroup at 24 KiB of LDS = 6 workgroups (18 waves) per CU (32 KiB =
//     5 workgroups of 4 waves for the 256-lane tiles); the 3
//     workgroup barriers per tile order LDS traffic only (s_waitcnt lgkmcnt(0); s_barrier).
//
// Layout of this file: the stage helpers (dequantise, IDCT passes, chroma read, colour, packs, byte store); LaneMap and
// jb_tile_kernel, the kernel described above; SmallMap and jb_small_body, the same stages as ONE 64-lane body for small
// launches, with its four entry points jb_small_kernel_444 / _420 / _16<2,1> / _16<1,2>; the launchers.
//
// Arithmetic is bit-exact with the reference: int32 dequantise (v_mul_i32_i24), the AAN graph
// of jpeg.cpp:598-662 evaluated in the same order with separate IEEE mul/add (this TU is built
// with -ffp-contract=off), truncation toward zero after each 1-D pass (v_trunc_f32: equal to the
// reference's float->int->float round trip for |x| < 2^31), colour per jpeg.cpp:521-535.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "jb_kernels.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;
typedef __attribute__((address_space(4))) int32_t q_const_t;  // scalar-loadable (constant) memory
typedef int32_t i32x16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(4))) i32x16_t q16_const_t __attribute__((aligned(4)));  // one s_load_dwordx16 of a table

__device__ __forceinline__ float kf(uint32_t bits) { return __builtin_bit_cast(float, bits); }

// f32 constants of reference include/types.hpp:5-19 (m*, s*) and jpeg.cpp:521-523, by bit pattern
#define JB_M1 kf(0x3FB504F3u)
#define JB_M2 kf(0x3F8A8BD4u)
#define JB_M3 kf(0x3FB504F3u)
#define JB_M4 kf(0x40273D74u)
#define JB_M5 kf(0x3F43EF15u)
#define JB_S0 kf(0x3EB504F3u)
#define JB_S1 kf(0x3EFB14BEu)
#define JB_S2 kf(0x3EEC835Eu)
#define JB_S3 kf(0x3ED4DB31u)
#define JB_S4 kf(0x3EB504F3u)
#define JB_S5 kf(0x3E8E39DAu)
#define JB_S6 kf(0x3E43EF15u)
#define JB_S7 kf(0x3DC7C5C2u)
#define JB_CR_R kf(0x3FB374BCu)
#define JB_CB_G kf(0x3EB020C5u)
#define JB_CR_G kf(0x3F36C8B4u)
#define JB_CB_B kf(0x3FE2D0E5u)

// Cache-policy bits (gfx940+: 1 = sc0, 2 = nt, 16 = sc1).  Every byte is touched once, so the
// LDS-DMA loads and the pixel stores are non-temporal: measured +4.8 % on the 4:4:4 stream
// (220 -> 210 us), neutral to +3 % for the stores of the other layouts.  The per-lane block
// loads of the direct path must NOT be nt: their 8 instructions re-use each 128-B line through
// L1, and nt made them 1.9x slower (154 -> 293 us on 4:2:0).
// (JB_LAB: tools/build_variant.sh builds measurement variants of this file -- other cache policies, stages
// skipped at run time -- next to the product; the product is always built without it)
#if !defined(JB_LAB) || !defined(JB_LOAD_AUX)
#undef JB_LOAD_AUX
#define JB_LOAD_AUX 2
#endif
#if !defined(JB_LAB) || !defined(JB_STORE_AUX)
#undef JB_STORE_AUX
#define JB_STORE_AUX 2
#endif
// Coded blocks per tile = lanes per workgroup: the smallest whole number of MCUs that fills whole
// waves with ONE component each.  4:4:4 (3 blocks per MCU) and 4:2:0 (6): 192 lanes = 64 / 32 MCUs
// (in 4:2:0 Cb and Cr share the third wave).  4:2:2 and 4:4:0 (4 blocks per MCU): 256 lanes = 64
// MCUs = two luma waves, a Cb wave, a Cr wave; with 192 lanes their waves mixed components, which
// cost a per-lane table select, per-lane strip addressing and a wave per SIMD.
constexpr int tile_blocks(int hs, int vs) { return hs * vs == 2 ? 256 : 192; }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() would also wait for the
// global stores of the previous colour phase (vmcnt(0)), putting HBM write latency on the
// critical path between the two phases.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// One 1-D pass of the AAN network (reference jpeg.cpp:598-662 / 666-730), in place, each
// output truncated toward zero exactly where the reference stores a float into an int.
__device__ __forceinline__ void aan_1d_io(float x0, float x1, float x2, float x3, float x4, float x5,
                                          float x6, float x7, float &y0, float &y1, float &y2,
                                          float &y3, float &y4, float &y5, float &y6, float &y7) {
  const float g0 = x0 * JB_S0;
  const float g1 = x4 * JB_S4;
  const float g2 = x2 * JB_S2;
  const float g3 = x6 * JB_S6;
  const float g4 = x5 * JB_S5;
  const float g5 = x1 * JB_S1;
  const float g6 = x7 * JB_S7;
  const float g7 = x3 * JB_S3;

  const float f4 = g4 - g7;
  const float f5 = g5 + g6;
  const float f6 = g5 - g6;
  const float f7 = g4 + g7;

  const float e2 = g2 - g3;
  const float e3 = g2 + g3;
  const float e5 = f5 - f7;
  const float e7 = f5 + f7;
  const float e8 = f4 + f6;

  const float d2 = e2 * JB_M1;
  const float d4 = f4 * JB_M2;
  const float d5 = e5 * JB_M3;
  const float d6 = f6 * JB_M4;
  const float d8 = e8 * JB_M5;

  const float c0 = g0 + g1;
  const float c1 = g0 - g1;
  const float c2 = d2 - e3;
  const float c4 = d4 + d8;
  const float c5 = d5 + e7;
  const float c6 = d6 - d8;
  const float c8 = c5 - c6;

  const float b0 = c0 + e3;
  const float b1 = c1 + c2;
  const float b2 = c1 - c2;
  const float b3 = c0 - e3;
  const float b4 = c4 - c8;
  const float b6 = c6 - e7;

  y0 = __builtin_truncf(b0 + e7);
  y1 = __builtin_truncf(b1 + b6);
  y2 = __builtin_truncf(b2 + c8);
  y3 = __builtin_truncf(b3 + b4);
  y4 = __builtin_truncf(b3 - b4);
  y5 = __builtin_truncf(b2 - c8);
  y6 = __builtin_truncf(b1 - b6);
  y7 = __builtin_truncf(b0 - e7);
}

// in place
__device__ __forceinline__ void aan_1d(float &x0, float &x1, float &x2, float &x3, float &x4,
                                       float &x5, float &x6, float &x7) {
  aan_1d_io(x0, x1, x2, x3, x4, x5, x6, x7, x0, x1, x2, x3, x4, x5, x6, x7);
}

__device__ __forceinline__ uint32_t pack_u8(float x, uint32_t byte, uint32_t old) {
  // reference jpeg.cpp:521-535: truncate toward zero, then clamp to 0..255.  v_cvt_pk_u8_f32
  // saturates to 0..255 by itself but rounds to nearest (probed on gfx950, tools/probe_cvt.hip),
  // so the truncation is explicit and the clamp is the instruction's own.
  return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_truncf(x), byte, old);
}

// 12 colour values (4 pixels x RGB, floats before truncation) -> 12 packed bytes.  The wave's
// f32 rounding mode is switched to round-toward-zero around the twelve v_cvt_pk_u8_f32, which then
// truncate AND saturate in one half-rate instruction each (bit-identical to truncate + clamp of
// reference jpeg.cpp:521-535 on all inputs: probed on gfx950, tools/probe_cvt.hip); the mode is
// back to round-to-nearest-even before any other float instruction of this wave can issue.
__device__ __forceinline__ void pack12_rtz(const float (&r)[4], const float (&g)[4], const float (&b)[4],
                                           uint32_t &w0, uint32_t &w1, uint32_t &w2) {
  asm volatile(
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
      "v_cvt_pk_u8_f32 %0, %3, 0, 0\n\t"
      "v_cvt_pk_u8_f32 %1, %8, 0, 0\n\t"
      "v_cvt_pk_u8_f32 %2, %13, 0, 0\n\t"
      "v_cvt_pk_u8_f32 %0, %4, 1, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %9, 1, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %14, 1, %2\n\t"
      "v_cvt_pk_u8_f32 %0, %5, 2, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %10, 2, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %11, 2, %2\n\t"
      "v_cvt_pk_u8_f32 %0, %6, 3, %0\n\t"
      "v_cvt_pk_u8_f32 %1, %7, 3, %1\n\t"
      "v_cvt_pk_u8_f32 %2, %12, 3, %2\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
      : "=&v"(w0), "=&v"(w1), "=&v"(w2)
      // byte order: w0 = r0 g0 b0 r1 | w1 = g1 b1 r2 g2 | w2 = b2 r3 g3 b3
      : "v"(r[0]), "v"(g[0]), "v"(b[0]), "v"(r[1]),   // %3..%6   -> w0 bytes 0..3
        "v"(g[2]), "v"(g[1]), "v"(b[1]), "v"(r[2]),   // %7 (w1 byte 3), %8..%10 -> w1 bytes 0..2
        "v"(g[3]), "v"(b[3]), "v"(b[2]), "v"(r[3]));  // %11 (w2 byte 2), %12 (w2 byte 3), %13, %14 -> w2 bytes 0,1
}

// Area-reduced output (SCALE > 1): the mean of the n u8 samples of a box, rounded half up -- floor((s + n/2) / n).
// A whole box (n = SCALE^2) divides by a shift; the clipped boxes of the last column / row (n = 1..63) exactly.
template <int SCALE>
__device__ __forceinline__ uint32_t box_mean(uint32_t s, int n) {
  constexpr int KK = SCALE * SCALE, SH = SCALE == 2 ? 2 : SCALE == 4 ? 4 : 6;
  if (n == KK) return (s + KK / 2) >> SH;
  const uint32_t d = (uint32_t)max(n, 1);
  return (s + d / 2) / d;
}

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef u32x4_t u32x4_u __attribute__((aligned(1)));  // 16 bytes at any byte address


// ---- the stages the kernels below are written with ----
// jb_tile_kernel's register allocation sits at the edge, and hipcc schedules it differently as soon as one of its
// arrays (raw, v, yy / r / g / b together) goes through a helper by reference, although every helper is inlined: there
// it calls the helpers that take values, or the chroma arrays alone, and keeps its loops over raw[] and v[] in place
// (instruction-identical to the code before the helpers existed: profiles/r07/isa_diff_existing_kernels.txt).  The
// small-grid body uses all of them.

// One coded block (eight 16-byte chunks at src) -> raw: row k = dwords 4k..4k+3, two int16 (columns 2j, 2j+1) per dword
__device__ __forceinline__ void load_block(const u32x4_t *src, uint32_t (&raw)[32]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u32x4_t t = src[j];
    raw[j * 4 + 0] = t.x, raw[j * 4 + 1] = t.y, raw[j * 4 + 2] = t.z, raw[j * 4 + 3] = t.w;
  }
}

// dequantise (jpeg.cpp:563-569) column i of a row, from the dword w that holds it: int32 product (v_mul_i32_i24),
// int->float on first use (jpeg.cpp:598)
__device__ __forceinline__ float dequant1(uint32_t w, int i, int q) {
  const int c = (i & 1) ? ((int)w >> 16) : (int)(short)(w & 0xffffu);
  return (float)__mul24(c, q);
}
// a whole block with the table at q (a lane of the small-grid kernels reads it from LDS, four entries per ds_read_b128)
__device__ __forceinline__ void dequantise(const uint32_t (&raw)[32], float (&v)[64], const int32_t *q) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int i = 0; i < 8; i += 4) {
      const int4 q4 = *(const int4 *)(q + k * 8 + i);
      const int qq[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
      for (int e = 0; e < 4; e++) v[k * 8 + i + e] = dequant1(raw[k * 4 + ((i + e) >> 1)], i + e, qq[e]);
    }
  }
}

// column pass, jpeg.cpp:596-663.  PERM: output row k goes to register row sigma(k), sigma = (0 1 4 5 2 3 6 7).
template <bool PERM = false>
__device__ __forceinline__ void idct_cols(float (&v)[64]) {
#pragma unroll
  for (int i = 0; i < 8; i++)
    aan_1d_io(v[0 * 8 + i], v[1 * 8 + i], v[2 * 8 + i], v[3 * 8 + i], v[4 * 8 + i], v[5 * 8 + i], v[6 * 8 + i], v[7 * 8 + i],
              v[0 * 8 + i], v[1 * 8 + i], v[(PERM ? 4 : 2) * 8 + i], v[(PERM ? 5 : 3) * 8 + i], v[(PERM ? 2 : 4) * 8 + i],
              v[(PERM ? 3 : 5) * 8 + i], v[6 * 8 + i], v[7 * 8 + i]);
}
// row pass, jpeg.cpp:664-731
__device__ __forceinline__ void idct_rows(float (&v)[64]) {
#pragma unroll
  for (int k = 0; k < 8; k++)
    aan_1d(v[k * 8 + 0], v[k * 8 + 1], v[k * 8 + 2], v[k * 8 + 3], v[k * 8 + 4], v[k * 8 + 5], v[k * 8 + 6], v[k * 8 + 7]);
}
__device__ __forceinline__ void idct_8x8(float (&v)[64]) { idct_cols(v), idct_rows(v); }

// The eight LDS-DMA loads with which a wave of the 4:4:4 kernel fetches the 64 blocks of a FULL tile that its own lanes
// consume (jb_tile_body.inc, stage 1: the landing zone and the swizzle are described there).  wave_coef: the tile's first
// byte + wave * 128; wave_lds: the wave's own 8 KiB.  The block of lane l2 of wave w is 3 * l2 + w, so load i reads at
// i * 3072 + (lane >> 3) * 384 + w * 128 + its swizzled chunk.  The chunk's swizzle term f2 = (i & 1) * 4 + (lane >> 4)
// flips bit 2 from one load to the next: two lane offsets that differ by 64 bytes, and a scalar base that steps by 3072.
__device__ __forceinline__ void load_full_tile_444(const uint8_t *wave_coef, char *wave_lds, int lane) {
  // (opaque, so that hipcc keeps them as the loads' 32-bit lane offsets next to a scalar base, and does not fold
  // each load's constant into a 64-bit lane address of its own)
  uint32_t off_even = (uint32_t)(lane >> 3) * 384u + (uint32_t)(((lane & 7) ^ (lane >> 4)) << 4);
  uint32_t off_odd = off_even ^ 64u;
  asm volatile("" : "+v"(off_even), "+v"(off_odd));
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t *step = wave_coef + i * 3072;
    asm volatile("" : "+s"(step));
    __builtin_amdgcn_global_load_lds((gbl_void_t *)(step + ((i & 1) ? off_odd : off_even)), (lds_void_t *)(wave_lds + i * 1024), 16, 0,
                                     JB_LOAD_AUX);
  }
}

// The chroma of four adjacent luma samples from the strips: the chroma sample of luma pixel (row, col) is
// (row/VS, col/HS) -- reference jpeg.cpp:518-520 -- so HS = 2 reads two samples and gives each to two pixels.
template <int HS>
__device__ __forceinline__ void load_chroma4(const char *pb, const char *pr, float (&cb)[4], float (&cr)[4]) {
  if (HS == 1) {
    const float4 a = *(const float4 *)pb;
    const float4 b = *(const float4 *)pr;
    cb[0] = a.x, cb[1] = a.y, cb[2] = a.z, cb[3] = a.w;
    cr[0] = b.x, cr[1] = b.y, cr[2] = b.z, cr[3] = b.w;
  } else {
    const float2 a = *(const float2 *)pb;
    const float2 b = *(const float2 *)pr;
    cb[0] = cb[1] = a.x, cb[2] = cb[3] = a.y;
    cr[0] = cr[1] = b.x, cr[2] = cr[3] = b.y;
  }
}

// colour transform of one pixel, jpeg.cpp:521-535 (floats before truncation)
__device__ __forceinline__ void ycc_px(float y, float cb, float cr, float &r, float &g, float &b) {
  r = (y + JB_CR_R * cr) + 128.0f;
  g = ((y - JB_CB_G * cb) - JB_CR_G * cr) + 128.0f;
  b = (y + JB_CB_B * cb) + 128.0f;
}

// The full-size conversion with its operands permuted: pack12_rtz writes bytes in the order r0 g0 b0 r1 | g1 b1 r2 g2 |
// b2 r3 g3 b3, so these arguments give ONE word per channel -- w[c] = the u8 samples of channel c, pixels 0..3.
__device__ __forceinline__ void pack_channels(const float (&r)[4], const float (&g)[4], const float (&b)[4], uint32_t (&w)[3]) {
  const float pr[4] = {r[0], r[3], g[2], b[1]}, pg[4] = {r[1], g[0], g[3], b[2]}, pb[4] = {r[2], g[1], b[0], b[3]};
  pack12_rtz(pr, pg, pb, w[0], w[1], w[2]);
}

// one pixel through three byte stores
__device__ __forceinline__ void store_px_bytes(uint8_t *o, float r, float g, float b) {
  o[0] = (uint8_t)pack_u8(r, 0, 0);
  o[1] = (uint8_t)pack_u8(g, 0, 0);
  o[2] = (uint8_t)pack_u8(b, 0, 0);
}

// Measurement variants (tools/ablate.sh through tools/build_variant.sh -DJB_LAB -DJB_EXP_NO_...): a stage is
// skipped at run time through a condition the compiler cannot fold, so the code and its registers stay.  The
// product is built without JB_LAB: every stage always runs.
#if defined(JB_LAB) && defined(JB_EXP_NO_LOAD)
#define JB_DO_LOAD(p) ((p).reserved == 777)
#else
#define JB_DO_LOAD(p) true
#endif
#if defined(JB_LAB) && defined(JB_EXP_NO_IDCT)
#define JB_DO_IDCT(p) ((p).reserved == 777)
#else
#define JB_DO_IDCT(p) true
#endif
#if defined(JB_LAB) && defined(JB_EXP_NO_COLOUR)
#define JB_DO_COLOUR(p) ((p).reserved == 777)
#else
#define JB_DO_COLOUR(p) true
#endif
#if defined(JB_LAB) && defined(JB_EXP_NO_STORE)
#define JB_DO_STORE(p) ((p).reserved == 777)
#else
#define JB_DO_STORE(p) true
#endif

}  // namespace

// Sorted-lane mapping: lanes take the tile's blocks sorted by component (all Y, then Cb, then
// Cr) so that a wave holds at most two components.  4:4:4: wave w = component w (its
// quantisation table is wave-uniform and lives in SGPRs); 4:2:0: waves 0,1 luma, wave 2 half Cb,
// half Cr.  s = sorted index 0..191.
template <int HS, int VS>
struct LaneMap {
  static constexpr int TB = tile_blocks(HS, VS);
  static constexpr int NY = HS * VS, NB = NY + 2, MCUS = TB / NB, NYT = NY * MCUS;
  __device__ static __forceinline__ int comp(int s) { return s < NYT ? 0 : (s < NYT + MCUS ? 1 : 2); }
  __device__ static __forceinline__ int mcu(int s) {
    const int c = comp(s);
    return c == 0 ? s / NY : s - NYT - (c - 1) * MCUS;
  }
  __device__ static __forceinline__ int slot(int s) { return comp(s) == 0 ? s % NY : 0; }  // luma block in MCU
  __device__ static __forceinline__ int block(int s) {                                      // decode order
    const int c = comp(s);
    return mcu(s) * NB + (c == 0 ? slot(s) : NY + c - 1);
  }
};

// the rows of a kernel's by-value table argument
static __device__ __forceinline__ const JbCrop *crops_of(const JbCropTable &table) { return table.c; }

// One workgroup (192 or 256 lanes) per tile.  See the file header for the three stages.
// MIXQ = false: every wave dequantises with ONE table (4:4:4 always; 4:2:0 when Cb and Cr name the
// same table, the usual case).  MIXQ = true: a wave may hold blocks of two components with
// different tables and selects per lane; kept out of the MIXQ = false instantiation because its
// register pressure would cost the common case a wave per SIMD.
// STAGED = true (linear tiling only): the colour stage packs the pixels back into LDS and the same wave then writes
// the strip row as whole 64-byte lines plus byte runs at its two ends, instead of one 12-byte store per lane at
// whatever alignment the row has (see "staged" below).  A MEASURED VARIANT, not a product path: it is only
// instantiated in -DJB_LAB builds (tools/build_variant.sh; JPEGBLK_STAGED_STORE=1 selects it there).  On the sizes
// it was meant for it is 1-3 % slower than the stores it replaces, and 4-10 % slower on aligned rows
// (profiles/r03/probe_staged.json): the aligned lines are worth about 5 %, the second trip
// through LDS and the serial pack-then-copy of a row per wave cost more.
// SCALE = 2, 4, 8 (row-bound tiling only): the area-reduced output (jbk_launch with a scale) -- stages 1 and 2 and the
// colour transform and u8 conversion of every pixel are those of SCALE = 1; only what is stored differs (see
// "scaled" below).  p.width / p.height stay the full image's; p.rgb and its strides describe the reduced image.
// FORMAT = 1, 2, 3 (JB_FMT_RGB_U8_CHW, _F32_CHW, _F16_CHW; row-bound tiling only, SCALE = 1): the planar output
// (jbk_launch with p.format set) -- again only what is stored differs (see "planar" below): the u8 values are those of FORMAT = 0.
// ROI = 1 (jbk_launch with p.roi set; row-bound tiling only, SCALE = 1, any FORMAT): the rectangle p.roi_x, p.roi_y,
// p.roi_w, p.roi_h of the image in that format -- the grid covers only the MCUs the rectangle touches, and the store
// stage (see "region of interest" below) writes only the pixels inside it.
// ROI = 2 (jbk_launch_crops; FORMAT = 0 only): the same with a rectangle per image, read from `table` (a kernel
// argument: the index is workgroup-uniform, so the reads are scalar loads from the argument segment).  The grid gives
// every image p.tiles_per_image workgroups, the most any image of the launch needs; a workgroup beyond its own image's
// n_tiles returns before its first load and its first barrier.  Image i is written as tight rows at p.rgb + tmp_offset.
// TABLE is empty but for ROI = 2, where it is JbCropTable: only those instantiations have a second kernel argument.
// FLAT = true (jb_tile_kernel_flat: 4:4:4, SCALE = 1, ROI = 0, the launches of jbk_flat_front): every tile is full and
// workgroup t's coefficients lie at flat_coef + t * 24576, flat_coef = p.coef as a leading scalar argument that arrives in
// SGPRs with the wave.  The eight loads are issued from it at once -- in front of the wait for p, which a wave otherwise
// sits out with nothing in flight, and of the tile arithmetic, which moves behind them -- and nothing else changes.
template <int HS, int VS, bool MIXQ, bool LINEAR, bool STAGED = false, int SCALE = 1, int FORMAT = 0, int ROI = 0, typename... TABLE>
// (5 waves/SIMD are asked for where that costs no spill: 4:4:4 and 4:4:0; forcing it on 4:2:0 or
// 4:2:2 spills and measured 9 % slower; the scaled 4:4:0 instantiations spill at 5 too)
__global__ __launch_bounds__(tile_blocks(HS, VS), (HS == 1 && (SCALE == 1 || VS == 1)) ? 5 : 1) void jb_tile_kernel(const JbLaunch p, const TABLE... table) {
  constexpr bool FLAT = false;
  [[maybe_unused]] const uint8_t *const flat_coef = nullptr;
#include "jb_tile_body.inc"
}
// The flat entry.  flat_coef stands in front of the structure: a leading scalar argument is delivered in SGPRs when the wave
// starts (kernel-argument preload: jb_kernels.o is built with -mllvm -amdgpu-kernarg-preload-count=1, which leaves a kernel
// whose first argument is a structure as it is; where the firmware does not preload, the compiler's prologue loads the same
// scalar and the entry keeps its shorter address chain).  TABLE: always empty, there for the body's sake.
template <bool LINEAR, int FORMAT, typename... TABLE>
__global__ __launch_bounds__(tile_blocks(1, 1), 5) void jb_tile_kernel_flat(const uint8_t *flat_coef, const JbLaunch p, const TABLE... table) {
  constexpr int HS = 1, VS = 1, SCALE = 1, ROI = 0;
  constexpr bool MIXQ = false, STAGED = false, FLAT = true;
#include "jb_tile_body.inc"
}

// ---- small grids: one WAVE per 16 (4:2:0: 8) MCUs -------------------------------------------------------------
// A single 1080p 4:4:4 image is 507 tiles of the kernel above on 256 CUs: every CU runs its two workgroups through
// load -> IDCT -> colour in step, and the launch is bounded by the length of that chain, not by traffic (DESIGN.md
// section 5.2).  These kernels cut the same work into four times as many independent pieces: a 64-lane workgroup
// owns MCUS MCUs of one MCU row, one lane per coded block, with the quantisation tables in LDS (per-lane component),
// 6-8 KiB of strips, and no barrier other workgroups wait on, so the phases of the eight or so waves on a CU
// interleave.  Arithmetic and its order are those of the kernel above.
// Selected by the host for launches of fewer than 3 workgroups per CU (jb_api.cpp; JPEGBLK_SMALL_GRID).
//
// Lane -> block, the counterpart of LaneMap: the luma blocks first (MCU l / NY, block l % NY in decode order), then
// MCUS Cb lanes, then MCUS Cr lanes:
//   4:4:4  16 MCUs: lanes 0-15 Y, 16-31 Cb, 32-47 Cr, 48-63 idle
//   4:2:0   8 MCUs: lanes 0-31 Y (top left, top right, bottom left, bottom right), 32-39 Cb, 40-47 Cr, 48-63 idle
//   4:2:2, 4:4:0  16 MCUs: lanes 0-31 Y (left / right, or top / bottom), 32-47 Cb, 48-63 Cr: the wave is full
// An idle lane repeats a Cr lane's loads and arithmetic, writes nothing into the strips, and takes part in the colour loop.
// Strips per phase: YROWS = 4 * VS luma rows (rows 4p..4p+3 of every block row) x YW samples, and the 4 chroma rows
// they need x CW samples per chroma component (VS = 2: rows 2p, 2p+1, 4+2p, 5+2p of the block, reference
// jpeg.cpp:518-520 -- a chroma lane picks them with a select per value; the 192-lane kernel permutes them in the
// column pass, which a wave of mixed lanes cannot).  The strips are skewed by 64 bytes so that they start in different banks.
template <int HS, int VS>
struct SmallMap {
  static_assert((HS == 1 || HS == 2) && (VS == 1 || VS == 2), "the four layouts of the ABI");
  static constexpr int NY = HS * VS, NB = NY + 2;
  static constexpr int MCUS = NY == 4 ? 8 : 16;       // MCUs per workgroup
  static constexpr int NYL = NY * MCUS;               // luma lanes
  static constexpr bool kFull = NB * MCUS == 64;      // no idle lanes
  static constexpr int YW = MCUS * 8 * HS, CW = MCUS * 8;   // strip widths in samples
  static constexpr int YROWS = 4 * VS;                // luma strip rows per phase
  static constexpr int kYStrip = YROWS * YW * 4 + (NY == 1 ? 64 : 0);  // bytes; 4:4:4 skews the luma strip too
  static constexpr int kCStrip = 4 * CW * 4 + 64;
  static constexpr int kQPitch = 64 + 4;              // dwords per table in LDS (the three tables start in different banks)
  static constexpr int kLds = kYStrip + 2 * kCStrip + 3 * kQPitch * 4;
  static constexpr int TPR = YW / 4;                  // 4-pixel tasks per row: 32, or 64 (4:2:2)
  static constexpr int ROWS_PER_IT = 64 / TPR;        // pixel rows per wave-iteration
  __device__ static __forceinline__ bool active(int l) { return kFull || l < NB * MCUS; }
  __device__ static __forceinline__ int comp(int l) { return l < NYL ? 0 : (l < NYL + MCUS ? 1 : 2); }
  __device__ static __forceinline__ int mcu(int l) { return l < NYL ? l / NY : (l & (MCUS - 1)); }
  __device__ static __forceinline__ int slot(int l) { return l < NYL ? l % NY : NY + comp(l) - 1; }  // block of the MCU in decode order
};

template <int HS, int VS>
__device__ __forceinline__ void jb_small_body(const JbLaunch &p) {
  using SM = SmallMap<HS, VS>;
  constexpr int MCUS = SM::MCUS, NB = SM::NB, YW = SM::YW, kYStrip = SM::kYStrip, kCStrip = SM::kCStrip, kCPitch = SM::CW * 4;
  __shared__ __attribute__((aligned(16))) char lds[SM::kLds];
  int32_t *const qlds = (int32_t *)(lds + kYStrip + 2 * kCStrip);
  const int lane = threadIdx.x;
  const int tile = blockIdx.x;
  const int img = tile / p.tiles_per_image;
  const int rem = tile - img * p.tiles_per_image;
  const int my = rem / p.tiles_per_row;
  const int mx0 = (rem - my * p.tiles_per_row) * MCUS;
  const int nvalid = min(MCUS, p.mcus_x - mx0);
  const int comp = SM::comp(lane), m = SM::mcu(lane), slot = SM::slot(lane);
  const uint8_t *tile_coef = (const uint8_t *)p.coef + (int64_t)img * p.coef_image_stride + ((int64_t)my * p.mcus_x + mx0) * (NB * 128);
  const int32_t *qsrc = (const int32_t *)((const uint8_t *)p.qtabs + (int64_t)img * p.qtab_image_stride);
#pragma unroll
  for (int i = 0; i < 3; i++) qlds[i * SM::kQPitch + lane] = qsrc[i * 64 + lane];
  float v[64];
  {
    uint32_t raw[32];
    load_block((const u32x4_t *)(tile_coef + (uint32_t)(min(m, nvalid - 1) * NB + slot) * 128u), raw);  // ragged: re-read the last MCU
    __syncthreads();  // the tables are in LDS
    dequantise(raw, v, qlds + comp * SM::kQPitch);
  }
  idct_8x8(v);

  // where this lane's block lands: luma block (bv, bh) of MCU m in strip rows 4*bv.., 8-sample column HS*m + bh; a
  // chroma block in its component's strip, column m.  16-B chunk c of a row is stored at c ^ ((c >> 3) & 1) (as above).
  const bool luma = comp == 0;
  const int bv = luma ? slot / HS : 0, bh = luma ? slot % HS : 0;
  const int col = luma ? m * HS + bh : m;
  const int sw = (col >> 2) & 1;
  const int pitch = luma ? YW * 4 : kCPitch;
  char *const dst = lds + (luma ? bv * 4 * (YW * 4) : kYStrip + (comp - 1) * kCStrip) + col * 32;
  // colour stage: one lane = 4 adjacent pixels, a wave-iteration = ROWS_PER_IT pixel rows
  const int x4 = lane & (SM::TPR - 1);
  const int rd_y = (x4 ^ ((x4 >> 3) & 1)) * 16;
  const int rd_c = HS == 2 ? ((x4 >> 1) ^ ((x4 >> 4) & 1)) * 16 + (x4 & 1) * 8 : rd_y;  // HS = 2: chroma chunk x4 / 2, its half x4 & 1
  uint8_t *const img_rgb = p.rgb + (int64_t)img * p.rgb_image_stride;
  const int x = mx0 * 8 * HS + x4 * 4;  // image column of this lane's first pixel
  const int npx = min(4, min(nvalid * 8 * HS, p.width - mx0 * 8 * HS) - x4 * 4);  // its pixels inside the image (<= 0: none)
#pragma unroll
  for (int phase = 0; phase < 2; phase++) {
    if (phase == 1) __syncthreads();
    if (SM::active(lane)) {
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
        const int kl = phase * 4 + kk;                                       // rows 4p .. 4p+3 of the block
        const int kc = VS == 2 ? phase * 2 + (kk & 1) + (kk >> 1) * 4 : kl;  // VS = 2 chroma: rows 2p, 2p+1, 4+2p, 5+2p
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (VS == 2 && !luma) ? v[kc * 8 + e] : v[kl * 8 + e];
        *(float4 *)(dst + kk * pitch + sw * 16) = make_float4(o[0], o[1], o[2], o[3]);
        *(float4 *)(dst + kk * pitch + (sw ^ 1) * 16) = make_float4(o[4], o[5], o[6], o[7]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SM::YROWS / SM::ROWS_PER_IT; it++) {
      const int r = it * SM::ROWS_PER_IT + (SM::ROWS_PER_IT == 2 ? lane >> 5 : 0);  // luma strip row
      const int y_in = phase * 4 + (r >> 2) * 8 + (r & 3);                          // pixel row within the MCU row
      const int y = my * 8 * VS + y_in;
      const float4 Y = *(const float4 *)(lds + r * (YW * 4) + rd_y);
      const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
      float cb[4], cr[4], rr[4], gg[4], bb[4];
      const int crow = (r / VS) * kCPitch;
      load_chroma4<HS>(lds + kYStrip + crow + rd_c, lds + kYStrip + kCStrip + crow + rd_c, cb, cr);
#pragma unroll
      for (int i = 0; i < 4; i++) ycc_px(yy[i], cb[i], cr[i], rr[i], gg[i], bb[i]);
      if (p.fast_store) {
        uint32_t w0, w1, w2;
        pack12_rtz(rr, gg, bb, w0, w1, w2);
        if (y < p.height && npx == 4) {
          // a wave-uniform descriptor at row 0 of the MCU row; the lane adds its row (a 32-bit offset: the host keeps
          // rgb_row_stride below 2^26) and column
          uint8_t *const rows = img_rgb + (int64_t)(my * 8 * VS) * p.rgb_row_stride + (int64_t)mx0 * (24 * HS);
          const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(rows, 0, 0x7ffffff0, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b96(u32x3_t{w0, w1, w2}, rsrc, y_in * (int)p.rgb_row_stride + x4 * 12, 0, JB_STORE_AUX);
        }
      }
      uint8_t *const o = img_rgb + (int64_t)y * p.rgb_row_stride + (int64_t)x * 3;
      if (y < p.height && npx > 0 && (!p.fast_store || npx < 4)) {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i < npx) store_px_bytes(o + i * 3, rr[i], gg[i], bb[i]);
      }
    }
  }
}

// the entry points (bench.py and the committed profiles know the kernels by these names)
__global__ __launch_bounds__(64) void jb_small_kernel_444(const JbLaunch p) { jb_small_body<1, 1>(p); }
__global__ __launch_bounds__(64) void jb_small_kernel_420(const JbLaunch p) { jb_small_body<2, 2>(p); }
template <int HS, int VS>
__global__ __launch_bounds__(64) void jb_small_kernel_16(const JbLaunch p) {
  static_assert(HS * VS == 2, "the four-blocks-per-MCU layouts: 4:2:2 and 4:4:0");
  jb_small_body<HS, VS>(p);
}

// the arguments with the prologue's division pairs (jb_divmagic.h) filled from the launch's own divisors: here, in front
// of the two places that launch jb_tile_kernel, so that no caller can pass a pair that does not match its divisor
static JbLaunch with_div(const JbLaunch &a) {
  JbLaunch p = a;
  p.div_tiles_per_image = jb_div_make(a.tiles_per_image);
  p.div_tiles_per_row = jb_div_make(a.tiles_per_row);
  p.div_mcus_x = jb_div_make(a.mcus_x);
  return p;
}

// Launches jb_tile_kernel<HS, VS, MIXQ, LINEAR, STAGED, SCALE, FORMAT, ROI>: every launch of the 192-lane kernel goes through
// here.  SCALE != 1 (the area-reduced store stage), FORMAT != 0 (the planar one) and ROI exist in the row-bound tiling only.
// MIXQ is decided here, and MIXQ = true is only instantiated for a layout that can need it.
template <int HS, int VS, int SCALE, int FORMAT, bool LINEAR = false, bool STAGED = false, int ROI = 0>
static hipError_t launch_tile(const JbLaunch &a, hipStream_t stream, bool flat = false) {
  const JbLaunch p = with_div(a);
  using LM = LaneMap<HS, VS>;
  if (flat) {  // the flat entry: the instantiations that have one, and only a launch it is true of
    if constexpr (HS == 1 && VS == 1 && SCALE == 1 && !STAGED && ROI == 0) {
      if (!jbk_flat_front(p, HS, VS, SCALE)) return hipErrorInvalidValue;
      (void)hipGetLastError();
      hipLaunchKernelGGL((jb_tile_kernel_flat<LINEAR, FORMAT>), dim3(p.n_tiles), dim3(LM::TB), 0, stream, (const uint8_t *)p.coef, p);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  }
  // does any wave hold two components whose tables may differ?  (never luma and chroma: jb_tile_kernel asserts it)
  constexpr bool kCbCrMixed = (LM::MCUS % 64 != 0);  // 4:2:0: Cb and Cr share the third wave
  const dim3 grid(p.n_tiles), block(LM::TB);
  // hipGetLastError below must report THIS launch: an error left in the thread's error slot by an
  // unrelated earlier call (a failed attribute query, say) is not this launch's
  (void)hipGetLastError();
  bool mixq = false;
  if constexpr (kCbCrMixed) {
    mixq = !p.chroma_q_equal;
    if (mixq) hipLaunchKernelGGL((jb_tile_kernel<HS, VS, true, LINEAR, STAGED, SCALE, FORMAT, ROI>), grid, block, 0, stream, p);
  }
  if (!mixq) hipLaunchKernelGGL((jb_tile_kernel<HS, VS, false, LINEAR, STAGED, SCALE, FORMAT, ROI>), grid, block, 0, stream, p);
  return hipGetLastError();
}

// one layout: which store stage (scale, p.format) and which tiling (p.linear, p.staged)
template <int HS, int VS>
static hipError_t launch_layout(const JbLaunch &p, int scale, hipStream_t stream, bool flat) {
  if (flat && (p.roi || scale != 1)) return hipErrorInvalidValue;
  if (p.roi) {  // the region of interest: its own store stage for every format, even when the rectangle is the whole image
    if (p.linear || scale != 1 || p.roi != 1) return hipErrorInvalidValue;  // (full-size row-bound tiling only; 2: jbk_launch_crops)
    if (p.format == 0) return launch_tile<HS, VS, 1, 0, false, false, 1>(p, stream);
    if (p.format == 1) return launch_tile<HS, VS, 1, 1, false, false, 1>(p, stream);
    if (p.format == 2) return launch_tile<HS, VS, 1, 2, false, false, 1>(p, stream);
    if (p.format == 3) return launch_tile<HS, VS, 1, 3, false, false, 1>(p, stream);
    return hipErrorInvalidValue;
  }
  if (p.format == 0 && scale == 1) {
    // the linear tiling is a separate instantiation: where the row-bound tiling leaves no tile
    // ragged (mcus_x a multiple of the tile length, e.g. 4096- and 8192-pixel rows) the simpler
    // row-bound code is 2 % faster
    constexpr bool kCanLinear = ((LaneMap<HS, VS>::MCUS * 8 * HS / 4) % 64 == 0);
#if defined(JB_LAB)
    if (kCanLinear && p.linear && p.staged) return launch_tile<HS, VS, 1, 0, kCanLinear, kCanLinear>(p, stream);
#endif
    if (kCanLinear && p.linear) return launch_tile<HS, VS, 1, 0, kCanLinear>(p, stream, flat);
    return launch_tile<HS, VS, 1, 0>(p, stream, flat);
  }
  if (p.linear) return hipErrorInvalidValue;  // (row-bound tiling only)
  if (p.format == 0) {  // the area-reduced output
    if (scale == 2) return launch_tile<HS, VS, 2, 0>(p, stream);
    if (scale == 4) return launch_tile<HS, VS, 4, 0>(p, stream);
    if (scale == 8) return launch_tile<HS, VS, 8, 0>(p, stream);
  } else if (scale == 1) {  // the planar output
    if (p.format == 1) return launch_tile<HS, VS, 1, 1>(p, stream, flat);
    if (p.format == 2) return launch_tile<HS, VS, 1, 2>(p, stream, flat);
    if (p.format == 3) return launch_tile<HS, VS, 1, 3>(p, stream, flat);
  }
  return hipErrorInvalidValue;
}

// the per-image rectangles: as launch_tile, with the table as the second kernel argument
template <int HS, int VS>
static hipError_t launch_crops(const JbLaunch &a, const JbCropTable &table, hipStream_t stream) {
  const JbLaunch p = with_div(a);  // (tiles_per_row is the table's, per image: the ROI = 2 kernels divide by it)
  using LM = LaneMap<HS, VS>;
  constexpr bool kCbCrMixed = (LM::MCUS % 64 != 0);
  const dim3 grid(p.n_tiles), block(LM::TB);
  (void)hipGetLastError();
  bool mixq = false;
  if constexpr (kCbCrMixed) {
    mixq = !p.chroma_q_equal;
    if (mixq) hipLaunchKernelGGL((jb_tile_kernel<HS, VS, true, false, false, 1, 0, 2, JbCropTable>), grid, block, 0, stream, p, table);
  }
  if (!mixq) hipLaunchKernelGGL((jb_tile_kernel<HS, VS, false, false, false, 1, 0, 2, JbCropTable>), grid, block, 0, stream, p, table);
  return hipGetLastError();
}

hipError_t jbk_launch_crops(const JbLaunch &p, const JbCropTable &table, int hs, int vs, hipStream_t stream) {
  // every workgroup indexes the table with tile / tiles_per_image: the grid must be whole images, at most a table's worth
  if (p.roi != 2 || p.linear || p.small_grid || p.format != 0 || p.tiles_per_image < 1 || p.n_tiles < 1 ||
      p.n_tiles % p.tiles_per_image != 0 || p.n_tiles / p.tiles_per_image > kJbCropsPerLaunch)
    return hipErrorInvalidValue;
  if (hs == 1 && vs == 1) return launch_crops<1, 1>(p, table, stream);
  if (hs == 2 && vs == 1) return launch_crops<2, 1>(p, table, stream);
  if (hs == 1 && vs == 2) return launch_crops<1, 2>(p, table, stream);
  if (hs == 2 && vs == 2) return launch_crops<2, 2>(p, table, stream);
  return hipErrorInvalidValue;
}

int jbk_mcus_per_tile(int hs, int vs) { return tile_blocks(hs, vs) / (hs * vs + 2); }

// The linear tiling needs MCU rows at least one 256-pixel segment long, so that a segment wraps to
// the next MCU row at most once.
int jbk_linear_ok(int hs, int vs, int mcus_x) {
  const int strip_tasks_per_row = jbk_mcus_per_tile(hs, vs) * 8 * hs / 4;
  if (strip_tasks_per_row % 64 != 0) return 0;  // (no layout: see tile_blocks)
  return mcus_x >= 256 / (8 * hs);
}

int jbk_small_mcus(int hs, int vs) {
  return hs == 2 ? (vs == 2 ? SmallMap<2, 2>::MCUS : SmallMap<2, 1>::MCUS) : (vs == 2 ? SmallMap<1, 2>::MCUS : SmallMap<1, 1>::MCUS);
}

hipError_t jbk_launch(const JbLaunch &p, int hs, int vs, int scale, hipStream_t stream, bool flat) {
  if (p.n_tiles <= 0) return hipSuccess;
  if (flat && p.small_grid) return hipErrorInvalidValue;
  if (p.small_grid) {  // (the host sets it with the tile counts of this tiling)
    void (*kernel)(const JbLaunch) = hs == 1 && vs == 1   ? jb_small_kernel_444
                                     : hs == 2 && vs == 2 ? jb_small_kernel_420
                                     : hs == 2 && vs == 1 ? jb_small_kernel_16<2, 1>
                                     : hs == 1 && vs == 2 ? jb_small_kernel_16<1, 2>
                                                          : nullptr;
    if (!kernel || scale != 1 || p.format != 0 || p.roi) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3(p.n_tiles), dim3(64), 0, stream, p);
    return hipGetLastError();
  }
  if (hs == 1 && vs == 1) return launch_layout<1, 1>(p, scale, stream, flat);
  if (hs == 2 && vs == 1) return launch_layout<2, 1>(p, scale, stream, flat);
  if (hs == 1 && vs == 2) return launch_layout<1, 2>(p, scale, stream, flat);
  if (hs == 2 && vs == 2) return launch_layout<2, 2>(p, scale, stream, flat);
  return hipErrorInvalidValue;
}

const char *jbk_kernel_name(int hs, int vs) {
  // <HS, VS, MIXQ, LINEAR>: LINEAR depends on the image width; MIXQ only exists for 4:2:0 whose
  // Cb and Cr name different tables
  if (hs == 1 && vs == 1) return "jb_tile_kernel<1, 1, false, *>";
  if (hs == 2 && vs == 1) return "jb_tile_kernel<2, 1, false, *>";
  if (hs == 1 && vs == 2) return "jb_tile_kernel<1, 2, false, *>";
  return "jb_tile_kernel<2, 2, *, *>";
}
