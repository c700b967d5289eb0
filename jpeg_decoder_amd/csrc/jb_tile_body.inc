// jb_tile_body.inc -- the body of the tile kernel, included by its two entries in jb_kernels.hip (see there: "One workgroup
// per tile"): jb_tile_kernel and jb_tile_kernel_flat.  Text, not a function: hipcc's register allocation of this kernel sits
// at the edge, and the body as an inlined function of both entries -- the arguments by reference or by value -- changed the
// registers of 27 of the 65 existing instantiations and gave one of them scratch.  Included this way all 65 keep their
// registers and their instruction count, and the 52 that do not use load_full_tile_444 their instructions to the letter
// (profiles/r22/resources_tile_kernels.txt).  The including kernel provides the template
// parameters HS, VS, MIXQ, LINEAR, STAGED, SCALE, FORMAT, ROI and FLAT as constants, the arguments p and table..., and
// flat_coef (FLAT only; otherwise null and unused).
  static_assert(!STAGED || LINEAR, "the staged store stage is an instantiation of the linear tiling");
  static_assert(SCALE == 1 || (!LINEAR && !STAGED && (SCALE == 2 || SCALE == 4 || SCALE == 8)),
                "the scaled store stage is an instantiation of the row-bound tiling");
  static_assert(FORMAT == 0 || (!LINEAR && !STAGED && SCALE == 1 && FORMAT >= 1 && FORMAT <= 3),
                "the planar store stage is an instantiation of the full-size row-bound tiling");
  static_assert(!ROI || (!LINEAR && !STAGED && SCALE == 1), "the ROI store stage is an instantiation of the full-size row-bound tiling");
  static_assert(ROI >= 0 && ROI <= 2 && (ROI != 2 || FORMAT == 0), "the per-image rectangles exist for the interleaved uint8 intermediate only");
  static_assert(sizeof...(TABLE) == (ROI == 2 ? 1 : 0), "the table is the second argument of the ROI = 2 instantiations alone");
  using LM = LaneMap<HS, VS>;
  constexpr int kTileBlocks = LM::TB;
  constexpr int kStripBytes = kTileBlocks * 128;  // half of the tile's f32 samples: 24 or 32 KiB
  constexpr int NB = LM::NB, MCUS = LM::MCUS, NYT = LM::NYT;
  constexpr int YW = MCUS * 8 * HS;             // luma strip width in pixels
  constexpr int CW = MCUS * 8;                  // chroma strip width in samples
  constexpr int YROWS = 4 * VS;                 // luma rows per phase (half of the tile's rows)
  constexpr int CB_OFF = YROWS * YW * 4;        // byte offsets of the strips in LDS
  constexpr int CR_OFF = CB_OFF + 4 * CW * 4;
  static_assert(CR_OFF + 4 * CW * 4 == kStripBytes, "strips must fill the strip area exactly");
  static_assert(NYT % 64 == 0, "whole luma waves: no wave mixes luma and chroma blocks");
  constexpr bool kPermChroma = (VS == 2) && (NYT % 64 == 0);  // 4:2:0: chroma blocks fill a whole wave
  // The 4-pixel group that straddles the right image edge (width % 4 != 0): two stores from the packed
  // words in the linear tiling -- the one small and odd-sized images take, where every row has such a
  // group -- and the byte-store loop elsewhere: in the row-bound instantiations (4096 / 8192-pixel
  // rows, where the case needs a width like 4093) and in 4:4:0 the extra code cost a wave per SIMD
  // or spilled (hipcc's allocation of this kernel is at the edge: 94-96 of 96 VGPRs).
  constexpr bool kTwoStoreTail = LINEAR && !(HS == 1 && VS == 2);
  constexpr bool kDirectLoad = !((NYT % 64 == 0) && (MCUS % 64 == 0) && (CB_OFF == 8192));  // all but 4:4:4
  __shared__ __attribute__((aligned(1024))) char lds[kStripBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  static_assert(!FLAT || (!kDirectLoad && !MIXQ && !STAGED && SCALE == 1 && ROI == 0), "the flat front end is the full-size 4:4:4 kernel's");

  int tile = blockIdx.x;
  if constexpr (FLAT) {
    // stage 1's loads (see there), from the preloaded base: 64-bit, the batch may be longer than 4 GiB
    if (JB_DO_LOAD(p)) load_full_tile_444(flat_coef + (uint64_t)blockIdx.x * kStripBytes + wave * 128, lds + wave * 8192, lane);
    // (everything below hangs on `tile`: opaque here, so that none of it -- and no wait for p -- is scheduled above the loads)
    asm volatile("" : "+s"(tile));
  }

  // ---- which tile (all wave-uniform) ----
  const int tiles_per_image = p.tiles_per_image;
  // blockIdx -> tile is the identity: workgroups are dealt round-robin over the 8 XCDs, so at any
  // moment the resident workgroups of ALL XCDs write one compact, advancing window of the output.
  // The "XCD-aware" alternative (every XCD owns one contiguous band of tiles, so that its L2 holds
  // whole rows) was measured and is slower: neutral on 4:4:4, -3.5 % on 4:2:0 (write-heavy), -1 %
  // elsewhere -- nothing is re-read, so there is no L2 locality to win, and eight separate write
  // windows cost HBM page locality (tools/probe_store2.hip: the same 403 MB written by one
  // advancing window reach 6.4 TB/s, by many separate streams 5.2 TB/s).
  // No division here: tile / tiles_per_image, rem / tiles_per_row and m0 / mcus_x are each one multiply-high and one
  // shift by a pair the launch computed (jb_divmagic.h; exact for every tile < 2^31).  A 32-bit division is a float
  // reciprocal, a trip through a VGPR and some 25 dependent scalar instructions, and two of them stood between the
  // kernel arguments' arrival and every wave's first load.
  const int img = (int)jb_div_apply((uint32_t)tile, p.div_tiles_per_image);
  const int rem = tile - img * tiles_per_image;
  // Two tilings.  Linear (p.linear, the default): a tile is 192/NB consecutive MCUs of the image's
  // MCU stream, whatever MCU rows they fall in -- every tile but the image's last is full for any
  // image width.  Row-bound: a tile is a run of MCUs of ONE MCU row (the last run of a row may be
  // short); used where it leaves no tile ragged, and for very narrow images.
  // the rectangle, its first MCU, its tiles per row, and where and how wide its output is: this image's row of the
  // table (ROI = 2) or the launch's (ROI = 1: read from p where they are used, as that stage always has)
  [[maybe_unused]] JbCrop crop = {};
  int tiles_per_row = p.tiles_per_row;
  if constexpr (ROI == 2) {
    crop = crops_of(table...)[img];
    if (rem >= crop.n_tiles) return;  // (workgroup-uniform, before the first load and the first barrier)
    tiles_per_row = crop.tiles_per_row;
  }
  const auto roi_x = [&] { if constexpr (ROI == 2) return crop.x; else return p.roi_x; };
  const auto roi_y = [&] { if constexpr (ROI == 2) return crop.y; else return p.roi_y; };
  const auto roi_w = [&] { if constexpr (ROI == 2) return crop.w; else return p.roi_w; };
  const auto roi_h = [&] { if constexpr (ROI == 2) return crop.h; else return p.roi_h; };
  const auto roi_mx = [&] { if constexpr (ROI == 2) return crop.mx; else return p.roi_mx; };
  const auto roi_my = [&] { if constexpr (ROI == 2) return crop.my; else return p.roi_my; };
  // the output rows' stride and the image's place: tight rows at the table's offset, or the launch's strides
  const auto roi_row_stride = [&] { if constexpr (ROI == 2) return 3LL * crop.w; else return p.rgb_row_stride; };
  int my, mx0, nvalid;
  if (LINEAR) {
    const int m0 = rem * MCUS;
    my = (int)jb_div_apply((uint32_t)m0, p.div_mcus_x);
    mx0 = m0 - my * p.mcus_x;
    nvalid = FLAT ? MCUS : min(MCUS, p.mcus_x * p.mcus_y - m0);  // (FLAT: every tile is full, that is what the launch checked)
  } else {
    // (ROI = 2: the divisor is the image's own, read from its row of the table, which has no room for a pair: those
    // instantiations keep this one division)
    if constexpr (ROI == 2) my = rem / tiles_per_row;
    else my = (int)jb_div_apply((uint32_t)rem, p.div_tiles_per_row);
    mx0 = (rem - my * tiles_per_row) * MCUS;
    // region of interest: the tile grid's origin is the MCU that holds the rectangle's first pixel; the coefficient
    // address below keeps the full image's mcus_x as its row pitch
    if constexpr (ROI != 0) my += roi_my(), mx0 += roi_mx();
    nvalid = FLAT ? MCUS : min(MCUS, p.mcus_x - mx0);
  }
  const int last_block = nvalid * NB - 1;
  const uint8_t *tile_coef = (const uint8_t *)p.coef + (int64_t)img * p.coef_image_stride +
                             ((int64_t)my * p.mcus_x + mx0) * (NB * 128);
  const q_const_t *qsrc = (const q_const_t *)((const uint8_t *)p.qtabs + (int64_t)img * p.qtab_image_stride);

  // ---- stage 2: this lane's block -> registers ----
  const int comp_a = LM::comp(wave * 64);       // first lane's component (wave-uniform)
  const int comp_b = LM::comp(wave * 64 + 63);  // last lane's component
  const q_const_t *qa = qsrc + comp_a * 64;
  const q_const_t *qb = qsrc + comp_b * 64;
  float v[64];
  {
    // ---- stage 1: this lane's block (128 contiguous bytes) -> 32 VGPRs.  Default: straight from
    // HBM with 8 dwordx4 loads.  Every lane of a wave-instruction touches a different 128-B line,
    // but the 8 instructions of the wave consume those 64 lines completely: measured 6.4-6.5 TB/s
    // on MI355X (tools/probe_load.hip), the same as perfectly coalesced loads.
    uint32_t raw[32];  // row k = dwords 4k..4k+3, two int16 (columns 2j, 2j+1) per dword
    [[maybe_unused]] i32x16_t qw[4] = {};  // LDS-DMA path: the wave's table, 16 entries each
    if (kDirectLoad) {
      const int n = min(LM::block(tid), last_block);  // ragged tile: re-read its last block
      const u32x4_t *src = (const u32x4_t *)(tile_coef + (uint32_t)n * 128u);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        u32x4_t t = {0, 0, 0, 0};
        if (JB_DO_LOAD(p)) t = src[j];  // default cache policy: the line is re-used by the next 7 loads
        raw[j * 4 + 0] = t.x;
        raw[j * 4 + 1] = t.y;
        raw[j * 4 + 2] = t.z;
        raw[j * 4 + 3] = t.w;
      }
    } else {
      // 4:4:4 only (measured 4 % faster there than the direct loads): LDS-DMA
      // (global_load_lds_dwordx4: no VGPRs, 1 KiB per wave-instruction, every 8 lanes fetch one
      // whole 128-B line).  Wave w = component w fetches exactly the 64 blocks its own lanes
      // consume into its own 8 KiB of LDS -- the same 8 KiB its strip occupies later -- so neither
      // the load nor the hand-over to the strips needs a workgroup barrier.  Chunk j of the block
      // of lane l lands at chunk position j ^ ((l>>1)&7) (applied to the per-lane GLOBAL address,
      // LDS-DMA writes LDS linearly), which makes the 128-B-strided ds_read_b128 conflict free.
      char *const wave_lds = lds + wave * 8192;
      if (JB_DO_LOAD(p)) {
        if constexpr (FLAT) {
          // (issued at the kernel's start)
        } else if (nvalid == MCUS) {
          // A full tile (wave-uniform; every tile of a 4096- or 8192-pixel row): nothing to clamp
          load_full_tile_444(tile_coef + wave * 128, wave_lds, lane);
          // (ends this path with a statement the other one does not have: hipcc otherwise merges the two paths' eighth
          // loads into one behind the join, addressed through a 64-bit lane pointer, behind the table's address arithmetic)
          asm volatile("");
        } else {
          // the ragged tile (the last of a row whose MCUs are no multiple of 64): blocks past the last are re-reads of it
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const int l2 = i * 8 + (lane >> 3);  // the lane whose block this chunk belongs to
            const int f2 = (l2 >> 1) & 7;
            const int nsrc = min(LM::block(wave * 64 + l2), last_block);
            const uint32_t off = (uint32_t)nsrc * 128u + (uint32_t)(((lane & 7) ^ f2) << 4);
            __builtin_amdgcn_global_load_lds((gbl_void_t *)(tile_coef + off), (lds_void_t *)(wave_lds + i * 1024), 16, 0, JB_LOAD_AUX);
          }
        }
      }
      // chunk j of this lane's block is at chunk position j ^ f: one lane address, and a constant under the XOR per read
      const int f = (lane >> 1) & 7;
      const int lane_base = wave * 8192 + lane * 128 + (f << 4);
      // The wave's table (4:4:4: one component per wave, so MIXQ and comp_b never matter here) is fetched while the
      // coefficients are on their way, and is in SGPRs when the wait for the coefficients ends: the wait statement takes
      // it as operands, so the four scalar loads cannot sink below it.  Left to itself hipcc issues them behind the
      // ds_reads' wait and waits for them in full before the first multiply -- a scalar-memory round trip on every
      // wave's critical path.
#pragma unroll
      for (int t = 0; t < 4; t++) qw[t] = *(const q16_const_t *)(qa + 16 * t);
      asm volatile("s_waitcnt vmcnt(0)" : "+s"(qw[0]), "+s"(qw[1]), "+s"(qw[2]), "+s"(qw[3]) : : "memory");
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint4 t = *(const uint4 *)(lds + (lane_base ^ (j << 4)));
        raw[j * 4 + 0] = t.x;
        raw[j * 4 + 1] = t.y;
        raw[j * 4 + 2] = t.z;
        raw[j * 4 + 3] = t.w;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // dequantise (jpeg.cpp:563-569): int32 product, int->float on first use (jpeg.cpp:598)
    constexpr bool kUniformWaves = (NYT % 64 == 0) && (MCUS % 64 == 0);  // 4:4:4: one component per wave
    // p.chroma_q_equal: Cb and Cr name the same table (the usual case), so a wave that mixes
    // Cb and Cr blocks is still uniform as far as dequantisation goes
    if (!MIXQ || kUniformWaves || comp_a == comp_b || (p.chroma_q_equal && comp_a != 0)) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int e = k * 8 + i;
          const int q = kDirectLoad ? qa[e] : qw[e >> 4][e & 15];
          v[e] = dequant1(raw[k * 4 + (i >> 1)], i, q);
        }
      }
    } else {
      const bool second = LM::comp(tid) == comp_b;
#pragma unroll
      for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          // both entries through scalar loads, then a per-lane select (v_cndmask)
          const int q0 = __builtin_amdgcn_readfirstlane(qa[k * 8 + i]);
          const int q1 = __builtin_amdgcn_readfirstlane(qb[k * 8 + i]);
          v[k * 8 + i] = dequant1(raw[k * 4 + (i >> 1)], i, second ? q1 : q0);
        }
      }
    }
  }
  if (JB_DO_IDCT(p)) {
  // 4:2:0: a chroma block is needed as rows {0,1,4,5} in the first colour phase and {2,3,6,7} in
  // the second (chroma row r covers luma rows 2r, 2r+1), a luma block as rows 0-3 / 4-7.  The
  // chroma wave therefore stores column-pass output row k in register row sigma(k), sigma =
  // (0 1 4 5 2 3 6 7), so that for every lane "register rows 0-3" is what phase 0 consumes and
  // only 32 registers have to wait for phase 1.  (Row passes do not care which row they hold.)
  if (kPermChroma && comp_a != 0) {
#pragma unroll
    for (int i = 0; i < 8; i++)  // column pass, jpeg.cpp:596-663, outputs permuted by sigma
      aan_1d_io(v[0 * 8 + i], v[1 * 8 + i], v[2 * 8 + i], v[3 * 8 + i], v[4 * 8 + i], v[5 * 8 + i],
                v[6 * 8 + i], v[7 * 8 + i],  //
                v[0 * 8 + i], v[1 * 8 + i], v[4 * 8 + i], v[5 * 8 + i], v[2 * 8 + i], v[3 * 8 + i],
                v[6 * 8 + i], v[7 * 8 + i]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++)  // column pass, jpeg.cpp:596-663
      aan_1d(v[0 * 8 + i], v[1 * 8 + i], v[2 * 8 + i], v[3 * 8 + i], v[4 * 8 + i], v[5 * 8 + i],
             v[6 * 8 + i], v[7 * 8 + i]);
  }
#pragma unroll
  for (int k = 0; k < 8; k++)  // row pass, jpeg.cpp:664-731
    aan_1d(v[k * 8 + 0], v[k * 8 + 1], v[k * 8 + 2], v[k * 8 + 3], v[k * 8 + 4], v[k * 8 + 5],
           v[k * 8 + 6], v[k * 8 + 7]);
  }

  // ---- stage 3: two phases (upper / lower half of the tile's pixel rows) ----
  // Where this lane's block lands in the strips.  VS == 1: every block contributes rows
  // 4*phase..4*phase+3.  VS == 2: luma blocks of block-row bv contribute all 8 rows in phase
  // bv; chroma blocks contribute rows 4*phase..4*phase+3 (chroma row r covers luma rows 2r, 2r+1).
  // A strip row is a sequence of 16-B chunks (4 samples); chunk c is stored at position
  // c ^ ((c>>3)&1) so that the 8 lanes of a ds_write_b128 group hit 8 different bank quads.
  // (everything per-lane here is derived from an opaque copy of the thread id, so that it is
  // materialised after the IDCT instead of occupying registers across it)
  int tid_late = tid;
  asm volatile("" : "+v"(tid_late));
  const int comp_l = LM::comp(tid_late), mcu_l = LM::mcu(tid_late), slot_l = LM::slot(tid_late);
  const int bv = comp_l == 0 ? slot_l / HS : 0;
  const int bh = comp_l == 0 ? slot_l - bv * HS : 0;
  const int pitch = comp_l == 0 ? (YW * 4) : CW * 4;
  const int blk_col = comp_l == 0 ? mcu_l * HS + bh : mcu_l;  // 8-sample column of the block in its strip
  const int sw = (blk_col >> 2) & 1;
  const int luma_off = bv * 4 * (YW * 4) + blk_col * 32;
  char *const dst = lds + (comp_l == 0 ? luma_off : (comp_l == 1 ? CB_OFF : CR_OFF) + blk_col * 32);
  char *const dst_lo = dst + sw * 16;        // samples 0..3 of a row
  char *const dst_hi = dst + (sw ^ 1) * 16;  // samples 4..7

  constexpr int TASKS_PER_ROW = YW / 4;
  constexpr int TASKS = YROWS * TASKS_PER_ROW;
  static_assert(TASKS % 64 == 0, "whole wave-iterations");
  static_assert(TASKS_PER_ROW % 64 == 0, "a wave-iteration stays within one strip row");
  uint8_t *const img_rgb = p.rgb + (ROI == 2 ? crop.tmp_offset : (int64_t)img * p.rgb_image_stride);
  // loop-invariant lane offsets of the colour stage (row-uniform layouts): the lane's 16-B luma
  // chunk within a 64-chunk segment and its chroma chunk, both with the strip swizzle applied
  // (the swizzle bit is bit 3 of the chunk index, which the segment number does not touch)
  // (computed from an opaque copy of the lane id so they are materialised here, after the IDCT,
  // instead of being kept in registers across it)
  const int lane_late = tid_late & 63;
  const int lane_y_off = (lane_late ^ ((lane_late >> 3) & 1)) * 16;
  const int lane_c_off = HS == 1 ? lane_y_off : (((lane_late >> 1) ^ ((lane_late >> 4) & 1)) * 16 + (lane_late & 1) * 8);
  // scaled: strip rows a lane sums per wave-iteration, wave-iterations per phase and per wave; SCALE = 8 carries
  // the sums of its boxes' upper halves (phase 0) to phase 1 in kSJ x 3 registers
  constexpr int kSR = SCALE < 4 ? SCALE : 4;
  constexpr int kSIT = (YROWS / kSR) * (TASKS_PER_ROW / 64);
  constexpr int kSJ = (kSIT + kTileBlocks / 64 - 1) / (kTileBlocks / 64);
  uint32_t acc8[kSJ][3] = {};

#pragma unroll
  for (int phase = 0; phase < 2; phase++) {
    if (phase == 1) lds_barrier();  // phase-0 colour reads are done: the strips may be rewritten
    // Every lane contributes rows 4*phase..4*phase+3 of its block (so half of every block is
    // consumed per phase and only 32 values wait in registers).  Luma block-row bv lands in
    // strip rows 4*bv..4*bv+3 (VS == 2: the strip holds image rows 4p..4p+3 and 8+4p..8+4p+3);
    // a chroma block contributes the chroma rows those luma rows need: row/VS of each, i.e.
    // rows 2p, 2p+1, 4+2p, 5+2p for VS == 2 (reference jpeg.cpp:518-520).
    static_assert(VS == 1 || kPermChroma, "luma and chroma lanes take the same register rows per phase");
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      const int k = phase * 4 + kk;
      *(float4 *)(dst_lo + kk * pitch) = make_float4(v[k * 8 + 0], v[k * 8 + 1], v[k * 8 + 2], v[k * 8 + 3]);
      *(float4 *)(dst_hi + kk * pitch) = make_float4(v[k * 8 + 4], v[k * 8 + 5], v[k * 8 + 6], v[k * 8 + 7]);
    }
    lds_barrier();

    if constexpr (STAGED) {
      // ---- staged: pack into LDS, then write line-aligned ----
      // Pass A.  One wave takes a whole strip row, segment after segment: the 12 packed bytes of a lane go back
      // into the row's own luma strip at segment * 768 + lane * 12 -- at or below every byte the wave has still to
      // read, and no other wave touches this row -- so the row ends up as npixels * 3 contiguous output bytes.
      constexpr int IPR = TASKS_PER_ROW / 64;
      for (int row = wave; row < YROWS; row += kTileBlocks / 64) {
        char *const rowp = lds + row * (YW * 4);
#pragma unroll
        for (int seg = 0; seg < IPR; seg++) {
          const float4 Y = *(const float4 *)(rowp + lane_y_off + seg * 1024);
          float cb[4], cr[4];
          const int coff = (row / VS) * (CW * 4) + seg * (1024 / HS);
          load_chroma4<HS>(lds + CB_OFF + lane_c_off + coff, lds + CR_OFF + lane_c_off + coff, cb, cr);
          const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
          float r[4], g[4], b[4];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            ycc_px(yy[i], cb[i], cr[i], r[i], g[i], b[i]);
          }
          uint32_t w0, w1, w2;
          pack12_rtz(r, g, b, w0, w1, w2);
          asm volatile("" ::: "memory");  // (the reads of this segment stay in front of its writes, the writes in front of the next reads)
          uint32_t *const o = (uint32_t *)(rowp + seg * 768 + lane_late * 12);
          o[0] = w0, o[1] = w1, o[2] = w2;
          asm volatile("" ::: "memory");
        }
        // Pass B, by the same wave on the row it has just packed (so nothing but its own LDS traffic has to be waited
        // for).  A strip row is the pixels of the tile's MCUs, which lie in one image row per MCU row the tile
        // touches: each such piece is written as [bytes up to the first 64-byte line][whole 16-byte chunks from
        // there][the last bytes], the chunks fetched from LDS at whatever byte offset that takes.  Whole lines
        // wherever the piece covers them, whatever the row stride.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int y_in = phase * 4 + (row >> 2) * 8 + (row & 3);
        int m = 0, my_k = my, mx_k = mx0;
        while (m < nvalid) {
          const int cnt = min(nvalid - m, p.mcus_x - mx_k);
          const int y = my_k * 8 * VS + y_in, x0 = mx_k * 8 * HS;
          const int len = min(cnt * 8 * HS, p.width - x0) * 3;   // bytes of the piece inside the image
          if (y < p.height && len > 0) {
            uint8_t *const dstp = img_rgb + (int64_t)y * p.rgb_row_stride + (int64_t)x0 * 3;
            const int src = row * (YW * 4) + m * (8 * HS * 3);     // LDS byte offset of the piece (a multiple of 8)
            const int head = min(len, (int)((64 - ((uintptr_t)dstp & 63)) & 63));
            const int nbody = (len - head) >> 4;
            const int tail = len - head - nbody * 16;
            if (lane_late < head) dstp[lane_late] = (uint8_t)lds[src + lane_late];
            if (lane_late < tail) dstp[len - tail + lane_late] = (uint8_t)lds[src + len - tail + lane_late];
            // (gfx950 reads 16 bytes of LDS at any byte address in one ds_read_b128: unaligned DS access is on under ROCm)
            const char *const from = lds + src + head;
            u32x4_t *const lines = (u32x4_t *)(dstp + head);
            for (int c = lane_late; c < nbody; c += 64) {
              const u32x4_t v4 = *(const u32x4_u *)(from + c * 16);
              __builtin_nontemporal_store(v4, lines + c);
            }
          }
          m += cnt;
          mx_k = 0;
          my_k++;
        }
      }
    } else if constexpr (SCALE > 1) {
      // ---- scaled: area-reduced output, one lane = a column of 4 adjacent pixels ----
      // A wave-iteration takes kSR strip rows (2 for SCALE = 2, else 4) of one 256-pixel segment: every lane
      // computes the colour of its 4 pixels in each row exactly as the full-size stage does (the same LDS reads, the
      // same transform, the same pack12_rtz conversion to u8) and adds the u8 samples up per channel.  SCALE = 2 and 4
      // boxes lie inside one phase (4:2:0 / 4:4:0 strip rows 0-3 and 4-7 are two block rows): the lane owns 2 / 1
      // whole boxes and stores them.  SCALE = 8: a box is two lanes wide (x4 even + odd) and both phases high; the
      // lane keeps its phase-0 sums in acc8 and in phase 1 the even lane adds its neighbour's sums and stores.
      // Samples past the image (MCU padding, rows below the last) never enter a sum.  Stores are 3- or 6-byte buffer
      // stores at any byte address; the byte-store knob is not looked at here.
      constexpr int IPR = TASKS_PER_ROW / 64;
      constexpr int SEG_MCUS = 256 / (8 * HS);
      uint8_t *const out_img = p.rgb + (int64_t)img * p.rgb_image_stride;
#pragma unroll
      for (int j = 0; j < kSJ; j++) {
        const int it = wave + j * (kTileBlocks / 64);
        if (it >= kSIT) break;
        const int rg = it / IPR, seg = it - rg * IPR;
        const int r0 = rg * kSR;                                            // first strip row of the group
        const int y0 = my * 8 * VS + phase * 4 + (r0 >> 2) * 8 + (r0 & 3);  // its image row
        const int ybox = SCALE == 8 ? y0 - phase * 4 : y0;                  // first image row of the lane's boxes
        const int xseg = (mx0 + seg * SEG_MCUS) * 8 * HS;                   // image column of the segment
        if (ybox >= p.height || xseg >= p.width) continue;                  // (wave-uniform)
        const int x = xseg + lane_late * 4;                                 // the lane's first pixel
        const int npx = min(4, p.width - x);                                // its pixels inside the image (<= 0: none)
        const uint32_t keep = npx >= 4 ? 0xffffffffu : npx <= 0 ? 0u : (1u << (8 * npx)) - 1u;
        // per channel: SCALE = 2 two 16-bit sums (pixels 0+1 | 2+3), else one sum of the 4 pixels
        uint32_t s[3] = {0, 0, 0};
#pragma unroll
        for (int rr = 0; rr < kSR; rr++) {
          if (y0 + rr >= p.height) break;  // (wave-uniform)
          const int row = r0 + rr;
          const float4 Y = *(const float4 *)(lds + lane_y_off + row * (YW * 4) + seg * 1024);
          float cb[4], cr[4];
          const int coff = (row / VS) * (CW * 4) + seg * (1024 / HS);
          load_chroma4<HS>(lds + CB_OFF + lane_c_off + coff, lds + CR_OFF + lane_c_off + coff, cb, cr);
          const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
          float r[4], g[4], b[4];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            ycc_px(yy[i], cb[i], cr[i], r[i], g[i], b[i]);
          }
          // the full-size conversion with its operands permuted: pack12_rtz writes bytes in the order
          // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, so these arguments give one word per channel (pixels 0..3)
        uint32_t w[3];
        pack_channels(r, g, b, w);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const uint32_t v8 = w[c] & keep;
            if (SCALE == 2) s[c] += (v8 & 0x00ff00ffu) + ((v8 >> 8) & 0x00ff00ffu);
            else s[c] = __builtin_amdgcn_sad_u8(v8, 0u, s[c]);  // + the sum of the 4 bytes
          }
        }
        const int ny = min(SCALE, p.height - ybox);
        if constexpr (SCALE == 2) {
          const int nx0 = min(2, p.width - x), nx1 = min(2, p.width - x - 2);
          uint32_t o0[3], o1[3];
#pragma unroll
          for (int c = 0; c < 3; c++) o0[c] = box_mean<2>(s[c] & 0xffffu, nx0 * ny), o1[c] = box_mean<2>(s[c] >> 16, nx1 * ny);
          const __amdgpu_buffer_rsrc_t rsrc =
              __builtin_amdgcn_make_buffer_rsrc(out_img + (int64_t)(ybox >> 1) * p.rgb_row_stride, 0, 0x7ffffff0, 0x00020000);
          const int voff = (x >> 1) * 3;
          if (nx1 > 0) {
            __builtin_amdgcn_raw_buffer_store_b32(o0[0] | o0[1] << 8 | o0[2] << 16 | o1[0] << 24, rsrc, voff, 0, JB_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(o1[1] | o1[2] << 8), rsrc, voff + 4, 0, JB_STORE_AUX);
          } else if (nx0 > 0) {
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(o0[0] | o0[1] << 8), rsrc, voff, 0, JB_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)o0[2], rsrc, voff + 2, 0, JB_STORE_AUX);
          }
        } else {
          int nx = npx;
          if constexpr (SCALE == 8) {
#pragma unroll
            for (int c = 0; c < 3; c++) acc8[j][c] += s[c];
            if (phase == 0) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = acc8[j][c] + (uint32_t)__shfl_xor((int)acc8[j][c], 1);
            nx = min(8, p.width - x);
          }
          if ((SCALE == 4 || (lane_late & 1) == 0) && nx > 0) {
            uint32_t o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = box_mean<SCALE>(s[c], nx * ny);
            const __amdgpu_buffer_rsrc_t rsrc =
                __builtin_amdgcn_make_buffer_rsrc(out_img + (int64_t)(ybox / SCALE) * p.rgb_row_stride, 0, 0x7ffffff0, 0x00020000);
            const int voff = (x / SCALE) * 3;
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(o[0] | o[1] << 8), rsrc, voff, 0, JB_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)o[2], rsrc, voff + 2, 0, JB_STORE_AUX);
          }
        }
      }
    } else if constexpr (ROI != 0) {
      // ---- region of interest: the pixels of [roi_x, roi_x + roi_w) x [roi_y, roi_y + roi_h), in any format ----
      // The wave-iterations, LDS reads, colour transform and u8 conversion are those of the full-size stage (FORMAT = 0)
      // or of the planar one; what differs is which of them are stored, and where.  Strip rows above or below the
      // rectangle and segments left or right of it are skipped wave-uniformly.  Of a segment's 256 pixels the rectangle
      // holds [a, b): the descriptor is based at pixel a's place in the output row and ends behind the last whole 4-pixel
      // group, so its range check drops the lanes right of the rectangle; the lanes left of it (a negative offset from
      // that base) get an offset past any range instead of the wrapped one.  The at most two lanes whose group the
      // left or the right edge cuts (one lane for both when the rectangle starts and ends in one group) store their
      // 1-3 inside pixels one by one.  Nothing outside the rectangle is written.  The byte-store knob is not looked at.
      constexpr int IPR = TASKS_PER_ROW / 64;
      constexpr int SEG_MCUS = 256 / (8 * HS);
      constexpr int ES = FORMAT == 0 ? 3 : FORMAT == 1 ? 1 : FORMAT == 2 ? 4 : 2;  // bytes per pixel in a row (of a plane)
      const int rx1 = roi_x() + roi_w(), ry1 = roi_y() + roi_h();
      for (int it = wave; it < TASKS / 64; it += kTileBlocks / 64) {
        const int row = it / IPR, seg = it - row * IPR;
        const int y = my * 8 * VS + phase * 4 + (row >> 2) * 8 + (row & 3);  // image row of the strip row
        const int xseg = (mx0 + seg * SEG_MCUS) * 8 * HS;                    // image column of the segment
        if (y < roi_y() || y >= ry1 || xseg >= rx1 || xseg + 256 <= roi_x()) continue;  // (wave-uniform)
        const float4 Y = *(const float4 *)(lds + lane_y_off + row * (YW * 4) + seg * 1024);
        float cb[4], cr[4];
        const int coff = (row / VS) * (CW * 4) + seg * (1024 / HS);
        load_chroma4<HS>(lds + CB_OFF + lane_c_off + coff, lds + CR_OFF + lane_c_off + coff, cb, cr);
        const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
        float r[4], g[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ycc_px(yy[i], cb[i], cr[i], r[i], g[i], b[i]);
        }
        const int a = max(roi_x() - xseg, 0), e = min(rx1 - xseg, 256);  // segment pixels inside the rectangle: a < e
        const int nrec = max((e & ~3) - a, 0) * ES;                       // bytes up to the end of the last whole group
        uint8_t *const segp = img_rgb + (int64_t)(y - roi_y()) * roi_row_stride() + (int64_t)(xseg + a - roi_x()) * ES;
        const int rel = lane_late * 4 - a;                    // the lane's first pixel, relative to pixel a
        const int voff = rel >= 0 ? rel * ES : 0x40000000;    // (left of the rectangle: past any range, never wrapped)
        // the edge groups: rare, so their lane tests go through an opaque copy and nothing of them is hoisted
        const bool ragged = ((a | e) & 3) != 0;               // (wave-uniform)
        int l4 = lane_late * 4;
        if (ragged) asm volatile("" : "+v"(l4));
        const bool cut = ragged && l4 < e && l4 + 4 > a && !(l4 >= a && l4 + 4 <= e);
        if constexpr (FORMAT == 0) {
          uint32_t w0, w1, w2;
          pack12_rtz(r, g, b, w0, w1, w2);
          const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(segp, 0, nrec, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b96(u32x3_t{w0, w1, w2}, rsrc, voff, 0, JB_STORE_AUX);
          if (cut) {
            const __amdgpu_buffer_rsrc_t edge = __builtin_amdgcn_make_buffer_rsrc(segp, 0, (e - a) * ES, 0x00020000);
            // the 12 packed bytes are r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3: pixel i is bytes 3i .. 3i+2
            const uint32_t px[4] = {w0, w0 >> 24 | w1 << 8, w1 >> 16 | w2 << 16, w2 >> 8};
#pragma unroll
            for (int i = 0; i < 4; i++)
              if (l4 + i >= a && l4 + i < e) {
                __builtin_amdgcn_raw_buffer_store_b16((uint16_t)px[i], edge, (l4 + i - a) * 3, 0, JB_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(px[i] >> 16), edge, (l4 + i - a) * 3 + 2, 0, JB_STORE_AUX);
              }
          }
        } else {
          uint32_t w[3];
          pack_channels(r, g, b, w);  // w[c] = the u8 samples of channel c, pixels 0..3 (as the planar stage)
#pragma unroll
          for (int c = 0; c < 3; c++) {
            uint8_t *const planep = segp + (int64_t)c * p.rgb_plane_stride;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(planep, 0, nrec, 0x00020000);
            const __amdgpu_buffer_rsrc_t edge = __builtin_amdgcn_make_buffer_rsrc(planep, 0, (e - a) * ES, 0x00020000);
            if constexpr (FORMAT == 1) {
              __builtin_amdgcn_raw_buffer_store_b32(w[c], rsrc, voff, 0, JB_STORE_AUX);
              if (cut) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                  if (l4 + i >= a && l4 + i < e)
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w[c] >> (8 * i)), edge, l4 + i - a, 0, JB_STORE_AUX);
              }
            } else {
              const float sc = p.scale[c], bi = p.bias[c];
              float f[4];
#pragma unroll
              for (int i = 0; i < 4; i++) f[i] = (float)((w[c] >> (8 * i)) & 0xffu) * sc + bi;
              if constexpr (FORMAT == 2) {
                const uint32_t u[4] = {__builtin_bit_cast(uint32_t, f[0]), __builtin_bit_cast(uint32_t, f[1]),
                                       __builtin_bit_cast(uint32_t, f[2]), __builtin_bit_cast(uint32_t, f[3])};
                __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{u[0], u[1], u[2], u[3]}, rsrc, voff, 0, JB_STORE_AUX);
                if (cut) {
#pragma unroll
                  for (int i = 0; i < 4; i++)
                    if (l4 + i >= a && l4 + i < e) __builtin_amdgcn_raw_buffer_store_b32(u[i], edge, (l4 + i - a) * 4, 0, JB_STORE_AUX);
                }
              } else {
                // (_Float16)x is v_cvt_f16_f32: round to nearest even (never the packed round-toward-zero conversion)
                uint32_t h[4];
#pragma unroll
                for (int i = 0; i < 4; i++) h[i] = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f[i]);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{h[0] | h[1] << 16, h[2] | h[3] << 16}, rsrc, voff, 0, JB_STORE_AUX);
                if (cut) {
#pragma unroll
                  for (int i = 0; i < 4; i++)
                    if (l4 + i >= a && l4 + i < e) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)h[i], edge, (l4 + i - a) * 2, 0, JB_STORE_AUX);
                }
              }
            }
          }
        }
      }
    } else if constexpr (FORMAT > 0) {
      // ---- planar: three planes R, G, B of u8 / f32 / f16, one lane = 4 adjacent pixels of one row ----
      // The wave-iterations are those of the full-size row-bound stage below: one strip row of one 256-pixel segment,
      // the same LDS reads and colour transform.  pack12_rtz with its operands permuted (as the scaled stage calls it)
      // gives ONE word per channel -- the four u8 samples of R, of G, of B, truncated and clamped exactly as FORMAT = 0
      // stores them -- so a lane stores 4 bytes per plane, or widens them: v_cvt_f32_ubyte0..3 (exact), one f32
      // multiply, one f32 add (separate instructions: this file is built with -ffp-contract=off), for f16 one
      // v_cvt_f16_f32.  All of these consume pack12_rtz's outputs, so they issue after it has switched the wave's
      // rounding mode back to nearest-even.  A wave-instruction writes 256 / 1024 / 512 contiguous bytes of one plane
      // row; the descriptor's range check drops the lanes past the right edge, and the one lane whose group straddles
      // it (width % 4 != 0) stores its 1-3 elements with one or two narrower stores.
      constexpr int IPR = TASKS_PER_ROW / 64;
      constexpr int SEG_MCUS = 256 / (8 * HS);
      constexpr int ES = FORMAT == 1 ? 1 : FORMAT == 2 ? 4 : 2;  // bytes per element
      for (int it = wave; it < TASKS / 64; it += kTileBlocks / 64) {
        const int row = it / IPR, seg = it - row * IPR;
        const int y = my * 8 * VS + phase * 4 + (row >> 2) * 8 + (row & 3);  // image row of the strip row
        const int xseg = (mx0 + seg * SEG_MCUS) * 8 * HS;                    // image column of the segment
        if (y >= p.height || xseg >= p.width) continue;                      // (wave-uniform; covers MCUs past nvalid)
        const float4 Y = *(const float4 *)(lds + lane_y_off + row * (YW * 4) + seg * 1024);
        float cb[4], cr[4];
        const int coff = (row / VS) * (CW * 4) + seg * (1024 / HS);
        load_chroma4<HS>(lds + CB_OFF + lane_c_off + coff, lds + CR_OFF + lane_c_off + coff, cb, cr);
        const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
        float r[4], g[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ycc_px(yy[i], cb[i], cr[i], r[i], g[i], b[i]);
        }
        // byte order of pack12_rtz: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 -> with these arguments w[c] = channel c, pixels 0..3
        uint32_t w[3];
        pack_channels(r, g, b, w);
        const int npx = min(256, p.width - xseg);    // pixels of the segment inside the image (wave-uniform)
        const int whole = npx >> 2, part = npx & 3;  // whole 4-pixel groups; pixels of the group that straddles the edge
        uint8_t *const segp = img_rgb + (int64_t)y * p.rgb_row_stride + (int64_t)xseg * ES;
        const int voff = lane_late * (4 * ES);
        const bool edge = part != 0 && lane_late == whole;
        const int voff2 = voff + (part == 3 ? 2 * ES : 0);  // where the edge group's odd element goes
#pragma unroll
        for (int c = 0; c < 3; c++) {
          uint8_t *const planep = segp + (int64_t)c * p.rgb_plane_stride;
          const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(planep, 0, whole * (4 * ES), 0x00020000);
          const __amdgpu_buffer_rsrc_t tail = __builtin_amdgcn_make_buffer_rsrc(planep, 0, 0x7ffffff0, 0x00020000);
          if constexpr (FORMAT == 1) {
            __builtin_amdgcn_raw_buffer_store_b32(w[c], rsrc, voff, 0, JB_STORE_AUX);
            if (edge) {
              if (part >= 2) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)w[c], tail, voff, 0, JB_STORE_AUX);
              if (part != 2) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(part == 3 ? w[c] >> 16 : w[c]), tail, voff2, 0, JB_STORE_AUX);
            }
          } else {
            const float sc = p.scale[c], bi = p.bias[c];
            float f[4];
#pragma unroll
            for (int i = 0; i < 4; i++) f[i] = (float)((w[c] >> (8 * i)) & 0xffu) * sc + bi;
            if constexpr (FORMAT == 2) {
              const uint32_t u[4] = {__builtin_bit_cast(uint32_t, f[0]), __builtin_bit_cast(uint32_t, f[1]),
                                     __builtin_bit_cast(uint32_t, f[2]), __builtin_bit_cast(uint32_t, f[3])};
              __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{u[0], u[1], u[2], u[3]}, rsrc, voff, 0, JB_STORE_AUX);
              if (edge) {
                if (part >= 2) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{u[0], u[1]}, tail, voff, 0, JB_STORE_AUX);
                if (part != 2) __builtin_amdgcn_raw_buffer_store_b32(part == 3 ? u[2] : u[0], tail, voff2, 0, JB_STORE_AUX);
              }
            } else {
              // (_Float16)x is v_cvt_f16_f32: round to nearest even (never the packed round-toward-zero conversion)
              uint32_t h[4];
#pragma unroll
              for (int i = 0; i < 4; i++) h[i] = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f[i]);
              const uint32_t h01 = h[0] | h[1] << 16, h23 = h[2] | h[3] << 16;
              __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{h01, h23}, rsrc, voff, 0, JB_STORE_AUX);
              if (edge) {
                if (part >= 2) __builtin_amdgcn_raw_buffer_store_b32(h01, tail, voff, 0, JB_STORE_AUX);
                if (part != 2) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(part == 3 ? h[2] : h[0]), tail, voff2, 0, JB_STORE_AUX);
              }
            }
          }
        }
      }
    } else
    // colour transform + store: one lane = 4 adjacent pixels of one row, one wave-iteration =
    // 256 adjacent pixels (768 contiguous output bytes)
    // image row of strip row sr: block-row sr/4, row 4*phase + sr%4 within the block
    for (int it = wave; it < TASKS / 64; it += kTileBlocks / 64) {
      {
        // Everything but the data is wave-uniform here: the row, the 256-pixel segment of the row,
        // the output address (a buffer descriptor per segment; lanes address it with the loop-
        // invariant offset lane*12 and the hardware range check drops lanes past the image edge).
        constexpr int IPR = TASKS_PER_ROW / 64;  // wave-iterations per strip row
        const int row = it / IPR, seg = it - row * IPR;
        // where the segment's 256 pixels (SEG_MCUS MCUs) go: MCU row my_s from MCU column mx_s on;
        // in the linear tiling the segment may run past the end of the MCU row and continue at
        // the start of the next one (at most once: the host only selects the linear tiling when
        // an MCU row holds at least one whole segment)
        constexpr int SEG_MCUS = 256 / (8 * HS);
        const int seg_valid = min(SEG_MCUS, nvalid - seg * SEG_MCUS);  // MCUs of the segment that exist
        if (seg_valid <= 0) continue;
        int my_s = my, mx_s = mx0 + seg * SEG_MCUS;
        if (LINEAR)
          while (mx_s >= p.mcus_x) {
            mx_s -= p.mcus_x;
            my_s++;
          }
        const int n_row = min(seg_valid, p.mcus_x - mx_s);  // MCUs before the wrap
        const int y_in = phase * 4 + (row >> 2) * 8 + (row & 3);  // pixel row within the MCU row
        if (!LINEAR && (my * 8 * VS + y_in >= p.height || mx_s * 8 * HS >= p.width)) continue;
        const float4 Y = *(const float4 *)(lds + lane_y_off + row * (YW * 4) + seg * 1024);
        float cb[4], cr[4];
        // chroma sample of luma pixel (row, col): (row/VS, col/HS) -- reference jpeg.cpp:518-520
        const int coff = (row / VS) * (CW * 4) + seg * (1024 / HS);
        load_chroma4<HS>(lds + CB_OFF + lane_c_off + coff, lds + CR_OFF + lane_c_off + coff, cb, cr);
        const float yy[4] = {Y.x, Y.y, Y.z, Y.w};
        float r[4], g[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if (JB_DO_COLOUR(p)) {
            ycc_px(yy[i], cb[i], cr[i], r[i], g[i], b[i]);
          } else {
            r[i] = yy[i], g[i] = cb[i], b[i] = cr[i];
          }
        }
        if (!JB_DO_STORE(p)) continue;
        uint32_t w0 = 0, w1 = 0, w2 = 0;
        // part 0: the MCUs before the wrap; part 1 (linear tiling only): the rest, one MCU row down
#pragma unroll
        for (int part = 0; part < (LINEAR ? 2 : 1); part++) {
          const int px0 = part == 0 ? 0 : n_row * 8 * HS;  // first segment pixel of the part
          const int y = (my_s + part) * 8 * VS + y_in;
          const int x0 = part == 0 ? mx_s * 8 * HS : 0;     // image column of that pixel
          const int npx = min((part == 0 ? n_row : seg_valid - n_row) * 8 * HS, p.width - x0);
          if (npx > 0 && y < p.height) {
            uint8_t *const segp = img_rgb + (int64_t)y * p.rgb_row_stride + (int64_t)x0 * 3;  // address of pixel px0
            const int rel = lane_late * 4 - px0;  // this lane's first pixel relative to the part
            if (p.fast_store && (part == 0 || rel >= 0)) {
              // whole 4-pixel groups through one 12-byte store per lane; the descriptor's range
              // check drops the lanes past the part's end
              pack12_rtz(r, g, b, w0, w1, w2);  // (again for the rare second part: cheaper than keeping it live)
              const int voff = LINEAR ? rel * 3 : lane_late * 12;
              const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(segp, 0, (npx >> 2) * 12, 0x00020000);
              __builtin_amdgcn_raw_buffer_store_b96(u32x3_t{w0, w1, w2}, rsrc, voff, 0, JB_STORE_AUX);
              if (kTwoStoreTail && (npx & 3)) {
                // the one group that straddles the right edge: its lane holds the 12 packed bytes and
                // stores the 3, 6 or 9 inside the image with two stores (nine byte stores, each a
                // wave-wide instruction, cost the odd-width bundled-image size 5 points of roofline)
                // (the scalar offset carries the +2 / +4 / +8, and the lane test goes through an opaque
                // copy: nothing of this rare path is hoisted into registers that live across the IDCT)
                const __amdgpu_buffer_rsrc_t tail = __builtin_amdgcn_make_buffer_rsrc(segp, 0, 0x7ffffff0, 0x00020000);
                int tv = voff;
                asm volatile("" : "+v"(tv));
                if (tv == (npx >> 2) * 12) {
                  const int t = npx & 3;
                  if (t == 3) {
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{w0, w1}, tail, tv, 0, JB_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)w2, tail, tv, 8, JB_STORE_AUX);
                  } else if (t == 2) {
                    __builtin_amdgcn_raw_buffer_store_b32(w0, tail, tv, 0, JB_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)w1, tail, tv, 4, JB_STORE_AUX);
                  } else {
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)w0, tail, tv, 0, JB_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w0 >> 16), tail, tv, 2, JB_STORE_AUX);
                  }
                }
              }
            }
            if (!p.fast_store || (!kTwoStoreTail && (npx & 3))) {
              // the byte-store knob (JPEGBLK_BYTE_STORE=1): every pixel through byte stores; and the
              // straddling group of the instantiations without the two-store tail
              const int first = p.fast_store ? (npx & ~3) : 0;
              // opaque copy of a value that is live anyway: keeps this rare path's address
              // arithmetic from being hoisted out of the loop into registers
              int tail_src = LINEAR ? rel : lane_late;
              asm volatile("" : "+v"(tail_src));
#pragma unroll
              for (int i = 0; i < 4; i++) {
                const int px = (LINEAR ? tail_src : tail_src * 4) + i;
                if (px >= first && px < npx) store_px_bytes(segp + px * 3, r[i], g[i], b[i]);
              }
            }
          }
          if (!LINEAR || n_row >= seg_valid) break;  // no second part
        }
      }
    }
  }
