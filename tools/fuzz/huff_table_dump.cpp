// huff_table_dump -- the device entropy decoder's lookup tables for a set of canonical Huffman tables, built by
// jb_huff_fill_table_ exactly as jb_huff_prepare_ builds them (one set, the tables in the given order, one pool of
// second-level tables), and written out for tests/test_huff_tables_cpu.py to check every 16-bit window against a
// decoder of its own.  A stand-alone program, built with ASan + UBSan (tools/fuzz/Makefile): the set lives in an
// exactly-sized heap block, so a second-level table beyond the pool is a report, not a silent write.
//   huff_table_dump in.bin out.bin
// in:  u8 n (1..6), then n x { u8 is_ac, u8 BITS[16], u8 count, u8 HUFFVAL[count] }
// out: u32 n, u32 second-level tables used, i32 index of the table the pool refused (-1: none),
//      u16 t1[n][1024], u16 t2[24][64]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <string>

#include "../../include/jpegblk.h"
#include "../../jpeg_decoder_amd/csrc/jb_internal.h"

// ---- stubs for the parts of the library that need a device (as in fuzz_frontend.cpp; none is called here) ----
static std::string g_err;
int jb_fail_(jb_ctx *, int code, const char *msg) {
  g_err = msg ? msg : "";
  return code;
}
void jb_ctx_set_last_desc_(jb_ctx *, const jb_image_desc *) {}
const JbKnobs *jb_ctx_knobs_(const jb_ctx *) {
  static const JbKnobs k;
  return &k;
}
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

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: huff_table_dump in.bin out.bin\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in(1 << 16);
  in.resize(fread(in.data(), 1, in.size(), f));
  fclose(f);
  size_t at = 0;
  auto need = [&](size_t n) {
    if (at + n > in.size()) {
      fprintf(stderr, "huff_table_dump: input ends early\n");
      exit(2);
    }
  };
  need(1);
  const uint32_t n = in[at++];
  if (n < 1 || n > kJbMaxTabs) return 2;
  JbHuffTables *set = (JbHuffTables *)malloc(sizeof(JbHuffTables));
  memset(set, 0, sizeof *set);
  uint32_t n_t2 = 0;
  int32_t refused = -1;
  for (uint32_t t = 0; t < n && refused < 0; t++) {
    need(18);
    const bool is_ac = in[at++] != 0;
    uint8_t counts[17] = {0};
    memcpy(counts + 1, &in[at], 16);
    at += 16;
    const size_t n_sym = in[at++];
    need(n_sym);
    size_t sum = 0;
    for (int l = 1; l <= 16; l++) sum += counts[l];
    if (sum != n_sym) return 2;
    std::vector<uint8_t> symbols(in.begin() + (long)at, in.begin() + (long)(at + n_sym));  // (exactly sized)
    at += n_sym;
    if (!jb_huff_fill_table_(counts, symbols.data(), is_ac, set, t, n, &n_t2)) refused = (int32_t)t;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(&n, 4, 1, f);
  fwrite(&n_t2, 4, 1, f);
  fwrite(&refused, 4, 1, f);
  fwrite(set->t1, sizeof set->t1[0], n, f);
  fwrite(set->t2, sizeof set->t2, 1, f);
  fclose(f);
  free(set);
  return 0;
}
