// jb_frontend.cpp -- host front end: the baseline rules of the JFIF marker parser, the baseline Huffman decoder, the
// host half of the device entropy decoder (jb_huff_prepare_) and the jb_decode_memory* / jb_decode_file* entry points.
//
// This is the part of the reference that STAYS on the host (reference jpeg.cpp:67-446 and
// 826-907, include/file.hpp, include/huffman.hpp).  It produces exactly what the reference's
// decodeHuffman() produces (jpeg.cpp:405-446): de-zigzagged integer coefficient blocks in
// MCU-interleaved scan order -- here packed as int16 straight into a caller buffer (pinned
// memory when it comes from jb_pinned_alloc) that is handed to the device seam.
//
// Written table-driven (9-bit lookahead + canonical fallback, 64-bit bit buffer) instead of
// the reference's bit-at-a-time linear code search (jpeg.cpp:300-320) and its per-byte heap
// allocation (file.hpp:26-52); the decoded integers are identical.
//
// The marker walk, the header it fills and the DQT / DHT / DRI segments are jb_markers.h's, shared with the general rules
// (jb_frontend_ext.cpp).  The rules of this file are the fast path for what the reference accepts: baseline SOF0
// (jpeg.cpp:69-73), exactly 3 components (jpeg.cpp:83-87), luma factors in {1,2}, chroma 1x1 (jpeg.cpp:110-136),
// table ids 0..3, one scan with Ss=0, Se=63, Ah=Al=0 (jpeg.cpp:255-264), APPn/COM ignored
// (file.hpp:201-207).  Files outside that (progressive, grayscale, several scans) get JB_ERR_UNSUPPORTED here and are
// then judged by the general rules from their first byte.  Deliberate differences from the reference:
//  * errors are returned (jb_status), never exit(1);
//  * 16-bit quantisation tables keep all 16 bits (the reference keeps the low byte only,
//    jpeg.cpp:216 -- no bundled image has one);
//  * restart intervals are counted in MCUs as ITU-T T.81 says; the reference's test
//    (jpeg.cpp:414,419) agrees with that only when an interval is a whole number of MCU rows
//    (true for its bundled images/img4.jpg: interval 100 = one row).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_hostmem.h"
#include "jb_huff_core.h"
#include "jb_internal.h"
#include "jb_markers.h"

using namespace jbe;

namespace {

// ---- the two rule sets for SOF and SOS ------------------------------------------------------------------------------
// The baseline rules below run first; the general rules (jb_frontend_ext.cpp parse_sof / parse_sos) have the last word on
// every file the baseline rules answer JB_ERR_UNSUPPORTED to, and only on those: any other answer of the baseline rules
// is final.  Both are pinned row by row in tests/golden/frontend_verdicts.json.  Where they differ on purpose:
//  * Order of the frame checks.  Baseline: per component its table id, then its sampling factors, and "empty image" behind
//    the components.  General: "empty image" in front of the components, the generic "bad sampling factor" (outside 1..4)
//    for every component, and the luma / chroma rules behind all of them.  A frame that breaks two rules is named by the
//    baseline rules' first one -- unless that is an UNSUPPORTED one (12-bit precision, a component count other than 3).
//  * A second SOF.  Baseline: accepted, the later frame overwrites the earlier.  General: "more than one frame header".
//    So a file of two baseline three-component frames decodes as its second one.
//  * Ns != 3, or scan components not in the frame's order: UNSUPPORTED by the baseline rules, so decided by the general
//    ones (a scan of fewer components, "scan component not in frame order", ...).
//  * SOF1 and SOF2: UNSUPPORTED by the baseline rules whatever the payload says, decoded by the general ones; the other
//    frame types have a text of their own in each set and the general one is what the caller sees.
//  * Scan parameters: baseline "spectral selection must be 0..63" / "successive approximation must be 0" are
//    UNSUPPORTED, so the general rules judge them (progressive: the four rules of T.81 G.1.1.1; sequential: "sequential
//    scans must cover coefficients 0..63").
//  * "quantisation table not found".  Baseline: per component in front of its Huffman tables.  General: behind all of the
//    scan's checks, for every component of the frame, at every scan.
//  * One component (`gray`: only jb_huff_prepare_ asks, for the device decoder).  The baseline rules then take a
//    one-component SOF0 with any sampling factors in 1..4 and a one-component scan; their refusals of such a scan are
//    JB_ERR_FORMAT with the general rules' texts, but for Ss / Se / Ah / Al, which stay UNSUPPORTED.  Once such a frame has
//    been seen ncomp stays 1, whatever a later SOF says.

int baseline_sof(Header &h, const uint8_t *s, size_t sl, bool gray, Err &e) {  // reference jpeg.cpp:67-146
  if (sl < 6) return set_err(e, JB_ERR_FORMAT, "bad SOF segment");
  if (s[0] != 8) return set_err(e, JB_ERR_UNSUPPORTED, "only 8-bit precision is supported");
  h.desc.height = (s[1] << 8) | s[2];
  h.desc.width = (s[3] << 8) | s[4];
  // one component (rejected by the reference, jpeg.cpp:83-87; the general rules deliver it as a 4:4:4 frame whose Cb and
  // Cr blocks are zero): its sampling factors are irrelevant
  const bool one = gray && s[5] == 1;
  if (!one && s[5] != 3) return set_err(e, JB_ERR_UNSUPPORTED, "only 3 components are supported");
  const int n = one ? 1 : 3;
  if (sl < 6 + 3u * (unsigned)n) return set_err(e, JB_ERR_FORMAT, "bad SOF segment");
  for (int c = 0; c < n; c++) {
    Header::Comp &cp = h.comp[c];
    cp.id = s[6 + 3 * c];
    cp.h = s[7 + 3 * c] >> 4;
    cp.v = s[7 + 3 * c] & 15;
    cp.tq = s[8 + 3 * c];
    if (cp.tq > 3) return set_err(e, JB_ERR_QTAB, "quantisation table id > 3");
    if (one) {
      if (cp.h < 1 || cp.h > 4 || cp.v < 1 || cp.v > 4) return set_err(e, JB_ERR_SAMPLING, "bad sampling factor");
    } else if (c == 0) {
      if ((cp.h != 1 && cp.h != 2) || (cp.v != 1 && cp.v != 2)) return set_err(e, JB_ERR_SAMPLING, "luma sampling factors must be 1 or 2");
    } else if (cp.h != 1 || cp.v != 1) {
      return set_err(e, JB_ERR_SAMPLING, "chroma sampling factors must be 1x1");
    }
    h.desc.qtab_id[c] = cp.tq;
  }
  if (one) {
    h.ncomp = 1;
    h.desc.qtab_id[1] = h.desc.qtab_id[2] = h.comp[0].tq;  // Cb = Cr = 0: any table does
  }
  h.desc.hs = one ? 1 : h.comp[0].h;
  h.desc.vs = one ? 1 : h.comp[0].v;
  h.desc.reserved = 0;
  if (h.desc.width < 1 || h.desc.height < 1) return set_err(e, JB_ERR_GEOMETRY, "empty image");
  h.have_sof = true;
  return JB_OK;
}

int baseline_sos(Header &h, const uint8_t *s, size_t sl, Err &e) {  // reference jpeg.cpp:233-287
  if (!h.have_sof) return set_err(e, JB_ERR_FORMAT, "SOS before SOF");
  const int n = h.ncomp;
  const bool one = n == 1;
  if (sl < 1 || s[0] != n)
    return one ? set_err(e, JB_ERR_FORMAT, "bad number of scan components") : set_err(e, JB_ERR_UNSUPPORTED, "only 3-component scans are supported");
  if (sl != 1 + 2u * (unsigned)n + 3) return set_err(e, JB_ERR_FORMAT, "bad SOS length");
  for (int c = 0; c < n; c++) {
    if (s[1 + 2 * c] != h.comp[c].id)
      return one ? set_err(e, JB_ERR_FORMAT, "scan component not in the frame") : set_err(e, JB_ERR_UNSUPPORTED, "scan component order differs from frame");
    h.dc_id[c] = s[2 + 2 * c] >> 4;
    h.ac_id[c] = s[2 + 2 * c] & 15;
    if (h.dc_id[c] > 3 || h.ac_id[c] > 3) return set_err(e, JB_ERR_FORMAT, "bad Huffman table id in SOS");
  }
  const uint8_t *t = s + 1 + 2 * n;  // Ss, Se, Ah / Al
  if (one) {
    if (t[0] != 0 || t[1] != 63 || t[2] != 0) return set_err(e, JB_ERR_UNSUPPORTED, "a sequential scan of all 64 coefficients only");
  } else {
    if (t[0] != 0 || t[1] != 63) return set_err(e, JB_ERR_UNSUPPORTED, "spectral selection must be 0..63");
    if (t[2] != 0) return set_err(e, JB_ERR_UNSUPPORTED, "successive approximation must be 0");
  }
  // process_image_data's table checks, reference jpeg.cpp:757-774
  for (int c = 0; c < n; c++) {
    if (!h.qset[h.desc.qtab_id[c]]) return set_err(e, JB_ERR_QTAB, "quantisation table not found");
    if (!h.dc[h.dc_id[c]].set) return set_err(e, JB_ERR_FORMAT, "Huffman DC table not found");
    if (!h.ac[h.ac_id[c]].set) return set_err(e, JB_ERR_FORMAT, "Huffman AC table not found");
  }
  return JB_OK;
}

// reference decodeHuffman (jpeg.cpp:405-446): MCUs in raster order, per MCU hs*vs luma blocks
// (v-major), Cb, Cr; DC predictors reset at restart boundaries
int decode_scan(const Header &fr, const jb_geometry &g, int16_t *coef, Err &e) {
  BitReader br(fr.scan, fr.scan + fr.scan_len);
  int pred[3] = {0, 0, 0};
  const int ny = fr.desc.hs * fr.desc.vs;
  const int64_t n_mcus = (int64_t)g.mcus_x * g.mcus_y;
  int until_restart = fr.restart_interval;
  int16_t *out = coef;
  for (int64_t m = 0; m < n_mcus; m++) {
    if (fr.restart_interval && until_restart == 0) {
      if (!br.restart()) return set_err(e, JB_ERR_FORMAT, "restart marker missing");
      pred[0] = pred[1] = pred[2] = 0;
      until_restart = fr.restart_interval;
    }
    for (int b = 0; b < ny + 2; b++) {
      const int c = b < ny ? 0 : b - ny + 1;
      if (!decode_block(br, fr.dc[fr.dc_id[c]], fr.ac[fr.ac_id[c]], pred[c], out))
        return set_err(e, JB_ERR_FORMAT, "corrupt entropy-coded data");
      out += 64;
    }
    until_restart--;
  }
  if (br.overran()) return set_err(e, JB_ERR_FORMAT, "entropy-coded data ends early");
  return JB_OK;
}

// One restart interval on its own: MCUs [m0, m1) from the clean bytes [b, b + len) that lay
// between two RSTn markers.  DC predictors start at 0 at every restart (T.81 F.2.1.3.1; reference
// jpeg.cpp:419-425), so intervals are independent.
int decode_interval(const Header &fr, const jb_geometry &g, const uint8_t *b, size_t len, const uint8_t *hard_limit,
                    int64_t m0, int64_t m1, int16_t *coef) {
  CleanReader br(b);
  int pred[3] = {0, 0, 0};
  const int ny = fr.desc.hs * fr.desc.vs;
  int16_t *out = coef + m0 * g.blocks_per_mcu * 64;
  for (int64_t m = m0; m < m1; m++)
    for (int blk = 0; blk < ny + 2; blk++) {
      const int c = blk < ny ? 0 : blk - ny + 1;
      if (!decode_block_clean(br, fr.dc[fr.dc_id[c]], fr.ac[fr.ac_id[c]], pred[c], out)) return JB_ERR_FORMAT;
      if (br.p > hard_limit) return JB_ERR_FORMAT;  // ran off the end of the scan (the padding keeps the loads in bounds)
      out += 64;
    }
  // more bits consumed than the interval holds: truncated or corrupt data
  return br.consumed_bits(b) > (int64_t)len * 8 ? JB_ERR_FORMAT : JB_OK;
}

// The scan: de-stuffed once (unstuff), then its restart intervals decoded by n_threads host
// threads (1 = this thread).  When the RSTn markers found do not match the frame -- a marker
// missing, an extra one, markers in a file without DRI -- the bit-serial reader above takes over:
// it tolerates what the reference's reader tolerates and produces the precise error.
int decode_scan_mt(const Header &fr, const jb_geometry &g, int16_t *coef, int n_threads, Err &e) {
  const int64_t n_mcus = (int64_t)g.mcus_x * g.mcus_y;
  const int ri = fr.restart_interval;
  const int64_t n_int = ri > 0 ? (n_mcus + ri - 1) / ri : 1;
  static thread_local CleanScan tls_scan;  // (kept per host thread: no allocation per image)
  CleanScan &cs = tls_scan;  // a plain reference: the worker threads below must see THIS thread's buffer
  unstuff(fr.scan, fr.scan + fr.scan_len, cs);
  if ((int64_t)cs.n_intervals() != n_int) return decode_scan(fr, g, coef, e);
  const uint8_t *base = cs.bytes.data();
  const uint8_t *hard_limit = base + cs.start.back() + 8;
  auto run = [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; i++) {
      const int64_t m0 = ri > 0 ? i * ri : 0, m1 = (ri > 0 && m0 + ri < n_mcus) ? m0 + ri : n_mcus;
      const int rc = decode_interval(fr, g, base + cs.start[(size_t)i], cs.start[(size_t)i + 1] - cs.start[(size_t)i],
                                     hard_limit, m0, m1, coef);
      if (rc != JB_OK) return rc;
    }
    return (int)JB_OK;
  };
  if (n_threads > n_int) n_threads = (int)n_int;
  if (n_threads <= 1) {
    // a failure is re-examined by the bit-serial reader, which words the error ("restart marker
    // missing", "ends early", ...) and is the authority on what is tolerated
    return run(0, n_int) == JB_OK ? JB_OK : decode_scan(fr, g, coef, e);
  }
  std::vector<int> rcs((size_t)n_threads, JB_OK);
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; t++)
    th.emplace_back([&, t] { rcs[(size_t)t] = run(n_int * t / n_threads, n_int * (t + 1) / n_threads); });
  for (auto &x : th) x.join();
  for (int rc : rcs)
    if (rc != JB_OK) return decode_scan(fr, g, coef, e);
  return JB_OK;
}

int report(jb_ctx *ctx, const Err &e) { return jb_fail_(ctx, e.code, e.msg.c_str()); }

// ---- jb_huff_prepare_: one image readied for the device-side entropy decoder (jb_huff.hip): see jb_huff.h -----------

// The tables in use and the block-in-MCU lookups.  A frame's three components name at most three tables of each kind
// (reference jpeg.cpp:148-196 reads up to four ids of each kind); AC tables first, then DC.  nullptr, or why not.
const char *prepare_tables(const Header &fr, JbHuffJob *job) {
  int ac_ids[3] = {-1, -1, -1}, dc_ids[3] = {-1, -1, -1}, ac_slot[3], dc_slot[3], n_ac = 0, n_dc = 0;
  for (int c = 0; c < fr.ncomp; c++) {
    for (int kind = 0; kind < 2; kind++) {
      int *ids = kind ? ac_ids : dc_ids, &n = kind ? n_ac : n_dc;
      const int id = kind ? fr.ac_id[c] : fr.dc_id[c];
      int slot = -1;
      for (int q = 0; q < n; q++)
        if (ids[q] == id) slot = q;
      if (slot < 0) ids[slot = n++] = id;
      (kind ? ac_slot : dc_slot)[c] = slot;
    }
  }
  job->n_tabs = (uint32_t)(n_ac + n_dc);
  job->img.n_tabs = job->n_tabs;
  memset(&job->tables, 0, sizeof job->tables);
  uint32_t n_t2 = 0;
  for (int q = 0; q < n_ac + n_dc; q++) {
    const bool is_ac = q < n_ac;
    const HuffTable &t = is_ac ? fr.ac[ac_ids[q]] : fr.dc[dc_ids[q - n_ac]];
    if (!jb_huff_fill_table_(t.counts, t.symbols, is_ac, &job->tables, (uint32_t)q, job->n_tabs, &n_t2))
      return "Huffman tables with more long codes than the device decoder's tables hold: host decoder";
  }
  // a single-component frame: one block per MCU in the scan, delivered as the Y block of a 4:4:4 MCU (Cb, Cr stay zero)
  const uint32_t ny = (uint32_t)(fr.desc.hs * fr.desc.vs);
  job->img.nb = fr.ncomp == 1 ? 1u : ny + 2;
  job->img.blk_bytes = fr.ncomp == 1 ? 384u : 128u;
  job->img.lut_ac = job->img.lut_dc = job->img.lut_comp = 0;
  for (uint32_t b = 0; b < job->img.nb; b++) {
    const uint32_t c = b < ny ? 0u : b - ny + 1u;
    job->img.lut_ac |= (uint32_t)ac_slot[c] << (4 * b);
    job->img.lut_dc |= (uint32_t)(n_ac + dc_slot[c]) << (4 * b);
    job->img.lut_comp |= c << (4 * b);
  }
  return nullptr;
}

// The clean scan and its interval table, against the limits of the device decoder.  nullptr, or which limit.
const char *prepare_scan(const Header &fr, JbHuffJob *job) {
  const int64_t n_mcus = (int64_t)job->geo.mcus_x * job->geo.mcus_y;
  const int ri = fr.restart_interval > 0 ? fr.restart_interval : 0;
  const int64_t n_int = ri > 0 ? (n_mcus + ri - 1) / ri : 1;
  static thread_local CleanScan tls_scan;
  CleanScan &cs = tls_scan;
  unstuff(fr.scan, fr.scan + fr.scan_len, cs);
  if ((int64_t)cs.n_intervals() != n_int) return "restart markers do not match the frame: host decoder";
  if (cs.start.back() > 0x0ffff000u) return "scan too large for 32-bit bit offsets: host decoder";
  job->scan_len = cs.start.back();
  job->scan.assign(cs.bytes.begin(), cs.bytes.begin() + (long)(job->scan_len + 64));  // (unstuff zero-pads far beyond 64)
  job->starts.resize(cs.start.size());
  for (size_t i = 0; i < cs.start.size(); i++) job->starts[i] = (uint32_t)cs.start[i];
  job->img.scan_off = job->img.int_off = job->img.table_set = 0;
  job->img.scan_len = (uint32_t)job->scan_len;
  job->img.n_int = (uint32_t)n_int;
  job->img.ri = (uint32_t)(ri > 0 ? ri : n_mcus);
  job->img.n_mcus = (uint32_t)n_mcus;
  job->img.coef_off = 0;
  job->img.wg0 = 0;
  if ((uint64_t)n_mcus * job->img.nb >= (1u << 24)) return "more blocks than the device decoder's 24-bit block index holds: host decoder";
  job->img.n_blocks = (uint32_t)(n_mcus * job->img.nb);
  // (the kernels address a block by a 32-bit byte offset, jbh_mul24(block, blk_bytes): a large single-component frame wraps it)
  if ((uint64_t)job->img.n_blocks * job->img.blk_bytes >= (1ull << 32)) return "more bytes of blocks than the device decoder's 32-bit block offset holds: host decoder";
  return nullptr;
}

// Every restart interval (a scan without DRI is one interval) is cut into chunks from its own first byte, one lane per
// chunk (jb_huff.h); the caller's knob may force the size (JPEGBLK_CHUNK_BYTES, jb_knobs.h: tests, A/B runs).
int prepare_chunks(JbHuffJob *job, uint32_t chunk_knob, const char **why) {
  const uint32_t chunk_bytes = (chunk_knob == 64 || chunk_knob == 128) ? chunk_knob : kJbChunkBytes;
  job->img.chunk_bytes = chunk_bytes;
  uint64_t n_chunks = 0;
  bool needs_sync = false;
  for (size_t i = 0; i + 1 < job->starts.size(); i++) {
    if (job->starts[i + 1] < job->starts[i]) return *why = "restart intervals out of order", JB_ERR_FORMAT;
    const uint32_t k = jb_chunks_of_(job->starts[i + 1] - job->starts[i], chunk_bytes);
    needs_sync |= k > 1;
    n_chunks += k;
  }
  if (n_chunks > 0x3fffffffu) return *why = "scan too large for the device decoder: host decoder", JB_ERR_UNSUPPORTED;
  job->img.n_chunks = (uint32_t)n_chunks;
  job->img.needs_sync = needs_sync ? 1u : 0u;
  job->img.state_off = 0;
  return JB_OK;
}

}  // namespace

bool jb_huff_fill_table_(const uint8_t counts[17], const uint8_t *symbols, bool is_ac, JbHuffTables *set, uint32_t tix, uint32_t n_tabs, uint32_t *n_t2) {
  return jb_huff_fill_table_impl_(counts, symbols, is_ac, set, tix, n_tabs, n_t2);
}

// ---- the front end in steps, on the shared header (jb_internal.h) ---------------------------------------------------
// The baseline rules over a file: its header and where its one scan begins.
int jb_parse_baseline_(const uint8_t *d, size_t n, Header &h, bool gray, Err &e) {
  MarkerWalk w(d, n);
  int rc = w.soi(e);
  while (rc == JB_OK) {
    rc = w.next(false, e);
    if (rc != MarkerWalk::kSegment) return rc;  // (an error: without a scan the walk does not end)
    rc = JB_OK;
    const uint8_t m = w.marker;
    if (m == 0xdb) {
      rc = parse_dqt(h, w.s, w.sl, e);
    } else if (m == 0xc0) {
      rc = baseline_sof(h, w.s, w.sl, gray, e);
    } else if (m == 0xc2) {
      rc = set_err(e, JB_ERR_UNSUPPORTED, "progressive JPEG is not supported");  // jpeg.cpp:69-73
    } else if (other_sof(m, 0xc1)) {
      rc = set_err(e, JB_ERR_UNSUPPORTED, "only baseline (SOF0) frames are supported");
    } else if (m == 0xc4) {
      rc = parse_dht(h, w.s, w.sl, true, e);
    } else if (m == 0xdd) {
      rc = parse_dri(h, w.s, w.sl, e);
    } else if (m == 0xda) {
      rc = baseline_sos(h, w.s, w.sl, e);
      h.scan = d + w.pos;
      h.scan_len = n - w.pos;
      return rc;
    }
    // APPn (E0-EF), COM (FE), anything else with a length: ignored (reference file.hpp:201-207)
  }
  return rc;
}

// The scan of a header the baseline rules took (three components) into `coef`.
int jb_decode_baseline_(const Header &h, int16_t *coef, size_t coef_cap_bytes, int n_threads, Err &e) {
  jb_geometry g;
  const int rc = jb_geometry_of(&h.desc, &g);
  if (rc) return set_err(e, rc, "bad frame geometry");
  if ((size_t)g.coef_bytes > coef_cap_bytes) return set_err(e, JB_ERR_CAPACITY, "coefficient buffer too small");
  return decode_scan_mt(h, g, coef, n_threads, e);
}

// A device job from a header the baseline rules took with `gray`: the table slots and lookups, the scan against the
// device decoder's limits, the chunk count.  *why: the text of a refusal.
int jb_huff_prepare_header_(const Header &h, JbHuffJob *job, uint32_t chunk_knob, const char **why) {
  job->desc = h.desc;
  memcpy(job->qtabs, h.qtabs, sizeof job->qtabs);
  int rc = jb_geometry_of(&h.desc, &job->geo);
  if (rc != JB_OK) return *why = "bad frame geometry", rc;
  if ((*why = prepare_tables(h, job)) || (*why = prepare_scan(h, job))) return JB_ERR_UNSUPPORTED;
  rc = prepare_chunks(job, chunk_knob, why);
  if (rc != JB_OK) return rc;
  if (h.restart_interval <= 0 && job->scan_len == 0) return *why = "empty scan", JB_ERR_FORMAT;
  return JB_OK;
}

int jb_huff_prepare_(const uint8_t *jpeg, size_t jpeg_bytes, JbHuffJob *job, std::string *err, uint32_t chunk_knob) {
  const std::unique_ptr<Header> h(new Header());
  Err e;
  const char *why = nullptr;
  int rc = jb_parse_baseline_(jpeg, jpeg_bytes, *h, true, e);
  if (rc == JB_OK) rc = jb_huff_prepare_header_(*h, job, chunk_knob, &why);
  if (err) *err = why ? why : rc ? e.msg : "";
  return rc;
}

extern "C" {

int jb_entropy_decode(const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc, uint16_t *qtabs,
                      int16_t *coef, size_t coef_cap_bytes) {
  return jb_entropy_decode_mt(jpeg, jpeg_bytes, desc, qtabs, coef, coef_cap_bytes, 1);
}

int jb_entropy_decode_mt(const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc, uint16_t *qtabs,
                         int16_t *coef, size_t coef_cap_bytes, int n_threads) {
  if (!jpeg || !desc) return jb_fail_(nullptr, JB_ERR_NULL, "jb_entropy_decode: NULL pointer");
  std::unique_ptr<Header> h(new Header());
  Err e;
  int rc = jb_parse_baseline_(jpeg, jpeg_bytes, *h, false, e);
  if (rc == JB_ERR_UNSUPPORTED) {
    // not the common case (baseline, three components, one interleaved scan): the general rules take progressive,
    // grayscale and multi-scan files, and reject the rest
    h.reset();
    std::string text;
    rc = jb_ext_decode_(jpeg, jpeg_bytes, desc, qtabs, coef, coef_cap_bytes, &text);
    return rc ? jb_fail_(nullptr, rc, text.c_str()) : JB_OK;
  }
  if (rc == JB_OK) {
    *desc = h->desc;
    if (qtabs) memcpy(qtabs, h->qtabs, sizeof h->qtabs);
    if (coef) rc = jb_decode_baseline_(*h, coef, coef_cap_bytes, n_threads, e);
  }
  return rc ? report(nullptr, e) : JB_OK;
}

}  // extern "C"

// What an entry point asks of the decode beyond the bytes: denom 1, 2, 4, 8; spec: null or format 0 (interleaved uint8)
// or a checked planar spec; roi: null or a rectangle of the frame (denom 1); target: null or the output's size (denom 1).
// The output's sizes come from the plan of the frame (jb_plan.h).
struct DecodeRequest {
  int denom = 1;
  const jb_output_spec *spec = nullptr;
  const jb_roi *roi = nullptr;
  const JbTarget *target = nullptr;
  const jb_fit *fit = nullptr;
};

// Every jb_decode_memory* and jb_decode_file* behind its shell (decode_entry): the file is parsed once per rule set, and
// both routes into the pixel kernel end in one tail (deliver).  Errors surface in this order: the draft's refusal, the
// header's, the plan's, the staging ring's, allocation, the scan's.
static int decode_memory_impl(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const DecodeRequest &rq, uint8_t **rgb,
                              int32_t *width, int32_t *height) {
  if (!jpeg || !rgb || !width || !height) return jb_fail_(ctx, JB_ERR_NULL, "jb_decode_memory: NULL pointer");
  *rgb = nullptr;
  if (rq.denom != 1 && rq.denom != 2 && rq.denom != 4 && rq.denom != 8) return jb_fail_(ctx, JB_ERR_GEOMETRY, "jb_decode_memory_scaled: denom is not 1, 2, 4 or 8");
  // "orientation" (include/jpegblk.h): the context's, or under JB_ORIENT_EXIF the file's own (1 when it has none)
  int orient = jb_ctx_orientation(ctx);
  // "draft decode": the plan is that of the context's draft frame; what does not go with a draft is refused before
  // anything is decoded
  const int draft = jb_ctx_draft(ctx);
  if (const char *why = jb_draft_refusal_(draft, jb_ctx_arithmetic(ctx), rq.denom, orient)) return jb_fail_(ctx, JB_ERR_UNSUPPORTED, why);
  if (orient == JB_ORIENT_EXIF && jb_exif_orientation(jpeg, jpeg_bytes, &orient) != JB_OK) orient = JB_ORIENT_STORED;
  // the one tail: plan -> allocate -> run(out, plan) -> publish
  auto deliver = [&](const jb_image_desc &desc, auto run) -> int {
    const jb_image_desc frame = jb_draft_desc_(&desc, draft);
    const JbOutPlan plan = jb_out_plan_(&frame, rq.denom, rq.spec, rq.roi, rq.target, nullptr, 0, orient, rq.fit);
    if (plan.status != JB_OK) return jb_fail_(ctx, plan.status, plan.why);
    uint8_t *out = jb_alloc_pixels_((size_t)plan.image_bytes);
    if (!out) return jb_fail_(ctx, JB_ERR_CAPACITY, "out of host memory");
    const int rc = run(out, plan);
    if (rc != JB_OK) {
      free(out);
      return rc;
    }
    *rgb = out;
    *width = plan.out_w;
    *height = plan.out_h;
    jb_ctx_set_last_desc_(ctx, &desc);
    return JB_OK;
  };
  Err e;
  // The entropy stage of a baseline file can run on the device too (jb_huff.hip): the host then only
  // parses the headers and removes the byte stuffing.  One image is one latency-bound submission
  // (a dozen and a half launches: about 1 ms whatever the size, then ~0.4 ms per megabyte of scan)
  // against 5.5 ms per megabyte on one host core, so by default the device takes files of
  // kAutoDeviceScan bytes of scan or more -- measured with round 3's kernels: 679x451 (80 KB) 0.56-0.85 ms against
  // 0.67-0.73 on the host, 1024x768 4:2:0 (204 KB) 0.63 against 1.19, 1280x720 4:2:0 (238 KB) 0.57 against 1.36,
  // 1920x1080 4:4:4 (760 KB) 0.51 against 3.9, 8192x8192 4:2:0 (17 MB) 7.5 against 94
  // (tools/single_latency.py, profiles/r03/single_latency.txt; the threshold was 256 KB with round 2's kernels).  JPEGBLK_GPU_HUFFMAN=0: always the host decoder;
  // =1: the device for every file with 16 restart intervals / chunks or more; =2: also fewer intervals.
  // Whatever the device decoder does not take or flags as corrupt goes through the host decoder
  // below, which gives the precise answer.
  constexpr size_t kAutoDeviceScan = (size_t)128 << 10;
  const JbKnobs &knobs = *jb_ctx_knobs_(ctx);  // (read when the context was created: jb_knobs.h)
  const bool forced = knobs.gpu_huffman == 1 || knobs.gpu_huffman == 2;
  const bool automatic = knobs.gpu_huffman < 0;
  const uint32_t min_int = knobs.gpu_huffman == 2 ? 1u : 16u;
  if (forced || (automatic && jpeg_bytes >= kAutoDeviceScan)) {
    // JPEGBLK_TIMING=1: where one decode(bytes) through the device path spends its time, on stderr
    const bool timing = knobs.timing == 1;
    const double t0 = timing ? jb_now_s_() : 0;
    const std::unique_ptr<JbHuffJob> job(new JbHuffJob());
    const std::unique_ptr<Header> hd(new Header());
    const char *why = nullptr;
    // (the baseline rules with one-component frames: the device decoder takes those too)
    if (jb_parse_baseline_(jpeg, jpeg_bytes, *hd, true, e) == JB_OK && jb_huff_prepare_header_(*hd, job.get(), knobs.chunk_bytes, &why) == JB_OK && jb_huff_worth_it_(*job, min_int) &&
        (forced || job->scan_len >= kAutoDeviceScan)) {
      const double t1 = timing ? jb_now_s_() : 0;
      const int drc = deliver(job->desc, [&](uint8_t *out, const JbOutPlan &plan) {
        const int jrc = jb_decode_job_(ctx, job.get(), out, plan);
        if (timing)
          fprintf(stderr, "jb_decode_memory(device path): prepare %.3f ms, submit + wait %.3f ms (%u intervals, %u chunks, %zu bytes of scan), rc %d\n",
                  (t1 - t0) * 1e3, (jb_now_s_() - t1) * 1e3, job->img.n_int, job->img.n_chunks, job->scan_len, jrc);
        return jrc;
      });
      if (drc != JB_ERR_FORMAT) return drc;  // a HIP / capacity error is not the stream's fault
    }
  }
  // the host decoder: the baseline rules, and on JB_ERR_UNSUPPORTED the general rules from the first byte
  const std::unique_ptr<Header> h(new Header());
  int rc = jb_parse_baseline_(jpeg, jpeg_bytes, *h, false, e);
  std::unique_ptr<Ext> x;
  if (rc == JB_ERR_UNSUPPORTED) {
    x.reset(new Ext());
    rc = jb_ext_parse_(jpeg, jpeg_bytes, *x, e);
  }
  if (rc) return jb_fail_(ctx, rc, e.msg.c_str());
  const Header &hd = x ? *x : *h;
  jb_geometry g;
  rc = jb_geometry_of(&hd.desc, &g);
  if (rc) return jb_fail_(ctx, rc, "bad frame geometry");
  return deliver(hd.desc, [&](uint8_t *out, const JbOutPlan &plan) {
    // the staging ring follows the frame (a context sized for another image, or created with (0,0))
    int drc = jb_ctx_reserve(ctx, (size_t)g.coef_bytes, (size_t)plan.image_bytes);
    if (drc) return drc;
    int16_t *coef = (int16_t *)jb_pinned_alloc_on(jb_ctx_device(ctx), (size_t)g.coef_bytes);
    if (!coef) return jb_fail_(ctx, JB_ERR_HIP, jb_last_error(nullptr));
    drc = x ? jb_ext_scans_(*x, coef, (size_t)g.coef_bytes, e) : jb_decode_baseline_(*h, coef, (size_t)g.coef_bytes, 1, e);
    if (drc) jb_fail_(ctx, drc, e.msg.c_str());
    else drc = jb_blocks_to_rgb_plan_(ctx, &hd.desc, coef, &hd.qtabs[0][0], out, plan);
    jb_pinned_free(coef);
    return drc;
  });
}

// The shell of the twelve entry points: the context, the entry point's own pointers (args_ok), *clear = nullptr, for a
// file (path_given) its bytes, the spec -- then the decode.  fn is the entry point's name as its texts spell it, which is
// not always its own: jb_decode_file_scaled reports as jb_decode_file; a bad spec is reported under the name of the
// jb_decode_memory* twin (spec_fn) by the file entry points too; and the pointers that every entry point has (the bytes,
// the output, the sizes) and the denominator are reported by decode_memory_impl as jb_decode_memory's / _scaled's.
static int decode_entry(jb_ctx *ctx, const char *fn, const char *spec_fn, bool args_ok, void **clear, bool path_given, const char *path,
                        const uint8_t *jpeg, size_t jpeg_bytes, const DecodeRequest &rq, void **out, int32_t *width, int32_t *height) {
  if (!ctx) return jb_fail_(nullptr, JB_ERR_NULL, (std::string(fn) + ": ctx is NULL").c_str());
  if (!args_ok) return jb_fail_(ctx, JB_ERR_NULL, (std::string(fn) + ": NULL pointer").c_str());
  if (clear) *clear = nullptr;
  std::vector<uint8_t> buf;
  if (path_given) {
    if (!path) return jb_fail_(ctx, JB_ERR_NULL, (std::string(fn) + ": path is NULL").c_str());
    if (!jb_read_file_(path, buf)) return jb_fail_(ctx, JB_ERR_FORMAT, (std::string("cannot open ") + path).c_str());
    jpeg = buf.data();
    jpeg_bytes = buf.size();
  }
  if (spec_fn && rq.spec && jb_tight_spec_check_(rq.spec) != JB_OK)
    return jb_fail_(ctx, JB_ERR_GEOMETRY, (std::string(spec_fn) + JB_TIGHT_SPEC_TEXT).c_str());
  return decode_memory_impl(ctx, jpeg, jpeg_bytes, rq, (uint8_t **)out, width, height);
}

static JbTarget target_of(const jb_resize *rs) { return rs ? JbTarget{rs->out_w, rs->out_h, rs->filter, rs->reserved} : JbTarget{0, 0, 0, 0}; }

extern "C" {

int jb_decode_memory(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, uint8_t **rgb, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_memory", nullptr, true, nullptr, false, nullptr, jpeg, jpeg_bytes, {}, (void **)rgb, width, height);
}

// denom = 1: jb_decode_memory; 2, 4, 8: the same decode with the area-reduced store stage (include/jpegblk.h)
int jb_decode_memory_scaled(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, int denom, uint8_t **rgb, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_memory", nullptr, true, nullptr, false, nullptr, jpeg, jpeg_bytes, {denom}, (void **)rgb, width, height);
}

// the same decode in an output format ("tensor-ready output", include/jpegblk.h); format 0 is jb_decode_memory
int jb_decode_memory_fmt(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_memory_fmt", "jb_decode_memory_fmt", spec && out, out, false, nullptr, jpeg, jpeg_bytes, {1, spec}, out, width, height);
}

// a rectangle of the same decode ("region of interest", include/jpegblk.h); spec: null = interleaved uint8
int jb_decode_memory_roi(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_output_spec *spec, void **out,
                         int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_memory_roi", "jb_decode_memory_roi", roi && out, out, false, nullptr, jpeg, jpeg_bytes, {1, spec, roi}, out, width, height);
}

// the same decode at a fixed output size ("fixed output size", include/jpegblk.h); roi: null = the whole image; spec:
// null = interleaved uint8
int jb_decode_memory_resized(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, int32_t out_w, int32_t out_h,
                             const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  const JbTarget t = {out_w, out_h, 0, 0};
  return decode_entry(ctx, "jb_decode_memory_resized", "jb_decode_memory_resized", out, out, false, nullptr, jpeg, jpeg_bytes, {1, spec, roi, &t}, out, width, height);
}

// the same with a resampling filter ("resampling filters", include/jpegblk.h)
int jb_decode_memory_filtered(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_resize *rs,
                              const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  const JbTarget t = target_of(rs);
  return decode_entry(ctx, "jb_decode_memory_filtered", "jb_decode_memory_filtered", out && rs, out, false, nullptr, jpeg, jpeg_bytes, {1, spec, roi, &t}, out, width, height);
}

// the same with a fit ("fit", include/jpegblk.h)
int jb_decode_memory_fit(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit,
                         const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  const JbTarget t = target_of(rs);
  return decode_entry(ctx, "jb_decode_memory_fit", "jb_decode_memory_fit", out && rs, out, false, nullptr, jpeg, jpeg_bytes, {1, spec, roi, &t, fit}, out, width, height);
}

int jb_decode_file(jb_ctx *ctx, const char *path, uint8_t **rgb, int32_t *width, int32_t *height) {
  return jb_decode_file_scaled(ctx, path, 1, rgb, width, height);
}

int jb_decode_file_scaled(jb_ctx *ctx, const char *path, int denom, uint8_t **rgb, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_file", nullptr, true, nullptr, true, path, nullptr, 0, {denom}, (void **)rgb, width, height);
}

int jb_decode_file_fmt(jb_ctx *ctx, const char *path, const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_file_fmt", "jb_decode_memory_fmt", spec && out, out, true, path, nullptr, 0, {1, spec}, out, width, height);
}

int jb_decode_file_roi(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_output_spec *spec, void **out, int32_t *width, int32_t *height) {
  return decode_entry(ctx, "jb_decode_file_roi", "jb_decode_memory_roi", roi && out, out, true, path, nullptr, 0, {1, spec, roi}, out, width, height);
}

int jb_decode_file_resized(jb_ctx *ctx, const char *path, const jb_roi *roi, int32_t out_w, int32_t out_h, const jb_output_spec *spec,
                           void **out, int32_t *width, int32_t *height) {
  const JbTarget t = {out_w, out_h, 0, 0};
  return decode_entry(ctx, "jb_decode_file_resized", "jb_decode_memory_resized", out, out, true, path, nullptr, 0, {1, spec, roi, &t}, out, width, height);
}

int jb_decode_file_filtered(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_resize *rs, const jb_output_spec *spec, void **out,
                            int32_t *width, int32_t *height) {
  const JbTarget t = target_of(rs);
  return decode_entry(ctx, "jb_decode_file_filtered", "jb_decode_memory_filtered", out && rs, out, true, path, nullptr, 0, {1, spec, roi, &t}, out, width, height);
}

int jb_decode_file_fit(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit, const jb_output_spec *spec,
                       void **out, int32_t *width, int32_t *height) {
  const JbTarget t = target_of(rs);
  return decode_entry(ctx, "jb_decode_file_fit", "jb_decode_memory_fit", out && rs, out, true, path, nullptr, 0, {1, spec, roi, &t, fit}, out, width, height);
}

}  // extern "C"
