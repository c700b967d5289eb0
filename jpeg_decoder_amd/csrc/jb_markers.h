// jb_markers.h -- internal: what the two rule sets of the host front end (jb_frontend.cpp: baseline, jb_frontend_ext.cpp:
// general) share in front of the entropy-coded bytes: the header a file's segments fill, the walk over its markers, and
// the one body each of DQT, DHT and DRI.  The frame and scan rules (SOF, SOS) are the rule sets' own; the list of where
// they differ on purpose is in jb_frontend.cpp, above baseline_sof.
#ifndef JB_MARKERS_H
#define JB_MARKERS_H

#include "jb_entropy.h"

namespace jbe {

// What the segments in front of a scan say.  About 210 KB (eight Huffman tables with their lookahead): on the heap.
struct Header {
  jb_image_desc desc;
  bool have_sof = false, progressive = false;
  int ncomp = 3;  // 1: a single-component frame (the baseline rules take those only for jb_huff_prepare_: `gray`)
  struct Comp {
    int id = 0, h = 1, v = 1, tq = 0;
  } comp[3];
  uint16_t qtabs[4][64] = {};  // de-zigzagged (reference types.hpp:88-90); all 16 bits of a 16-bit table
  bool qset[4] = {false, false, false, false};
  HuffTable dc[4], ac[4];
  int restart_interval = 0;
  // the baseline rules' one scan: table ids per frame component, and its bytes up to the end of the buffer
  int dc_id[3] = {0, 0, 0}, ac_id[3] = {0, 0, 0};
  const uint8_t *scan = nullptr;
  size_t scan_len = 0;
};

// The walk over the markers of [d, d + n): next() gives one segment with a payload at a time.
struct MarkerWalk {
  const uint8_t *d;
  size_t n, pos = 2;
  uint8_t marker = 0;
  const uint8_t *s = nullptr;  // the payload behind the length
  size_t sl = 0, at = 0;       // its bytes; where the segment's FF stands
  enum { kSegment = 1, kEnd = 2 };

  MarkerWalk(const uint8_t *data, size_t bytes) : d(data), n(bytes) {}
  int soi(Err &e) const {
    return !d || n < 4 || d[0] != 0xff || d[1] != 0xd8 ? set_err(e, JB_ERR_FORMAT, "not a JPEG file (no SOI)") : (int)JB_OK;
  }
  // kSegment, kEnd (EOI or the end of the bytes, accepted only once a scan has been decoded: have_scan) or an error.
  // Fill bytes in front of a marker and the markers without a payload (SOI, TEM, RSTn) are passed over; APPn, COM and
  // anything else with a length is the caller's to ignore (reference file.hpp:201-207).
  int next(bool have_scan, Err &e) {
    while (true) {
      if (pos + 1 >= n) return have_scan ? (int)kEnd : set_err(e, JB_ERR_FORMAT, "truncated file (no SOS)");
      if (d[pos] != 0xff) return set_err(e, JB_ERR_FORMAT, "marker expected");
      at = pos;
      while (pos < n && d[pos] == 0xff) pos++;
      if (pos >= n) return have_scan ? (int)kEnd : set_err(e, JB_ERR_FORMAT, "truncated file");
      marker = d[pos++];
      if (marker == 0xd8 || marker == 0x01 || (marker >= 0xd0 && marker <= 0xd7)) continue;
      if (marker == 0xd9) return have_scan ? (int)kEnd : set_err(e, JB_ERR_FORMAT, "EOI before SOS");
      if (pos + 2 > n) return set_err(e, JB_ERR_FORMAT, "truncated segment");
      const size_t len = ((size_t)d[pos] << 8) | d[pos + 1];
      if (len < 2 || pos + len > n) return set_err(e, JB_ERR_FORMAT, "bad segment length");
      s = d + pos + 2;
      sl = len - 2;
      pos += len;
      return kSegment;
    }
  }
};

// a frame header this project does not decode: SOF3..SOF15 without DHT (C4), JPG (C8) and DAC (CC)
inline bool other_sof(uint8_t m, uint8_t first) { return m >= first && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc; }

inline int parse_dqt(Header &h, const uint8_t *s, size_t sl, Err &e) {  // reference jpeg.cpp:197-231
  size_t i = 0;
  while (i < sl) {
    const int pq = s[i] >> 4, tq = s[i] & 15;
    i++;
    if (tq > 3) return set_err(e, JB_ERR_QTAB, "quantisation table id > 3");
    const size_t need = pq ? 128 : 64;
    if (pq > 1 || i + need > sl) return set_err(e, JB_ERR_FORMAT, "bad DQT segment");
    for (int k = 0; k < 64; k++)
      h.qtabs[tq][kZigZag[k]] = pq ? (uint16_t)((s[i + 2 * k] << 8) | s[i + 2 * k + 1]) : s[i + k];
    h.qset[tq] = true;
    i += need;
  }
  return JB_OK;
}

// cached: the tables through HuffTable::build_cached (the baseline rules: the files of a batch mostly carry the same
// tables); the symbols behind the last one are zeroed because that cache compares whole arrays
inline int parse_dht(Header &h, const uint8_t *s, size_t sl, bool cached, Err &e) {  // reference jpeg.cpp:148-196
  size_t i = 0;
  while (i < sl) {
    if (i + 17 > sl) return set_err(e, JB_ERR_FORMAT, "bad DHT segment");
    const int tc = s[i] >> 4, th = s[i] & 15;
    if (th > 3 || tc > 1) return set_err(e, JB_ERR_FORMAT, "bad Huffman table id");
    HuffTable &t = tc ? h.ac[th] : h.dc[th];
    int total = 0;
    t.counts[0] = 0;
    for (int l = 1; l <= 16; l++) {
      t.counts[l] = s[i + l];
      total += s[i + l];
    }
    i += 17;
    if (total > 256 || i + total > sl) return set_err(e, JB_ERR_FORMAT, "bad DHT segment");
    memcpy(t.symbols, s + i, (size_t)total);
    i += (size_t)total;
    memset(t.symbols + total, 0, (size_t)(256 - total));
    if (!(cached ? t.build_cached(tc != 0) : t.build(tc != 0))) return set_err(e, JB_ERR_FORMAT, "over-subscribed Huffman table");
  }
  return JB_OK;
}

inline int parse_dri(Header &h, const uint8_t *s, size_t sl, Err &e) {  // reference jpeg.cpp:289-298
  if (sl != 2) return set_err(e, JB_ERR_FORMAT, "bad DRI segment");
  h.restart_interval = (s[0] << 8) | s[1];
  return JB_OK;
}

// The general rules' header: the frame's geometry, each component's own block grid (non-interleaved scans), where the
// coefficients go, and where the walk stands (jb_frontend_ext.cpp).
struct Ext : Header {
  jb_geometry g;
  struct Grid {
    int bw = 0, bh = 0;
  } grid[3];
  int16_t *coef = nullptr;
  int ny = 1, bpm = 3;
  const uint8_t *bytes = nullptr;  // the file, and the first SOS in it: where the scans begin
  size_t n_bytes = 0, first_sos = 0;

  // block (by, bx) of frame component c -> its place in the MCU-interleaved array
  inline int16_t *block(int c, int by, int bx) const {
    int64_t idx;
    if (c == 0) {
      const int hs = desc.hs, vs = desc.vs;
      idx = ((int64_t)(by / vs) * g.mcus_x + bx / hs) * bpm + (by % vs) * hs + bx % hs;
    } else {
      idx = ((int64_t)by * g.mcus_x + bx) * bpm + ny + c - 1;
    }
    return coef + idx * 64;
  }
};

}  // namespace jbe

#endif
