// jb_exif.cpp -- "orientation" (include/jpegblk.h): the Exif Orientation tag of a JPEG byte stream.  Host-only and
// free-standing, so tools/fuzz builds it for the CPU with sanitizers.  Every read goes through `at`, which knows the
// end of what may be read: first the file's, inside the APP1 payload the segment's.
#include "../../include/jpegblk.h"

namespace {

struct Bytes {
  const uint8_t *p;
  size_t n;
  bool has(size_t off, size_t len) const { return off <= n && len <= n - off; }
  uint32_t u16(size_t off, bool big) const { return big ? (uint32_t)p[off] << 8 | p[off + 1] : (uint32_t)p[off + 1] << 8 | p[off]; }
  uint32_t u32(size_t off, bool big) const { return big ? u16(off, big) << 16 | u16(off + 2, big) : u16(off + 2, big) << 16 | u16(off, big); }
};

// the TIFF structure behind "Exif\0\0": 1..8, or 1 for everything else
int tiff_orientation(const Bytes t) {
  if (!t.has(0, 8)) return 1;
  const bool big = t.p[0] == 'M' && t.p[1] == 'M';
  if (!big && !(t.p[0] == 'I' && t.p[1] == 'I')) return 1;
  if (t.u16(2, big) != 42) return 1;
  const size_t ifd = t.u32(4, big);
  if (!t.has(ifd, 2)) return 1;
  const size_t n = t.u16(ifd, big);
  for (size_t i = 0; i < n; i++) {
    const size_t e = ifd + 2 + 12 * i;  // (at most 2^32 + 2 + 12 * 65535: no overflow in 64 bits)
    if (!t.has(e, 12)) return 1;
    if (t.u16(e, big) != 0x0112) continue;
    if (t.u16(e + 2, big) != 3 || t.u32(e + 4, big) != 1) return 1;  // SHORT, count 1: the value lies in the entry
    const uint32_t v = t.u16(e + 8, big);
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

}  // namespace

extern "C" int jb_exif_orientation(const uint8_t *jpeg, size_t bytes, int *orientation) {
  if (!jpeg || !orientation) return JB_ERR_NULL;
  *orientation = 1;
  const Bytes f = {jpeg, bytes};
  if (!f.has(0, 2) || jpeg[0] != 0xFF || jpeg[1] != 0xD8) return JB_ERR_FORMAT;
  size_t at = 2;
  while (f.has(at, 4)) {
    if (jpeg[at] != 0xFF) return JB_OK;  // not a marker: nothing this parser can walk
    const int m = jpeg[at + 1];
    if (m == 0xFF) {  // a fill byte
      at++;
      continue;
    }
    if (m == 0xDA || m == 0xD9) return JB_OK;                            // SOS, EOI: the headers are over
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0xD8 || m == 0) {  // markers without a length
      at += 2;
      continue;
    }
    const size_t len = (size_t)jpeg[at + 2] << 8 | jpeg[at + 3];
    if (len < 2 || !f.has(at + 2, len)) return JB_OK;  // a length that leaves the file
    if (m == 0xE1 && len >= 8 && jpeg[at + 4] == 'E' && jpeg[at + 5] == 'x' && jpeg[at + 6] == 'i' && jpeg[at + 7] == 'f' &&
        jpeg[at + 8] == 0 && jpeg[at + 9] == 0) {
      *orientation = tiff_orientation(Bytes{jpeg + at + 10, len - 8});
      return JB_OK;  // the first Exif segment decides
    }
    at += 2 + len;
  }
  return JB_OK;
}
