// exif_check -- jb_exif_orientation (csrc/jb_exif.cpp) under AddressSanitizer + UBSan: every prefix and every
// single-byte mutation (all 255 other values of every byte) of valid files, each in a heap block of exactly its length,
// so a read outside [jpeg, jpeg + bytes) is a report.  Whatever the bytes, the answer is JB_OK with a value in 1..8, or
// JB_ERR_FORMAT with 1 when they do not start with SOI.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/jpegblk.h"

static long n_calls = 0;

static void put16(std::vector<uint8_t> &v, unsigned x, bool big) {
  v.push_back((uint8_t)(big ? x >> 8 : x));
  v.push_back((uint8_t)(big ? x : x >> 8));
}
static void put32(std::vector<uint8_t> &v, unsigned x, bool big) {
  put16(v, big ? x >> 16 : x & 0xffff, big);
  put16(v, big ? x & 0xffff : x >> 16, big);
}

// SOI, APP0 (JFIF), an Exif APP1 whose IFD0 holds ImageWidth, Orientation and XResolution, DQT stub, SOS, data, EOI
static std::vector<uint8_t> file_with(int value, bool big) {
  std::vector<uint8_t> t;  // the TIFF structure
  t.push_back(big ? 'M' : 'I'), t.push_back(big ? 'M' : 'I');
  put16(t, 42, big);
  put32(t, 8, big);
  put16(t, 3, big);
  put16(t, 0x0100, big), put16(t, 4, big), put32(t, 1, big), put32(t, 640, big);
  put16(t, 0x0112, big), put16(t, 3, big), put32(t, 1, big), put16(t, (unsigned)value, big), put16(t, 0, big);
  put16(t, 0x011a, big), put16(t, 5, big), put32(t, 1, big), put32(t, 50, big);
  put32(t, 0, big);
  put32(t, 72, big), put32(t, 1, big);
  std::vector<uint8_t> f = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  f.push_back(0xFF), f.push_back(0xE1);
  put16(f, (unsigned)(2 + 6 + t.size()), true);
  for (char c : {'E', 'x', 'i', 'f', '\0', '\0'}) f.push_back((uint8_t)c);
  f.insert(f.end(), t.begin(), t.end());
  for (uint8_t b : {0xFF, 0xDB, 0x00, 0x04, 0x00, 0x01, 0xFF, 0xDA, 0x00, 0x02, 0x12, 0x34, 0xFF, 0xD9}) f.push_back(b);
  return f;
}

static int call(const uint8_t *bytes, size_t n) {
  uint8_t *exact = (uint8_t *)malloc(n ? n : 1);  // (malloc(0) may be null: then one byte that is never promised)
  if (n) memcpy(exact, bytes, n);
  int o = -1;
  const int rc = jb_exif_orientation(exact, n, &o);
  free(exact);
  n_calls++;
  const bool soi = n >= 2 && bytes[0] == 0xFF && bytes[1] == 0xD8;
  if (rc != (soi ? JB_OK : JB_ERR_FORMAT) || o < 1 || o > 8 || (rc != JB_OK && o != 1)) {
    printf("FAIL: %zu bytes, rc %d, orientation %d\n", n, rc, o);
    exit(1);
  }
  return o;
}

int main() {
  for (int big = 0; big < 2; big++)
    for (int value = 0; value <= 9; value++) {
      const std::vector<uint8_t> f = file_with(value, big != 0);
      const int want = value >= 1 && value <= 8 ? value : 1;
      if (call(f.data(), f.size()) != want) return printf("FAIL: value %d (%s) reads %d\n", value, big ? "MM" : "II", call(f.data(), f.size())), 1;
      if (value != 6) continue;
      // every prefix: the tag is only believed once its entry lies inside the bytes -- and the segment inside the file
      for (size_t n = 0; n < f.size(); n++) {
        const int o = call(f.data(), n);
        if (o != 1 && o != want) return printf("FAIL: prefix %zu reads %d\n", n, o), 1;
      }
      std::vector<uint8_t> m = f;
      for (size_t i = 0; i < f.size(); i++) {
        for (int v = 0; v < 256; v++)
          if (v != f[i]) m[i] = (uint8_t)v, call(m.data(), m.size());
        m[i] = f[i];
      }
    }
  int o = 0;
  if (jb_exif_orientation(nullptr, 4, &o) != JB_ERR_NULL || jb_exif_orientation((const uint8_t *)"\xff\xd8", 2, nullptr) != JB_ERR_NULL)
    return printf("FAIL: null arguments\n"), 1;
  printf("%ld exif calls ok\n", n_calls);
  return 0;
}
