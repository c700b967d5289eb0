// tools/fuzz/frontend_verdicts.cpp -- the host front end's verdict on every file of tests/frontend_cases.py, one row
// per case: what tests/golden/frontend_verdicts.json records and tests/test_frontend_verdicts_cpu.py compares.  Built
// for the CPU from the front end's own sources with AddressSanitizer + UBSan, the device half stubbed as in
// fuzz_frontend.cpp; the stubs of the two device routes note which one was asked for and with which plan.
//
//   make -C tools/fuzz frontend_verdicts && tools/fuzz/frontend_verdicts <cases file> <good.jpg> <corrupt.jpg>
// ("-" for the two files: no rows of the entry points)
//
// The cases file (tools/record_frontend_verdicts.py writes it):
//   S <seed> <hex>                               a seed file
//   B <case> <hex>                               a case given by its bytes
//   C <case> <seed> <length> [<offset>:<hex>]... a case that is the first <length> bytes of a seed with bytes replaced
//   H <case> <seed> <length> [<offset>:<hex>]... the same, its row without the calls that decode the scan (b1, b3, bs)
// A row is "<case>\t<field>\t<field>...", a field "<call>=<status>|<text>[|<what came back>]":
//   a          jb_entropy_decode, headers only: the descriptor
//   b1, b3     jb_entropy_decode_mt with a buffer of the frame's size (one block when `a` failed) at 1 and 3 threads:
//              the descriptor, SHA-256 prefixes of the tables and of the coefficients
//   bs         the same at 1 thread with a buffer one block too small
//   c0, c64    jb_huff_prepare_ at chunk knob 0 and 64: a SHA-256 prefix over the job
//   d          jb_huff_worth_it_ of c0's job at min_intervals 1 and 16
// The second section ("entry:" rows) walks the twelve jb_decode_memory* / jb_decode_file* entry points.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_internal.h"  // (of the csrc directory the build names: -I)

// ---- stubs for the parts of the library that need a device (prototypes: jb_internal.h, include/jpegblk.h) ----
static std::string g_err, g_route;
static JbKnobs g_knobs;
static int g_job_rc = JB_OK;  // what the device route answers
int jb_fail_(jb_ctx *, int code, const char *msg) {
  g_err = msg ? msg : "";
  return code;
}
void jb_ctx_set_last_desc_(jb_ctx *, const jb_image_desc *d) { g_route += " last=" + std::to_string(d->width) + "x" + std::to_string(d->height); }
const JbKnobs *jb_ctx_knobs_(const jb_ctx *) { return &g_knobs; }
static std::string plan_text(const JbOutPlan &p) {
  return std::to_string(p.out_w) + "x" + std::to_string(p.out_h) + "," + std::to_string((long long)p.image_bytes) + "B,fmt" + std::to_string(p.format);
}
int jb_decode_job_(jb_ctx *, const JbHuffJob *job, uint8_t *, const JbOutPlan &p) {
  g_route += " device(" + plan_text(p) + "," + std::to_string(job->img.n_chunks) + "chunks)";
  return g_job_rc == JB_OK ? JB_OK : jb_fail_(nullptr, g_job_rc, "device route stub");
}
int jb_blocks_to_rgb_plan_(jb_ctx *, const jb_image_desc *, const int16_t *, const uint16_t *, uint8_t *, const JbOutPlan &p) {
  g_route += " host(" + plan_text(p) + ")";
  return JB_OK;
}
extern "C" {
const char *jb_last_error(const jb_ctx *) { return g_err.c_str(); }
void *jb_pinned_alloc(size_t n) { return malloc(n); }
void *jb_pinned_alloc_on(int, size_t n) { return malloc(n); }
int jb_ctx_reserve(jb_ctx *, size_t coef, size_t) {
  g_route += " reserve(" + std::to_string(coef) + ")";
  return JB_OK;
}
int jb_ctx_device(const jb_ctx *) { return 0; }
int jb_ctx_orientation(const jb_ctx *) { return JB_ORIENT_EXIF; }
int jb_ctx_arithmetic(const jb_ctx *) { return JB_ARITH_REFERENCE; }
int jb_ctx_draft(const jb_ctx *) { return 1; }
void jb_pinned_free(void *p) { free(p); }
int jb_device_numa_node(int) { return JB_ERR_STATE; }
}

// ---- SHA-256 (FIPS 180-4) ----
struct Sha256 {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint8_t buf[64];
  uint64_t len = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t *p) {
    static uint32_t k[64];
    if (!k[0]) {  // the fractional parts of the cube roots of the first 64 primes
      int n = 0;
      for (int c = 2; n < 64; c++) {
        bool prime = true;
        for (int d = 2; d * d <= c; d++) prime &= c % d != 0;
        if (prime) {
          const long double r = cbrtl((long double)c);
          k[n++] = (uint32_t)((r - floorl(r)) * 4294967296.0L);
        }
      }
    }
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  }
  void add(const void *data, size_t n) {
    const uint8_t *p = (const uint8_t *)data;
    while (n) {
      if (len % 64 == 0 && n >= 64) {  // whole blocks straight from the data
        block(p);
        p += 64, n -= 64, len += 64;
        continue;
      }
      buf[len++ % 64] = *p++;
      n--;
      if (len % 64 == 0) block(buf);
    }
  }
  template <class T> void add_value(const T &v) { add(&v, sizeof v); }
  std::string hex(int digits = 16) {
    const uint64_t bits = len * 8;
    const uint8_t one = 0x80, zero = 0;
    add(&one, 1);
    while (len % 64 != 56) add(&zero, 1);
    for (int i = 7; i >= 0; i--) {
      const uint8_t b = (uint8_t)(bits >> (8 * i));
      add(&b, 1);
    }
    char s[65];
    for (int i = 0; i < 8; i++) snprintf(s + 8 * i, 9, "%08x", h[i]);
    return std::string(s, (size_t)digits);
  }
};

static std::string desc_text(const jb_image_desc &d) {
  char s[96];
  snprintf(s, sizeof s, "%dx%d,%dx%d,q%d%d%d", d.width, d.height, d.hs, d.vs, d.qtab_id[0], d.qtab_id[1], d.qtab_id[2]);
  return s;
}
static std::string field(const char *call, int rc, const std::string &extra = "") {
  return std::string("\t") + call + "=" + std::to_string(rc) + "|" + (rc ? g_err : "") + (extra.empty() ? "" : "|" + extra);
}

static std::string verdict(const std::vector<uint8_t> &f, bool decode_scan) {
  std::string row;
  jb_image_desc desc;
  uint16_t q[256];
  g_err.clear();
  const int ra = jb_entropy_decode(f.data(), f.size(), &desc, q, nullptr, 0);
  row += field("a", ra, ra ? "" : desc_text(desc));
  jb_geometry g;
  size_t cap = 128;
  if (ra == JB_OK) {
    if (jb_geometry_of(&desc, &g) != JB_OK || g.coef_bytes > (64ll << 20)) {
      row += "\tb=frame too large for a fixture";
      decode_scan = false;
    } else {
      cap = (size_t)g.coef_bytes;
    }
  }
  for (int pass = 0; decode_scan && pass < 3; pass++) {  // 1 thread, 3 threads, one block too small
    const size_t c = pass == 2 ? cap - 128 : cap;
    std::vector<int16_t> coef(c / 2 + 1, (int16_t)0x5555);  // exactly sized on the heap: ASan sees one byte too many
    coef.resize(c / 2);
    coef.shrink_to_fit();
    jb_image_desc d2;
    memset(q, 0, sizeof q);
    g_err.clear();
    const int rc = jb_entropy_decode_mt(f.data(), f.size(), &d2, q, coef.data(), c, pass == 1 ? 3 : 1);
    std::string extra;
    if (rc == JB_OK) {
      Sha256 ht, hc;
      ht.add(q, sizeof q);
      hc.add(coef.data(), c);
      extra = desc_text(d2) + "," + ht.hex() + "," + hc.hex();
    }
    row += field(pass == 0 ? "b1" : pass == 1 ? "b3" : "bs", rc, extra);
  }
  for (uint32_t knob : {0u, 64u}) {
    auto job = std::make_unique<JbHuffJob>();
    std::string text;
    const int rc = jb_huff_prepare_(f.data(), f.size(), job.get(), &text, knob);
    g_err = text;
    std::string extra;
    if (rc == JB_OK) {
      Sha256 h;
      const JbHuffImage &im = job->img;
      h.add_value(job->n_tabs);
      for (uint32_t v : {im.scan_off, im.scan_len, im.int_off, im.n_int, im.ri, im.n_mcus, im.nb, im.table_set, im.lut_ac, im.lut_dc, im.lut_comp,
                         im.n_chunks, im.state_off, im.n_blocks, im.chunk_bytes, im.wg0, im.needs_sync, im.blk_bytes, im.n_tabs})
        h.add_value(v);
      h.add_value(im.coef_off);
      h.add_value(job->desc);
      h.add(job->qtabs, sizeof job->qtabs);
      h.add(job->starts.data(), job->starts.size() * sizeof(uint32_t));
      h.add_value((uint64_t)job->scan_len);
      h.add(job->scan.data(), job->scan.size());
      h.add_value(job->tables);
      extra = std::to_string(im.n_int) + "int," + std::to_string(im.n_chunks) + "chunks," + h.hex();
    }
    row += field(knob ? "c64" : "c0", rc, extra);
    if (!knob) row += std::string("\td=") + (rc ? "-" : jb_huff_worth_it_(*job, 1) ? "1" : "0") + (rc ? "-" : jb_huff_worth_it_(*job, 16) ? "1" : "0");
  }
  return row;
}

static std::vector<uint8_t> unhex(const char *s, size_t n) {
  auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
  std::vector<uint8_t> out(n / 2);
  for (size_t i = 0; i < n / 2; i++) out[i] = (uint8_t)(v(s[2 * i]) << 4 | v(s[2 * i + 1]));
  return out;
}

static bool read_all(const char *path, std::vector<uint8_t> &out) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  uint8_t tmp[65536];
  size_t got;
  while ((got = fread(tmp, 1, sizeof tmp, fp)) > 0) out.insert(out.end(), tmp, tmp + got);
  fclose(fp);
  return true;
}

// ---- the twelve entry points ----
struct Args {
  jb_ctx *ctx;
  const uint8_t *jpeg;
  size_t n;
  const char *path;
  int denom;
  const jb_roi *roi;
  const jb_resize *rs;
  const jb_fit *fit;
  const jb_output_spec *spec;
  void **out;
  int32_t *w, *h;
};
struct Entry {
  const char *name;
  const char *pointers;  // j jpeg, p path, r roi, s resize, f fit, k spec, o out, w width, h height
  std::function<int(const Args &)> call;
};

static void entry_rows(const char *good_path, const char *bad_path) {
  std::vector<uint8_t> good, bad;
  if (!read_all(good_path, good) || !read_all(bad_path, bad)) {
    fprintf(stderr, "cannot read %s or %s\n", good_path, bad_path);
    exit(2);
  }
  const Entry entries[] = {
      {"jb_decode_memory", "jowh", [](const Args &a) { return jb_decode_memory(a.ctx, a.jpeg, a.n, (uint8_t **)a.out, a.w, a.h); }},
      {"jb_decode_memory_scaled", "jowh", [](const Args &a) { return jb_decode_memory_scaled(a.ctx, a.jpeg, a.n, a.denom, (uint8_t **)a.out, a.w, a.h); }},
      {"jb_decode_memory_fmt", "jkowh", [](const Args &a) { return jb_decode_memory_fmt(a.ctx, a.jpeg, a.n, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_memory_roi", "jrkowh", [](const Args &a) { return jb_decode_memory_roi(a.ctx, a.jpeg, a.n, a.roi, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_memory_resized", "jrkowh", [](const Args &a) { return jb_decode_memory_resized(a.ctx, a.jpeg, a.n, a.roi, a.rs->out_w, a.rs->out_h, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_memory_filtered", "jrskowh", [](const Args &a) { return jb_decode_memory_filtered(a.ctx, a.jpeg, a.n, a.roi, a.rs, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_memory_fit", "jrsfkowh", [](const Args &a) { return jb_decode_memory_fit(a.ctx, a.jpeg, a.n, a.roi, a.rs, a.fit, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_file", "powh", [](const Args &a) { return jb_decode_file(a.ctx, a.path, (uint8_t **)a.out, a.w, a.h); }},
      {"jb_decode_file_scaled", "powh", [](const Args &a) { return jb_decode_file_scaled(a.ctx, a.path, a.denom, (uint8_t **)a.out, a.w, a.h); }},
      {"jb_decode_file_fmt", "pkowh", [](const Args &a) { return jb_decode_file_fmt(a.ctx, a.path, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_file_roi", "prkowh", [](const Args &a) { return jb_decode_file_roi(a.ctx, a.path, a.roi, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_file_resized", "prkowh", [](const Args &a) { return jb_decode_file_resized(a.ctx, a.path, a.roi, a.rs->out_w, a.rs->out_h, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_file_filtered", "prskowh", [](const Args &a) { return jb_decode_file_filtered(a.ctx, a.path, a.roi, a.rs, a.spec, a.out, a.w, a.h); }},
      {"jb_decode_file_fit", "prsfkowh", [](const Args &a) { return jb_decode_file_fit(a.ctx, a.path, a.roi, a.rs, a.fit, a.spec, a.out, a.w, a.h); }},
  };
  {
    jb_image_desc d;
    g_err.clear();
    int rc = jb_entropy_decode(nullptr, 0, &d, nullptr, nullptr, 0);
    printf("entry:jb_entropy_decode:NULL j\t%d|%s\n", rc, g_err.c_str());
    g_err.clear();
    rc = jb_entropy_decode_mt(good.data(), good.size(), nullptr, nullptr, nullptr, 0, 3);
    printf("entry:jb_entropy_decode_mt:NULL desc\t%d|%s\n", rc, g_err.c_str());
  }
  static int dummy;
  jb_ctx *const ctx = (jb_ctx *)&dummy;  // (the stubs never look inside it)
  const jb_roi roi = {1, 2, 9, 5};
  const jb_resize rs = {7, 6, 0, 0};
  const jb_fit fit = {JB_FIT_STRETCH, JB_FIT_CENTER, {0, 0, 0}, 0, 0};
  jb_output_spec spec;
  memset(&spec, 0, sizeof spec);
  spec.format = 1;
  jb_output_spec loose = spec;
  loose.plane_stride = 4096;
  for (const Entry &e : entries) {
    const bool from_file = e.pointers[0] == 'p';
    auto run = [&](const std::string &what, Args a, int huffman = -1, int job_rc = JB_OK) {
      void *out = (void *)&dummy;  // (a refusal that leaves *out alone shows as "kept")
      int32_t w = -1, h = -1;
      if (a.out) a.out = &out;
      if (a.w) a.w = &w;
      if (a.h) a.h = &h;
      g_knobs = JbKnobs();
      g_knobs.gpu_huffman = huffman;
      g_job_rc = job_rc;
      g_err.clear();
      g_route.clear();
      const int rc = e.call(a);
      const char *o = out == (void *)&dummy ? "kept" : out ? "set" : "null";
      printf("entry:%s:%s\t%d|%s|out=%s,%dx%d|route:%s\n", e.name, what.c_str(), rc, rc ? g_err.c_str() : "", o, w, h, g_route.c_str());
      if (out != (void *)&dummy) free(out);
    };
    void *o = nullptr;
    int32_t w = 0, h = 0;
    const Args ok = {ctx, good.data(), good.size(), good_path, 1, &roi, &rs, &fit, &spec, &o, &w, &h};
    Args a = ok;
    a.ctx = nullptr;
    run("ctx NULL", a);
    for (const char *p = e.pointers; *p; p++) {
      a = ok;
      switch (*p) {
        case 'j': a.jpeg = nullptr; break;
        case 'p': a.path = nullptr; break;
        case 'r': a.roi = nullptr; break;
        case 's': a.rs = nullptr; break;
        case 'f': a.fit = nullptr; break;
        case 'k': a.spec = nullptr; break;
        case 'o': a.out = nullptr; break;
        case 'w': a.w = nullptr; break;
        case 'h': a.h = nullptr; break;
      }
      run(std::string("NULL ") + *p, a);
      a.ctx = nullptr;  // ... and which of the two is reported first
      run(std::string("ctx NULL, NULL ") + *p, a);
    }
    for (int denom : {0, 2, 3}) {
      a = ok;
      a.denom = denom;
      run("denom " + std::to_string(denom), a);
    }
    a = ok;
    a.spec = &loose;
    run("loose spec", a);
    a.out = nullptr;
    run("loose spec, NULL o", a);
    if (from_file) {
      a = ok;
      a.path = "/nonexistent/frontend_verdicts.jpg";
      run("no such file", a);
      a.spec = &loose;
      run("no such file, loose spec", a);
    }
    for (int huffman : {-1, 0, 1, 2})
      for (int job_rc : {(int)JB_OK, (int)JB_ERR_FORMAT, (int)JB_ERR_HIP}) {
        const std::string tag = "huffman " + std::to_string(huffman) + ", device answers " + std::to_string(job_rc);
        run("good file, " + tag, ok, huffman, job_rc);
        a = ok;
        a.jpeg = bad.data(), a.n = bad.size(), a.path = bad_path;
        run("corrupt file, " + tag, a, huffman, job_rc);
      }
  }
}

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s <cases file> <good.jpg> <corrupt.jpg>\n", argv[0]);
    return 2;
  }
  FILE *fp = fopen(argv[1], "r");
  if (!fp) return 2;
  std::map<std::string, std::vector<uint8_t>> seeds;
  char *line = nullptr;
  size_t cap = 0;
  ssize_t len;
  while ((len = getline(&line, &cap, fp)) > 0) {
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    if (len < 3) continue;
    // the name may hold blanks: fields are separated by tabs
    std::vector<char *> tok;
    for (char *t = strtok(line, "\t"); t; t = strtok(nullptr, "\t")) tok.push_back(t);
    if (tok.size() < 2) return 2;
    if (tok[0][0] == 'S') {
      seeds[tok[1]] = tok.size() > 2 ? unhex(tok[2], strlen(tok[2])) : std::vector<uint8_t>();
      continue;
    }
    std::vector<uint8_t> f;
    if (tok[0][0] == 'B') {
      if (tok.size() > 2) f = unhex(tok[2], strlen(tok[2]));
    } else {
      if (tok.size() < 4 || !seeds.count(tok[2])) return 2;
      f = seeds[tok[2]];
      f.resize((size_t)atol(tok[3]) <= f.size() ? (size_t)atol(tok[3]) : f.size());
      for (size_t i = 4; i < tok.size(); i++) {
        char *colon = strchr(tok[i], ':');
        if (!colon) return 2;
        const std::vector<uint8_t> patch = unhex(colon + 1, strlen(colon + 1));
        const size_t at = (size_t)atol(tok[i]);
        if (at + patch.size() > f.size()) return 2;
        memcpy(f.data() + at, patch.data(), patch.size());
      }
    }
    f.shrink_to_fit();
    printf("%s%s\n", tok[1], verdict(f, tok[0][0] != 'H').c_str());
  }
  free(line);
  fclose(fp);
  if (strcmp(argv[2], "-") != 0) entry_rows(argv[2], argv[3]);
  return 0;
}
