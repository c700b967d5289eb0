// jb_hostutil.cpp -- host helpers that need no HIP: the PPM / BMP writers and jb_free of include/jpegblk.h, file
// reading, the clock, the CPUs this process may use (affinity mask, cgroup quota, NUMA node of a device) and the check
// of an output spec that has no strides to be checked against yet.  Plain C++: tools/fuzz builds this file for the CPU
// with the sanitizers, next to the front end.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include <sched.h>
#include <sys/stat.h>

#include "jb_internal.h"

namespace {

int failf(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return jb_fail_(nullptr, code, buf);
}

}  // namespace

extern "C" {

void jb_free(void *p) { free(p); }

int jb_write_ppm(const char *path, const uint8_t *rgb, int32_t width, int32_t height, int64_t rgb_stride) {
  if (!path || !rgb) return failf(JB_ERR_NULL, "jb_write_ppm: NULL pointer");
  if (width < 1 || height < 1 || rgb_stride < 3LL * width) return failf(JB_ERR_GEOMETRY, "jb_write_ppm: bad geometry");
  FILE *f = fopen(path, "wb");
  if (!f) return failf(JB_ERR_FORMAT, "cannot open %s for writing", path);
  fprintf(f, "P6\n%d %d\n255\n", width, height);
  for (int y = 0; y < height; y++)
    if (fwrite(rgb + (int64_t)y * rgb_stride, 1, (size_t)width * 3, f) != (size_t)width * 3) {
      fclose(f);
      return failf(JB_ERR_FORMAT, "short write to %s", path);
    }
  fclose(f);
  return JB_OK;
}

int jb_write_bmp(const char *path, const uint8_t *rgb, int32_t width, int32_t height, int64_t rgb_stride) {
  if (!path || !rgb) return failf(JB_ERR_NULL, "jb_write_bmp: NULL pointer");
  if (width < 1 || height < 1 || rgb_stride < 3LL * width) return failf(JB_ERR_GEOMETRY, "jb_write_bmp: bad geometry");
  const int64_t row_bytes = (3LL * width + 3) & ~3LL;  // rows are padded to 4 bytes
  const int64_t file_bytes = 54 + row_bytes * height;
  if (file_bytes > 0xffffffffLL) return failf(JB_ERR_CAPACITY, "jb_write_bmp: %dx%d exceeds the 4 GiB BMP limit", width, height);
  FILE *f = fopen(path, "wb");
  if (!f) return failf(JB_ERR_FORMAT, "cannot open %s for writing", path);
  uint8_t hdr[54] = {'B', 'M'};
  auto le32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; i++) hdr[at + i] = (uint8_t)(v >> (8 * i)); };
  le32(2, (uint32_t)file_bytes);
  le32(10, 54);                    // offset of the pixel array
  le32(14, 40);                    // BITMAPINFOHEADER
  le32(18, (uint32_t)width);
  le32(22, (uint32_t)height);      // positive: bottom-up
  hdr[26] = 1;                     // planes
  hdr[28] = 24;                    // bits per pixel; compression 0 (BI_RGB)
  le32(34, (uint32_t)(row_bytes * height));
  le32(38, 2835);                  // 72 dpi
  le32(42, 2835);
  bool ok = fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr;
  std::vector<uint8_t> row((size_t)row_bytes, 0);
  for (int y = height - 1; ok && y >= 0; y--) {
    const uint8_t *src = rgb + (int64_t)y * rgb_stride;
    for (int x = 0; x < width; x++) {
      row[3 * x + 0] = src[3 * x + 2];
      row[3 * x + 1] = src[3 * x + 1];
      row[3 * x + 2] = src[3 * x + 0];
    }
    ok = fwrite(row.data(), 1, row.size(), f) == row.size();
  }
  if (fclose(f) != 0) ok = false;
  return ok ? JB_OK : failf(JB_ERR_FORMAT, "short write to %s", path);
}

}  // extern "C"

double jb_now_s_() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// A regular file is read in one piece of its size (a batch reads thousands of them); anything else that opens -- a
// pipe, a device -- in chunks until it ends.
bool jb_read_file_(const char *path, std::vector<uint8_t> &buf) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  struct stat st;
  bool ok;
  if (fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode)) {
    const size_t n = (size_t)st.st_size;
    buf.resize(n);
    ok = (n ? fread(buf.data(), 1, n, f) : 0) == n;
  } else {
    buf.clear();
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    ok = ferror(f) == 0;
  }
  fclose(f);
  return ok;
}

bool jb_read_prefix_(const char *path, size_t limit, std::vector<uint8_t> &buf, bool *whole) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  buf.resize(limit + 1);
  const size_t got = fread(buf.data(), 1, limit + 1, f);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return false;
  *whole = got <= limit;
  buf.resize(got < limit ? got : (*whole ? got : limit));
  return true;
}

int jb_cpu_quota_(bool *fraction) {
  long quota = -1, period = 100000;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    if (fscanf(f, "%31s %ld", q, &period) >= 1 && strcmp(q, "max") != 0) quota = atol(q);
    fclose(f);
  } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    if (fscanf(g, "%ld", &quota) != 1) quota = -1;
    fclose(g);
    if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(h, "%ld", &period) != 1) period = 100000;
      fclose(h);
    }
  }
  const bool have = quota > 0 && period > 0;
  if (fraction) *fraction = have && quota % period != 0;
  return have ? (int)(quota / period) : 0;
}

// More entropy threads than that only time-slice against each other and against the HIP runtime's own threads: measured
// on a 16-CPU quota, 24-32 threads halved the rate of 16 (8192x8192: 187 -> 98-110 images/s).
int jb_available_cpus_() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (n < 1) n = (int)std::thread::hardware_concurrency();
  if (n < 1) n = 1;
  bool fraction = false;
  const int by_quota = jb_cpu_quota_(&fraction) + (fraction ? 1 : 0);  // (a part of a CPU counts as one)
  if (by_quota >= 1 && by_quota < n) n = by_quota;
  return n;
}

// which CPUs the threads of a decoder on `device` are bound to (n = 0: none): worked out once per (device, knob) --
// sysfs, the cgroup quota and the affinity mask of the first caller, 16 threads of every pass of every run asked for
// them again -- then only applied
static int numa_cpus_for_(int device, int numa_knob, cpu_set_t *out) {
  if (numa_knob == 0) return 0;
  const bool forced = numa_knob == 1;
  const int node = jb_device_numa_node(device);
  if (node < 0) return 0;
  char path[96];
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return 0;
  char list[4096] = {0};
  const bool got = fgets(list, sizeof list, f) != nullptr;
  fclose(f);
  if (!got) return 0;
  cpu_set_t cur, want;
  if (sched_getaffinity(0, sizeof cur, &cur) != 0) return 0;
  CPU_ZERO(&want);
  int n = 0;
  for (char *p = list; *p;) {  // "0-15,128-143"
    char *end;
    long a = strtol(p, &end, 10), b = a;
    if (end == p) break;
    if (*end == '-') b = strtol(end + 1, &end, 10);
    for (long c = a; c <= b && c < CPU_SETSIZE; c++)
      if (c >= 0 && CPU_ISSET((int)c, &cur)) {
        CPU_SET((int)c, &want);
        n++;
      }
    p = (*end == ',') ? end + 1 : end;
    if (*end != ',') break;
  }
  if (n == 0 || n == CPU_COUNT(&cur)) return 0;  // nothing to narrow
  // Only where the process owns at least a node's worth of CPU time (a rank of a dedicated node).
  // Under a cgroup CPU quota smaller than the node -- a share of a machine other tenants use too --
  // the scheduler does better unpinned: measured on a 16-CPU share of a 256-CPU box, 16 entropy
  // threads on 8192x8192 files: 139 images/s free, 114 bound to the GPU's node (JPEGBLK_NUMA=1 forces).
  if (!forced) {
    bool fraction = false;
    const int quota = jb_cpu_quota_(&fraction);  // (rounded down: 15.5 CPUs are less than a node of 16)
    if ((quota > 0 || fraction) && quota < n) return 0;
  }
  *out = want;
  return n;
}

// Bind the calling host thread to the CPUs of the NUMA node closest to `device` (intersected with
// the CPUs the thread may already use; nothing changes when the node is unknown, the intersection
// is empty, or JPEGBLK_NUMA=0).  The entropy threads of one rank then read their files, decode and
// write their pinned staging on the socket their GPU hangs off.  Returns the CPUs in the new mask,
// 0 = left as it was.
int jb_bind_thread_near_device_(int device, int numa_knob) {  // numa_knob: JbKnobs::numa of the calling decoder
  struct Entry {
    int n;
    cpu_set_t set;
  };
  static std::mutex mu;
  static std::map<std::pair<int, int>, Entry> cache;
  Entry e;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({device, numa_knob});
    if (it == cache.end()) {
      Entry fresh;
      CPU_ZERO(&fresh.set);
      fresh.n = numa_cpus_for_(device, numa_knob, &fresh.set);
      it = cache.emplace(std::make_pair(device, numa_knob), fresh).first;
    }
    e = it->second;
  }
  if (e.n <= 0) return 0;
  if (sched_setaffinity(0, sizeof e.set, &e.set) != 0) return 0;
  return e.n;
}

int jb_tight_spec_check_(const jb_output_spec *spec) {
  if (jb_output_spec_check(spec, 1, 1 << 20) != JB_OK || (spec->format != JB_FMT_RGB_U8_HWC && spec->plane_stride != 0)) return JB_ERR_GEOMETRY;
  return JB_OK;
}
