// views_kernel_check -- the bodies of the two view kernels (csrc/jb_resample.hip: jb_resample_kernel and jb_filter_kernel
// in their kViews instantiations) compiled for the CPU: the HIP built-ins they use are stubbed below, a launch is a loop
// over the block index, and a workgroup is 256 host threads that meet at a barrier where the kernel has one.  Built with
// AddressSanitizer + UBSan; the scratch (the unions, back to back, + 4 bytes: less than the slack the seam leaves), the
// destination and the LDS are heap blocks of exactly the promised size, so any access outside them is a report.  The
// last view's source ends on the last pixel of the scratch.  Expected values: the header's definitions written out
// per pixel, then the mirror.
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define JB_KERNELS_HOST
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
struct HostIdx {
  unsigned x;
};
static thread_local HostIdx threadIdx, blockIdx;
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static pthread_barrier_t host_barrier;
static int32_t *host_lds = nullptr;
#define JB_DYNAMIC_LDS(name) int32_t *const name = host_lds
static inline void __syncthreads() { pthread_barrier_wait(&host_barrier); }
using std::max;
using std::min;
struct HostRsrc {
  const uint8_t *base;
  int range;
};
typedef HostRsrc __amdgpu_buffer_rsrc_t;
static inline HostRsrc host_make_rsrc(uint8_t *p, int, int range, int) { return HostRsrc{p, range}; }
// a raw buffer load: 0 beyond the descriptor's range, else the bytes -- read for real, so that a range that promises
// more than the allocation holds is a sanitizer report
static inline uint32_t host_load_b32(HostRsrc r, int off, int, int) {
  if (off < 0 || off + 4 > r.range) return 0;
  uint32_t v;
  memcpy(&v, r.base + off, 4);
  return v;
}
// binary16 where the host compiler has no _Float16: float -> half, round to nearest even (the device's one convert)
struct HostHalf {
  uint16_t bits;
  explicit HostHalf(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) bits = (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0));
    else if (mag >= 0x477ff000u) bits = (uint16_t)(sign | 0x7c00u);
    else if (mag < 0x33000001u) bits = (uint16_t)sign;
    else {
      const int e = (int)(mag >> 23) - 127;
      const uint32_t sig = (mag & 0x7fffffu) | 0x800000u;
      const int shift = e >= -14 ? 13 : 13 + (-14 - e);
      const uint32_t kept = sig >> shift, rest = sig & ((1u << shift) - 1), half = 1u << (shift - 1);
      uint32_t h = e >= -14 ? ((uint32_t)(e + 15) << 10) + (kept - 0x400u) : kept;
      if (rest > half || (rest == half && (h & 1))) h++;
      bits = (uint16_t)(sign | h);
    }
  }
};
#define _Float16 HostHalf
#define __builtin_amdgcn_make_buffer_rsrc host_make_rsrc
#define __builtin_amdgcn_raw_buffer_load_b32 host_load_b32
#define __builtin_amdgcn_readfirstlane(x) (x)
#include "../../jpeg_decoder_amd/csrc/jb_resample.hip"

static const uint8_t kSent = 0xA5;
static long n_cases = 0;
static const float kScale[3] = {1.0f / (255.0f * 0.229f), 1.0f / 255.0f, 1.0f + 1.0f / 2048.0f}, kBias[3] = {-0.485f / 0.229f, 0.0f, 0.25f};

// ---- a launch: `blocks` workgroups of `threads` host threads -------------------------------------------------------------
struct Launch {
  void (*body)(const void *args);
  const void *args;
  unsigned blocks, threads;
  size_t lds_bytes;
};
struct Worker {
  const Launch *l;
  unsigned tid;
};
static void *worker(void *arg) {
  const Worker *w = (const Worker *)arg;
  for (unsigned b = 0; b < w->l->blocks; b++) {
    if (w->tid == 0) host_lds = w->l->lds_bytes ? (int32_t *)malloc(w->l->lds_bytes) : nullptr;  // exactly what the launch asked for
    pthread_barrier_wait(&host_barrier);
    threadIdx.x = w->tid, blockIdx.x = b;
    w->l->body(w->l->args);
    pthread_barrier_wait(&host_barrier);
    if (w->tid == 0) free(host_lds);
  }
  return nullptr;
}
static void run(const Launch &l) {
  pthread_barrier_init(&host_barrier, nullptr, l.threads);
  std::vector<pthread_t> th(l.threads);
  std::vector<Worker> w(l.threads);
  for (unsigned t = 0; t < l.threads; t++) {
    w[t] = Worker{&l, t};
    if (pthread_create(&th[t], nullptr, worker, &w[t]) != 0) {
      printf("FAIL: cannot start a thread\n");
      exit(1);
    }
  }
  for (unsigned t = 0; t < l.threads; t++) pthread_join(th[t], nullptr);
  pthread_barrier_destroy(&host_barrier);
}

struct AreaArgs {
  JbResample p;
  JbViewTable t;
};
template <int FORMAT>
static void area_body(const void *a) {
  const AreaArgs *x = (const AreaArgs *)a;
  jb_resample_kernel<FORMAT, kViews, JbViewTable>(x->p, x->t);
}
struct FilterArgs {
  JbFilter q;
  JbViewFilterTable t;
};
template <int FILTER, int FORMAT>
static void filter_body(const void *a) {
  const FilterArgs *x = (const FilterArgs *)a;
  jb_filter_kernel<FILTER, FORMAT, kViews, JbViewFilterTable>(x->q, x->t);
}

// ---- the definitions of include/jpegblk.h, per pixel -----------------------------------------------------------------------
struct Rect {
  int x, y, w, h;
};
// "fixed output size": the exact area resize of frame[r.y.., r.x..] to ow x oh
static void area_ref(const std::vector<uint8_t> &frame, int fw, const Rect &r, int ow, int oh, std::vector<uint8_t> &out) {
  out.assign((size_t)3 * ow * oh, 0);
  const int64_t iw = r.w, ih = r.h, d = iw * ih;
  for (int k = 0; k < oh; k++)
    for (int j = 0; j < ow; j++)
      for (int c = 0; c < 3; c++) {
        int64_t s = 0;
        for (int64_t rr = 0; rr < ih; rr++) {
          const int64_t wy = std::min<int64_t>((rr + 1) * oh, (k + 1) * ih) - std::max<int64_t>(rr * oh, k * ih);
          if (wy <= 0) continue;
          for (int64_t i = 0; i < iw; i++) {
            const int64_t wx = std::min<int64_t>((i + 1) * ow, (j + 1) * iw) - std::max<int64_t>(i * ow, j * iw);
            if (wx > 0) s += wy * wx * frame[((size_t)(r.y + rr) * fw + (size_t)(r.x + i)) * 3 + c];
          }
        }
        out[((size_t)k * ow + j) * 3 + c] = (uint8_t)((s + d / 2) / d);
      }
}
// "resampling filters": Pillow's two passes over the whole frame, weights by jb_filter.h's arithmetic
static void axis_weights(int filter, int in_size, int in0, int in1, int n, std::vector<int> &lo, std::vector<std::vector<int32_t>> &k) {
  const JbFilterAxis a = jb_filter_axis(filter, in_size, in0, in1, n);
  lo.resize(n), k.resize(n);
  for (int j = 0; j < n; j++) {
    double c;
    int l, h;
    jb_filter_bounds(a, j, &c, &l, &h);
    std::vector<double> w(h - l);
    double ww = 0.0;
    for (int t = 0; t < h - l; t++) w[t] = jb_filter_weight(a, l, c, t), ww += w[t];
    lo[j] = l, k[j].resize(h - l);
    for (int t = 0; t < h - l; t++) k[j][t] = jb_filter_fixed(ww != 0.0 ? w[t] / ww : w[t]);
  }
}
static int clip_u8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static void filter_ref(const std::vector<uint8_t> &frame, int fw, int fh, const Rect &r, int ow, int oh, int filter, std::vector<uint8_t> &out) {
  std::vector<int> lox, loy;
  std::vector<std::vector<int32_t>> kx, ky;
  axis_weights(filter, fw, r.x, r.x + r.w, ow, lox, kx);
  axis_weights(filter, fh, r.y, r.y + r.h, oh, loy, ky);
  std::vector<uint8_t> T((size_t)3 * fh * ow);
  for (int y = 0; y < fh; y++)
    for (int j = 0; j < ow; j++)
      for (int c = 0; c < 3; c++) {
        int s = 1 << 21;
        for (size_t t = 0; t < kx[j].size(); t++) s += kx[j][t] * frame[((size_t)y * fw + lox[j] + t) * 3 + c];
        T[((size_t)y * ow + j) * 3 + c] = (uint8_t)clip_u8(s >> 22);
      }
  out.assign((size_t)3 * ow * oh, 0);
  for (int k = 0; k < oh; k++)
    for (int j = 0; j < ow; j++)
      for (int c = 0; c < 3; c++) {
        int s = 1 << 21;
        for (size_t t = 0; t < ky[k].size(); t++) s += ky[k][t] * T[((size_t)(loy[k] + t) * ow + j) * 3 + c];
        out[((size_t)k * ow + j) * 3 + c] = (uint8_t)clip_u8(s >> 22);
      }
}

// ---- one case: two images of K = 3 views each, their unions back to back in an exactly-sized scratch -------------------------
static void one(int filter, int fmt, int ow, int oh, bool mirror, int pad_row, int pad_plane, int pad_img) {
  const int fw = 90, fh = 40, K = 3, N = 2;
  std::vector<uint8_t> frame[N];
  for (int i = 0; i < N; i++) {
    frame[i].resize((size_t)3 * fw * fh);
    for (size_t b = 0; b < frame[i].size(); b++) frame[i][b] = (uint8_t)((b * 131 + (b >> 8) * 7 + 1 + 77 * i) ^ (b % 7 == 0 ? 0xff : 0));
  }
  // image 0: the whole frame, one pixel, a thin strip; image 1: disjoint corners and a view that ends the union (and so
  // the scratch): its last source pixel is the scratch's last pixel
  Rect views[N][K] = {{{0, 0, fw, fh}, {89, 39, 1, 1}, {1, 20, 88, 1}}, {{3, 2, 20, 10}, {40, 5, 7, 30}, {60, 25, 30, 15}}};
  if (filter) views[0][0] = Rect{0, 0, 39, 39}, views[0][2] = Rect{1, 20, 38, 1};  // (the tap cap: a 1 x 1 target reduces at most 39x)
  Rect src[N][K], uni[N];
  for (int i = 0; i < N; i++) {
    int x0 = 1 << 30, y0 = 1 << 30, x1 = 0, y1 = 0;
    for (int v = 0; v < K; v++) {
      src[i][v] = views[i][v];
      if (filter) {
        int a, b, c, d;
        jb_filter_span(jb_filter_axis(filter, fw, views[i][v].x, views[i][v].x + views[i][v].w, ow), ow, &a, &b);
        jb_filter_span(jb_filter_axis(filter, fh, views[i][v].y, views[i][v].y + views[i][v].h, oh), oh, &c, &d);
        src[i][v] = Rect{a, c, b - a, d - c};
      }
      x0 = std::min(x0, src[i][v].x), y0 = std::min(y0, src[i][v].y);
      x1 = std::max(x1, src[i][v].x + src[i][v].w), y1 = std::max(y1, src[i][v].y + src[i][v].h);
    }
    uni[i] = Rect{x0, y0, x1 - x0, y1 - y0};
  }
  int64_t offset[N], total = 0;
  for (int i = 0; i < N; i++) offset[i] = total, total += 3LL * uni[i].w * uni[i].h;
  uint8_t *scratch = (uint8_t *)malloc((size_t)total + 4);
  memset(scratch, 0x5a, (size_t)total + 4);
  for (int i = 0; i < N; i++)
    for (int y = 0; y < uni[i].h; y++)
      memcpy(scratch + offset[i] + (size_t)3 * uni[i].w * y, &frame[i][((size_t)(uni[i].y + y) * fw + uni[i].x) * 3], (size_t)3 * uni[i].w);

  const int es = fmt == 2 ? 4 : fmt == 3 ? 2 : 1, n_out = N * K;
  const int64_t row = fmt == 0 ? 3LL * ow + pad_row : ((int64_t)ow + pad_row) * es;
  const int64_t plane = fmt == 0 ? 0 : row * oh + (int64_t)pad_plane * es;
  const int64_t img = fmt == 0 ? row * oh + pad_img : 3 * plane + (int64_t)pad_img * es;
  const size_t dst_bytes = (size_t)((n_out - 1) * img + (fmt == 0 ? (oh - 1) * row + 3LL * ow : 2 * plane + (oh - 1) * row + (int64_t)ow * es));
  uint8_t *dst = (uint8_t *)malloc(dst_bytes), *want = (uint8_t *)malloc(dst_bytes);
  memset(dst, kSent, dst_bytes);
  memset(want, kSent, dst_bytes);

  JbResample p;
  memset(&p, 0, sizeof p);
  p.src = scratch, p.dst = dst;
  p.dst_image_stride = img, p.dst_row_stride = row, p.dst_plane_stride = plane;
  p.ow = ow, p.oh = oh, p.n_images = n_out;
  for (int c = 0; c < 3; c++) p.scale[c] = kScale[c], p.bias[c] = kBias[c];
  const auto flag = [&](int n) { return mirror && n != 3; };  // (one unmirrored row inside a mirrored launch)
  if (!filter) {
    AreaArgs a;
    memset(&a, 0, sizeof a);
    a.p = p;
    for (int n = 0; n < n_out; n++) {
      const int i = n / K, v = n % K;
      a.t.r[n] = JbViewRow{offset[i], 3 * uni[i].w, views[i][v].x - uni[i].x, views[i][v].y - uni[i].y, views[i][v].w, views[i][v].h, flag(n) ? 1 : 0};
    }
    dim3 grid;
    if (!resample_args_ok(a.p, fmt, kJbCropsPerLaunch) || !rows_ok(a.t, n_out)) {
      printf("FAIL: the launch validation refuses format %d target %dx%d\n", fmt, ow, oh);
      exit(1);
    }
    if (!resample_grid(a.p, &grid)) exit(2);
    void (*const bodies[4])(const void *) = {area_body<0>, area_body<1>, area_body<2>, area_body<3>};
    run(Launch{bodies[fmt], &a, grid.x, 64u * kResampleRows, 0});
  } else {
    FilterArgs a;
    memset(&a, 0, sizeof a);
    a.q.base = p;
    a.q.frame_w = fw, a.q.frame_h = fh;
    for (int n = 0; n < n_out; n++) {
      const int i = n / K, v = n % K;
      a.t.r[n] = JbFilterRow{views[i][v].x, views[i][v].y, views[i][v].w, views[i][v].h, uni[i].x, uni[i].y, uni[i].w, uni[i].h, offset[i]};
      if (flag(n)) a.t.mirror |= 1u << n;
    }
    dim3 grid;
    const size_t lds = resample_args_ok(a.q.base, fmt, kJbCropsPerLaunch) ? filter_plan(a.q, a.t.r, n_out, filter, &grid, true) : 0;
    if (!lds) {
      printf("FAIL: filter_plan refuses filter %d target %dx%d\n", filter, ow, oh);
      exit(1);
    }
    void (*const bodies[2][4])(const void *) = {{filter_body<1, 0>, filter_body<1, 1>, filter_body<1, 2>, filter_body<1, 3>},
                                                 {filter_body<2, 0>, filter_body<2, 1>, filter_body<2, 2>, filter_body<2, 3>}};
    run(Launch{bodies[filter - 1][fmt], &a, grid.x, 256u, lds});
  }

  for (int n = 0; n < n_out; n++) {
    const int i = n / K, v = n % K;
    std::vector<uint8_t> u;
    if (filter) filter_ref(frame[i], fw, fh, views[i][v], ow, oh, filter, u);
    else area_ref(frame[i], fw, views[i][v], ow, oh, u);
    for (int y = 0; y < oh; y++)
      for (int x = 0; x < ow; x++)
        for (int c = 0; c < 3; c++) {
          const uint8_t px = u[((size_t)y * ow + (flag(n) ? ow - 1 - x : x)) * 3 + c];  // the mirror, LAST
          uint8_t *at = want + n * img + y * row + (fmt == 0 ? 3 * x + c : c * plane + (int64_t)x * es);
          volatile float prod = (float)px * kScale[c];
          const float f = prod + kBias[c];
          if (es == 1) *at = px;
          else if (es == 4) memcpy(at, &f, 4);
          else {
            const _Float16 hf = (_Float16)f;
            memcpy(at, &hf, 2);
          }
        }
  }
  if (memcmp(dst, want, dst_bytes) != 0) {
    size_t at = 0;
    while (dst[at] == want[at]) at++;
    printf("FAIL: filter %d format %d target %dx%d mirror %d: byte %zu of %zu is %d, want %d\n", filter, fmt, ow, oh, (int)mirror, at, dst_bytes,
           dst[at], want[at]);
    exit(1);
  }
  free(scratch), free(dst), free(want);
  n_cases++;
}

// ---- the launchers' checks (jb_resample.hip: resample_args_ok, view_row_ok, crop_row_ok) -----------------------------------
// From one accepted launch of two rows, every one of these changes alone -- to the SECOND row, so that the loops are seen
// to reach it -- must be refused.
static long n_validation = 0;
static void expect(bool accepted, bool want, const char *what) {
  if (accepted != want) {
    printf("FAIL: the launch validation %s %s\n", accepted ? "accepts" : "refuses", what);
    exit(1);
  }
  n_validation++;
}
static void validation() {
  JbResample p;
  JbViewTable vt;
  JbCropTable ct;
  memset(&p, 0, sizeof p);
  memset(&vt, 0, sizeof vt);
  memset(&ct, 0, sizeof ct);
  p.ow = 70, p.oh = 9, p.n_images = 2;
  for (int i = 0; i < 2; i++) {
    vt.r[i] = JbViewRow{8100LL * i, 3 * 90, 3, 2, 20, 10, i};  // a 20 x 10 view at (3, 2) of a union 90 wide
    ct.c[i].w = 20, ct.c[i].h = 10, ct.c[i].tmp_offset = 600LL * i;
  }
  expect(resample_args_ok(p, 0, kJbCropsPerLaunch) && resample_args_ok(p, 3, kJbCropsPerLaunch) && rows_ok(vt, 2) && rows_ok(ct, 2), true,
         "the launch the refused ones are made from");
  const auto view = [&](const char *what, auto change) {
    JbViewTable t = vt;
    change(t.r[1]);
    expect(rows_ok(t, 2), false, what);
  };
  view("a view row with w = 0", [](JbViewRow &r) { r.w = 0; });
  view("a view row with h = 0", [](JbViewRow &r) { r.h = 0; });
  view("a view row with w = 65536", [](JbViewRow &r) { r.w = 65536; });
  view("a view row with dx = -1", [](JbViewRow &r) { r.dx = -1; });
  view("a view row with dy = -1", [](JbViewRow &r) { r.dy = -1; });
  view("a view row with dy = 65536", [](JbViewRow &r) { r.dy = 65536; });
  view("a view row with src_offset = -1", [](JbViewRow &r) { r.src_offset = -1; });
  view("a view row with src_row_bytes = 3 * 65535 + 1", [](JbViewRow &r) { r.src_row_bytes = 3 * 65535 + 1; });
  view("a view row with 3 * (dx + w) = src_row_bytes + 3", [](JbViewRow &r) { r.dx = r.src_row_bytes / 3 - r.w + 1; });
  view("a view row with mirror = 2", [](JbViewRow &r) { r.mirror = 2; });
  const auto crop = [&](const char *what, auto change) {
    JbCropTable t = ct;
    change(t.c[1]);
    expect(rows_ok(t, 2), false, what);
  };
  crop("a crop row with w = 0", [](JbCrop &c) { c.w = 0; });
  crop("a crop row with h = 0", [](JbCrop &c) { c.h = 0; });
  crop("a crop row with w = 65536", [](JbCrop &c) { c.w = 65536; });
  crop("a crop row with tmp_offset = -1", [](JbCrop &c) { c.tmp_offset = -1; });
  const auto launch = [&](const char *what, int format, auto change) {
    JbResample q = p;
    change(q);
    expect(resample_args_ok(q, format, kJbCropsPerLaunch), false, what);
  };
  launch("format = -1", -1, [](JbResample &) {});
  launch("format = 4", 4, [](JbResample &) {});
  launch("ow = 0", 0, [](JbResample &q) { q.ow = 0; });
  launch("ow = 65536", 0, [](JbResample &q) { q.ow = 65536; });
  launch("n_images = 0", 0, [](JbResample &q) { q.n_images = 0; });
  launch("n_images = kJbCropsPerLaunch + 1", 0, [](JbResample &q) { q.n_images = kJbCropsPerLaunch + 1; });
}

int main() {
  const int targets[][2] = {{1, 1}, {1, 5}, {64, 3}, {65, 3}, {70, 9}};
  for (int filter = 0; filter <= 2; filter++)
    for (int fmt = 0; fmt < 4; fmt++)
      for (const auto &t : targets)
        for (int mirror = 0; mirror < 2; mirror++) {
          one(filter, fmt, t[0], t[1], mirror != 0, 0, 0, 0);
          if (t[0] == 70) one(filter, fmt, t[0], t[1], mirror != 0, 1, 5, 7);
        }
  printf("%ld view kernel cases ok\n", n_cases);
  validation();
  printf("%ld launch validation cases ok\n", n_validation);
  return 0;
}
