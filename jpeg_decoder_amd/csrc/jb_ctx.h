// jb_ctx.h -- the context behind the C ABI, as the two files see it that drive HIP for it: jb_api.cpp (the staging
// ring, the download engine, the submissions) and jb_seam.cpp (the pixel launch of every route).  Private, with HIP
// types: nothing else includes it (what other files may call is declared in jb_internal.h).
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>

#include <hip/hip_runtime_api.h>

#include "jb_internal.h"

struct Slot {
  void *d_coef = nullptr;
  void *d_rgb = nullptr;
  int32_t *h_q = nullptr;  // pinned int32[3][64]
  int32_t *d_q = nullptr;
  // device-side entropy decoding (jb_huff.hip): the submission's packed scans, interval tables and
  // Huffman table sets (pinned host copy + device copy), and one status word per image
  uint8_t *h_blob = nullptr;
  size_t h_blob_cap = 0;
  void *d_blob = nullptr;
  size_t blob_cap = 0;
  uint32_t *h_status = nullptr;  // pinned, kMaxBatch words
  uint32_t *d_status = nullptr;
  int n_status = 0;              // images of the submission in flight whose status words must be checked
  hipEvent_t computed = nullptr;  // kernel finished (upload stream) -> the download may start
  hipEvent_t done = nullptr;      // pixels are in the caller's buffer
  // a download that the context's download thread has not issued yet (see jb_ctx::dl_*): `done` is only recorded
  // once it has, so whoever waits for the slot waits for this to clear first
  std::atomic<int> dl_pending{0};
  bool busy = false;
  int ticket = -1;
};

struct DlEngine;  // the device's download engine (jb_api.cpp)

struct jb_ctx {
  int device = 0;
  JbKnobs knobs;                  // the environment as it was when the context was created (jb_knobs.h)
  hipStream_t stream = nullptr;   // primary: uploads + kernels of the ring; device-resident launches with a NULL stream
  hipStream_t stream2 = nullptr;  // downloads of the staging ring
  // Submissions whose entropy stage runs on the device: a decoder launch is latency-bound (a lane
  // walks its interval's blocks one after the other: milliseconds, whatever the group size), so
  // several of them must be in flight at once; each such submission runs whole on one of these.
  static constexpr int kPool = 16;
  hipStream_t pool[kPool] = {};
  // Single-image submissions of host coefficients: K independent (upload + kernel, download) stream
  // pairs used in turn -- pair 0 is (stream, stream2).  Within a pair the download of image i
  // overlaps the upload of image i + K (the link runs both ways); across pairs the chains of
  // different submitters do not queue behind each other.
  // Measured with 16 submitting threads (profiles/r02b/ab_stream_pairs.txt): 1080p images (19 MB
  // per submission) 1,951 images/s with one pair, 2,631 with eight; 8192x8192 images (402 MB) 164
  // with one pair, 91 with eight -- several large copies in one direction at a time share the link
  // badly -- so submissions of 64 MB or more all use pair 0.
  static constexpr int kMaxPairs = 8;
  static constexpr size_t kLargeSubmission = (size_t)64 << 20;
  int n_pairs = 8;
  hipStream_t pair_up[kMaxPairs] = {}, pair_down[kMaxPairs] = {};
  unsigned n_single_submits = 0;
  unsigned n_group_submits = 0;
  size_t max_coef = 0, max_rgb = 0, rgb_alloc = 0;
  int n_slots = 0;
  int n_slots_req = 1;  // ring depth asked for at creation (used when jb_ctx_reserve builds the ring later)
  Slot slots[64];  // n_slots of them are in use
  Slot huff_aux;   // blob + status of jb_entropy_decode_device (the only fields of it in use)
  int next_slot = 0;
  int next_ticket = 1;
  int n_cus = 256;                 // compute units of the device
  size_t blob_hint = 0;            // the largest device blob any slot has been given (huff_stage)
  long long n_device_entropy = 0;  // images whose entropy stage ran on the device (jb_huff.hip)
  jb_image_desc last_desc = {0, 0, 0, 0, {0, 0, 0}, 0};  // frame of the last jb_decode_file / jb_decode_memory
  std::string error;
  DlEngine *dl = nullptr;   // the device's download engine, once this context has handed it a copy
  int dl_outstanding = 0;   // copies handed over and not issued yet (under dl->mu)
  // Which of several contexts' ready copies the engine issues first: the smaller number.  The batch decoder gives
  // every run the next number, so that of two batches in flight the OLDER one gets the link and finishes, instead of
  // both sharing it and finishing together (two batches that share evenly fall into step, and the start-up of the
  // next pair then overlaps nothing).
  std::atomic<uint64_t> dl_age{0};
  std::string dl_error;     // (under dl->mu)
  // "Fixed output size": the tight uint8 intermediates between the pixel kernel and jb_resample_kernel, one scratch per
  // stream that has carried such a launch (the two launches and the next pair on the same stream are ordered; launches
  // on different streams of the ring run side by side and must not share one).  Each grows on demand, is reused, and
  // holds at most knobs.resize_tmp_bytes (or one image, when that is larger) plus the slack the kernel's loads want.
  struct Tmp {
    void *d = nullptr;
    size_t cap = 0;
  };
  std::mutex tmp_mu;
  std::map<hipStream_t, Tmp> tmp;
  // "Decoder arithmetic" (include/jpegblk.h): JB_ARITH_*, what every later pixel launch of this context computes in.
  // Under JB_ARITH_LIBJPEG a launch decodes into uint8 Y, Cb, Cr planes first (jb_libjpeg.hip): `planes` holds them, a
  // scratch per stream like `tmp` and apart from it -- the resized routes keep their intermediate in `tmp` while the
  // pixel launch that fills it reads the planes.
  int arithmetic = JB_ARITH_REFERENCE;
  std::map<hipStream_t, Tmp> planes;
  // "Orientation" (include/jpegblk.h): JB_ORIENT_* or 2..8, what the plans of this context's later calls are made for
  // (jb_plan.h: the plan carries the value to the launch).  Its intermediates live in `tmp`.
  int orientation = JB_ORIENT_STORED;
  // "Draft decode" (include/jpegblk.h): 1, 2, 4, 8.  Not 1: the plans of this context's later calls are made for the
  // draft frame (jb_draft_desc_) and its pixel launches (JB_ARITH_LIBJPEG's alone) decode that frame.
  int draft = 1;
  // which front end the last launch of the tile kernel took (JB_FRONT_*, jb_ctx_last_front) and whether its tiling was linear
  int last_front = JB_FRONT_NONE, last_linear = 0;
};

// the error text of a failed call, formatted: into the context (ctx may be null) and the calling thread (jb_fail_)
__attribute__((format(printf, 3, 4))) static inline int fail(jb_ctx *ctx, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return jb_fail_(ctx, code, buf);
}

#define JB_HIP(ctx, call)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) return fail(ctx, JB_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Makes the context's device current for the duration of a call and restores the caller's
// (a jb_ctx may live on any GPU of the node; the calling thread may be using another one).
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

static inline int check_desc(jb_ctx *ctx, const jb_image_desc *d, jb_geometry *g) {
  int rc = jb_geometry_of(d, g);
  if (rc == JB_ERR_NULL) return fail(ctx, rc, "null descriptor");
  if (rc == JB_ERR_GEOMETRY) return fail(ctx, rc, "image size %dx%d outside 1..65535", d->width, d->height);
  if (rc == JB_ERR_SAMPLING) return fail(ctx, rc, "luma sampling factors %dx%d not in {1,2}x{1,2}", d->hs, d->vs);
  if (rc == JB_ERR_QTAB) return fail(ctx, rc, "quantisation table id outside 0..3");
  return rc;
}

// (jb_seam.cpp) the pixel launch of a batch on `stream` or (null) the context's primary stream; plan: what the pixels
// look like (jb_plan.h); fn: the entry point's name, for the error text
__attribute__((visibility("hidden"))) int seam_launch(jb_ctx *ctx, const jb_device_batch *b, void *stream, const JbOutPlan &plan,
                                                     const char *fn);
