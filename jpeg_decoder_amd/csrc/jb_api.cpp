// jb_api.cpp -- the C ABI of include/jpegblk.h over the HIP kernels of jb_kernels.hip.
//
// Host side of the seam dequantize(); inverseDCT(); YCbCrToRGB(); (reference
// jpeg.cpp:786-788).  A jb_ctx owns two HIP streams and a ring of staging slots (device
// coefficient / pixel buffers + a pinned quant-table block each) so that the copies and the
// kernel of image i overlap the host Huffman stage of image i+1.  One stream uploads and
// computes (H2D + kernel), the other downloads (D2H, ordered after the kernel by an event), so
// the pixels of image i travel device->host while the coefficients of image i+1 travel
// host->device (the link is full duplex: 57 GB/s one way, 97 GB/s both ways, tools/probe_pcie.hip).  There is deliberately NO CPU
// fallback here: without a usable HIP device every compute entry point fails with JB_ERR_HIP.
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <new>
#include <thread>

#include "jb_ctx.h"
#include "jb_kernels.h"

namespace {

// The staging ring drives up to 8 stream pairs and 16 pool streams per context; the HIP runtime
// maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue
// run their kernels one after the other.  Measured with 16 submitting threads: 1,024 1080p files
// 2,838 -> 3,211 images/s (host entropy), 4,807 -> 5,428 (device entropy), 128 files 2,398 -> 3,344,
// with 16 queues instead of 4.  So the library asks for 16 when it is loaded -- only if the variable
// is not set already, and only effective if the process has not initialised HIP yet: an application
// that initialises HIP first (torch, say) sets GPU_MAX_HW_QUEUES=16 itself, or loads this library
// first.  The setting is process-wide (every HIP user of the process gets 16 queues);
// JPEGBLK_HW_QUEUES=0 leaves the runtime's default alone, =N asks for N (include/jpegblk.h says the same).
__attribute__((constructor)) void jb_ask_for_hw_queues() {
  const char *k = getenv("JPEGBLK_HW_QUEUES");
  if (k && k[0] == '0' && k[1] == 0) return;
  if (getenv("GPU_MAX_HW_QUEUES")) return;  // the application's own choice stands
  setenv("GPU_MAX_HW_QUEUES", (k && k[0]) ? k : "16", 0);
}

thread_local std::string g_tls_error = "";

}  // namespace

// one download handed to the device's download thread
struct DlItem {
  jb_ctx *ctx;
  uint64_t age;  // the context's dl_age when the copy was handed over: the engine serves the smallest first
  Slot *slot;
  void *dst;
  const void *src;
  size_t bytes;                                    // 1-D copy ...
  size_t dst_pitch, src_pitch, row_bytes, rows;    // ... or, rows > 0, a 2-D one
  void *status_dst;
  const void *status_src;
  size_t status_bytes;
};

// Downloads of the submissions whose entropy stage runs on the device, in the order their KERNELS FINISH, back to
// back on one stream -- one engine per DEVICE, shared by every context on it (two batch decoders on one GPU, the
// two sides of jb_batch_decoder_submit): the link has one direction to give, and copies of several contexts issued
// side by side share it at 45 GB/s where one stream gets 57.  Issued by the submitting threads on their own
// streams, several copies shared the link the same way; on one dedicated stream in SUBMISSION order a copy whose
// kernels were still queued held up every copy behind it.  So the submitter records `computed` behind its kernels
// and hands the copy to this thread, which issues whichever is ready, two deep.
struct DlEngine {
  int device = 0;
  int refs = 0;  // contexts holding it (under g_dl_mu)
  std::thread thread;
  std::mutex mu;
  std::condition_variable cv, issued_cv;
  std::deque<DlItem> queue;
  bool stop = false;
  hipStream_t stream = nullptr;
};

namespace {

// The staging ring of a context (device coefficient / pixel buffers, a pinned table block and two
// events per slot, plus the download stream), sized from ctx->max_coef / ctx->rgb_alloc.  The
// caller holds a DeviceGuard on ctx->device, so the pinned table blocks are pinned against THAT
// device (and land on its NUMA node), not against whatever device the calling thread had current.
hipError_t build_ring(jb_ctx *ctx) {
  hipError_t e = hipSuccess;
  if (!ctx->stream2) e = hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking);
  for (int i = 0; e == hipSuccess && i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    e = hipMalloc(&s.d_coef, round_up((int64_t)ctx->max_coef, 256));
    if (e == hipSuccess) e = hipMalloc(&s.d_rgb, ctx->rgb_alloc);
    if (e == hipSuccess && !s.d_q) e = hipMalloc((void **)&s.d_q, 768 * 256);  // tables of up to 256 images
    if (e == hipSuccess && !s.h_q) e = hipHostMalloc((void **)&s.h_q, 768 * 256, hipHostMallocDefault);
    // (hipEventBlockingSync -- waiting threads sleep instead of spinning -- was measured with 16 waiting
    // threads on a 16-CPU share: no difference, 6,003 vs 5,671 and 216 vs 217 images/s)
    if (e == hipSuccess && !s.done) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    if (e == hipSuccess && !s.computed) e = hipEventCreateWithFlags(&s.computed, hipEventDisableTiming);
    // what a submission decoded on the device needs beside the coefficients: status words, and a blob for the scan
    // bytes and the decoder's per-chunk state -- about a seventh of the coefficient bytes for quality-75 files --
    // made here, with the ring, rather than by the first submission that lands on the slot
    if (e == hipSuccess && !s.h_status && ctx->knobs.gpu_huffman != 0) {
      e = hipHostMalloc((void **)&s.h_status, 4 * 256, hipHostMallocDefault);
      if (e == hipSuccess) e = hipMalloc((void **)&s.d_status, 4 * 256);
    }
    if (e == hipSuccess && !s.d_blob && ctx->knobs.gpu_huffman != 0 && ctx->n_slots > 1) {
      const size_t cap = ctx->max_coef / 6 + ((size_t)256 << 10);
      e = hipMalloc(&s.d_blob, cap);
      if (e == hipSuccess) s.blob_cap = cap;
    }
  }
  return e;
}

// The ring slot of the next submission: strict round robin; a full ring blocks the submitter on the
// oldest submission (back-pressure).  (Taking the first slot whose submission has completed instead
// -- submissions on different streams complete out of order -- was measured with 16 submitting
// threads: no gain on 1,024 1080p or 64 8192x8192 files, 2-4 % slower on 8,192 small images and on
// the host-entropy path, where the queries under the shared lock cost more than the rare wait:
// profiles/r02b/ab_ring_order.txt.)
// the submission in slot `s` has completed: its download has been issued (by the download thread, if it went
// that way) and has finished
int slot_finish(jb_ctx *ctx, Slot &s) {
  if (s.dl_pending.load(std::memory_order_acquire)) {
    std::unique_lock<std::mutex> lk(ctx->dl->mu);
    ctx->dl->issued_cv.wait(lk, [&] { return s.dl_pending.load(std::memory_order_acquire) == 0; });
    if (!ctx->dl_error.empty()) return fail(ctx, JB_ERR_HIP, "%s", ctx->dl_error.c_str());
  }
  JB_HIP(ctx, hipEventSynchronize(s.done));
  return JB_OK;
}

int take_slot(jb_ctx *ctx, Slot **out) {
  Slot &s = ctx->slots[ctx->next_slot];
  if (s.busy) {
    const int rc = slot_finish(ctx, s);
    if (rc) return rc;
    s.busy = false;
  }
  *out = &s;
  return JB_OK;
}

std::mutex g_dl_mu;
std::map<int, DlEngine *> g_dl;  // device -> its download engine, while any context holds it

void dl_thread_main(DlEngine *eng) {
  (void)hipSetDevice(eng->device);
  // two copies deep, by the engine's OWN events (a context -- and its slots' events -- may be destroyed as soon as
  // its copies have finished, while this thread still remembers them)
  hipEvent_t mark[2] = {nullptr, nullptr};
  bool marked[2] = {false, false};
  for (hipEvent_t &m : mark) (void)hipEventCreateWithFlags(&m, hipEventDisableTiming);
  unsigned n_issued = 0;
  for (;;) {
    DlItem it;
    bool have = false;
    {
      std::unique_lock<std::mutex> lk(eng->mu);
      eng->cv.wait(lk, [&] { return eng->stop || !eng->queue.empty(); });
      if (eng->stop && eng->queue.empty()) break;
      // the oldest batch's ready copy; within a batch, the one handed over first
      auto best = eng->queue.end();
      for (auto q = eng->queue.begin(); q != eng->queue.end(); ++q) {
        if (best != eng->queue.end() && q->age >= best->age) continue;
        const hipError_t e = hipEventQuery(q->slot->computed);
        if (e != hipErrorNotReady) best = q;  // finished (or failed: the copy below will say so)
      }
      if (best != eng->queue.end()) {
        it = *best;
        eng->queue.erase(best);
        have = true;
      }
      (void)hipGetLastError();  // (hipErrorNotReady is not an error of this thread's next call)
    }
    if (!have) {
      std::this_thread::sleep_for(std::chrono::microseconds(20));
      continue;
    }
    // two copies deep: the engine always has the next one, and nothing queues up behind a slow host
    const unsigned m = n_issued++ & 1;
    if (marked[m]) (void)hipEventSynchronize(mark[m]);  // the copy before the last has finished
    hipError_t e;
    if (it.rows) e = hipMemcpy2DAsync(it.dst, it.dst_pitch, it.src, it.src_pitch, it.row_bytes, it.rows, hipMemcpyDeviceToHost, eng->stream);
    else e = hipMemcpyAsync(it.dst, it.src, it.bytes, hipMemcpyDeviceToHost, eng->stream);
    if (e == hipSuccess && it.status_bytes) e = hipMemcpyAsync(it.status_dst, it.status_src, it.status_bytes, hipMemcpyDeviceToHost, eng->stream);
    if (e == hipSuccess) e = hipEventRecord(it.slot->done, eng->stream);
    marked[m] = mark[m] && hipEventRecord(mark[m], eng->stream) == hipSuccess;
    {
      std::lock_guard<std::mutex> lk(eng->mu);
      if (e != hipSuccess && it.ctx->dl_error.empty()) it.ctx->dl_error = std::string("download thread: ") + hipGetErrorString(e);
      it.slot->dl_pending.store(0, std::memory_order_release);
      it.ctx->dl_outstanding--;
    }
    eng->issued_cv.notify_all();
  }
  for (hipEvent_t m : mark)
    if (m) (void)hipEventDestroy(m);
}

// hand a download to the device's download thread (engine and thread are made on first use); the caller has
// recorded item.slot->computed and holds a DeviceGuard on ctx->device
int dl_enqueue(jb_ctx *ctx, const DlItem &item) {
  if (!ctx->dl) {
    std::lock_guard<std::mutex> g(g_dl_mu);
    DlEngine *&eng = g_dl[ctx->device];
    if (!eng) {
      std::unique_ptr<DlEngine> fresh(new DlEngine());
      fresh->device = ctx->device;
      JB_HIP(ctx, hipStreamCreateWithFlags(&fresh->stream, hipStreamNonBlocking));
      fresh->thread = std::thread(dl_thread_main, fresh.get());
      eng = fresh.release();
    }
    eng->refs++;
    ctx->dl = eng;
  }
  item.slot->dl_pending.store(1, std::memory_order_release);
  {
    std::lock_guard<std::mutex> lk(ctx->dl->mu);
    ctx->dl_outstanding++;
    ctx->dl->queue.push_back(item);
  }
  ctx->dl->cv.notify_one();
  return JB_OK;
}

// every download this context handed over has been issued
void dl_drain(jb_ctx *ctx) {
  if (!ctx->dl) return;
  std::unique_lock<std::mutex> lk(ctx->dl->mu);
  ctx->dl->issued_cv.wait(lk, [&] { return ctx->dl_outstanding == 0; });
}

// ... and has finished: the slots' `done` events (the engine's stream also carries other contexts' copies)
hipError_t dl_wait_copies(jb_ctx *ctx) {
  dl_drain(ctx);
  for (int i = 0; i < ctx->n_slots; i++)
    if (ctx->slots[i].done) {
      const hipError_t e = hipEventSynchronize(ctx->slots[i].done);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

// the context lets go of the device's engine; the last one out stops the thread
void dl_release(jb_ctx *ctx) {
  if (!ctx->dl) return;
  (void)dl_wait_copies(ctx);
  DlEngine *eng = ctx->dl;
  ctx->dl = nullptr;
  std::lock_guard<std::mutex> g(g_dl_mu);
  if (--eng->refs > 0) return;
  g_dl.erase(eng->device);
  {
    std::lock_guard<std::mutex> lk(eng->mu);
    eng->stop = true;
  }
  eng->cv.notify_all();
  eng->thread.join();
  (void)hipStreamSynchronize(eng->stream);
  (void)hipStreamDestroy(eng->stream);
  delete eng;
}

// nothing of this context is in flight any more: the downloads handed to the engine, and every stream it has made
hipError_t sync_all_streams(jb_ctx *ctx) {
  hipError_t e = dl_wait_copies(ctx);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && ctx->stream2) e = hipStreamSynchronize(ctx->stream2);
  for (hipStream_t ps : ctx->pool)
    if (e == hipSuccess && ps) e = hipStreamSynchronize(ps);
  for (int k = 1; k < jb_ctx::kMaxPairs; k++) {
    if (e == hipSuccess && ctx->pair_up[k]) e = hipStreamSynchronize(ctx->pair_up[k]);
    if (e == hipSuccess && ctx->pair_down[k]) e = hipStreamSynchronize(ctx->pair_down[k]);
  }
  return e;
}

}  // namespace

extern "C" {

int jb_abi_version(void) { return JB_ABI_VERSION; }

int jb_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(nullptr, JB_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int jb_ctx_create(int device_id, size_t max_coef_bytes, size_t max_rgb_bytes, int n_slots, jb_ctx **out) {
  if (!out) return fail(nullptr, JB_ERR_NULL, "jb_ctx_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  JB_HIP(nullptr, hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev)
    return fail(nullptr, JB_ERR_HIP, "device %d not available (%d HIP devices visible)", device_id, ndev);
  if ((max_coef_bytes == 0) != (max_rgb_bytes == 0))
    return fail(nullptr, JB_ERR_CAPACITY, "max_coef_bytes and max_rgb_bytes must both be zero or both non-zero");
  if (n_slots < 1) n_slots = 1;
  if (n_slots > 64) n_slots = 64;
  jb_ctx *ctx = new (std::nothrow) jb_ctx();
  if (!ctx) return fail(nullptr, JB_ERR_CAPACITY, "out of host memory");
  ctx->device = device_id;
  ctx->max_coef = max_coef_bytes;
  ctx->max_rgb = max_rgb_bytes;
  ctx->rgb_alloc = max_rgb_bytes ? (size_t)round_up((int64_t)max_rgb_bytes, 256) : 0;  // device rows are tightly packed
  ctx->n_slots = max_coef_bytes ? n_slots : 0;
  ctx->n_slots_req = n_slots;
  ctx->knobs = jb_knobs_read();
  DeviceGuard guard(device_id);
  hipError_t e = hipSuccess;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) ctx->n_cus = cus;
    (void)hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e == hipSuccess && ctx->n_slots > 0) e = build_ring(ctx);
  if (e != hipSuccess) {
    int rc = fail(nullptr, JB_ERR_HIP, "jb_ctx_create: %s", hipGetErrorString(e));
    jb_ctx_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return JB_OK;
}

void jb_ctx_destroy(jb_ctx *ctx) {
  if (!ctx) return;
  DeviceGuard guard(ctx->device);
  dl_release(ctx);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  for (hipStream_t &ps : ctx->pool)
    if (ps) {
      (void)hipStreamSynchronize(ps);
      (void)hipStreamDestroy(ps);
      ps = nullptr;
    }
  for (int k = 1; k < jb_ctx::kMaxPairs; k++)
    for (hipStream_t *ps : {&ctx->pair_up[k], &ctx->pair_down[k]})
      if (*ps) {
        (void)hipStreamSynchronize(*ps);
        (void)hipStreamDestroy(*ps);
        *ps = nullptr;
      }
  for (int i = 0; i < 64; i++) {
    Slot &s = ctx->slots[i];
    if (s.d_coef) (void)hipFree(s.d_coef);
    if (s.d_rgb) (void)hipFree(s.d_rgb);
    if (s.d_q) (void)hipFree(s.d_q);
    if (s.h_q) (void)hipHostFree(s.h_q);
    if (s.h_blob) (void)hipHostFree(s.h_blob);
    if (s.d_blob) (void)hipFree(s.d_blob);
    if (s.h_status) (void)hipHostFree(s.h_status);
    if (s.d_status) (void)hipFree(s.d_status);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.computed) (void)hipEventDestroy(s.computed);
  }
  {
    Slot &s = ctx->huff_aux;
    if (s.h_blob) (void)hipHostFree(s.h_blob);
    if (s.d_blob) (void)hipFree(s.d_blob);
    if (s.h_status) (void)hipHostFree(s.h_status);
    if (s.d_status) (void)hipFree(s.d_status);
  }
  for (auto &kv : ctx->tmp)
    if (kv.second.d) (void)hipFree(kv.second.d);  // (hipFree waits for the device: launches on a caller's stream included)
  for (auto &kv : ctx->planes)
    if (kv.second.d) (void)hipFree(kv.second.d);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  delete ctx;
}

const char *jb_last_error(const jb_ctx *ctx) { return ctx ? ctx->error.c_str() : g_tls_error.c_str(); }

void *jb_ctx_stream(jb_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int jb_ctx_synchronize(jb_ctx *ctx) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_ctx_synchronize: ctx is NULL");
  DeviceGuard guard(ctx->device);
  JB_HIP(ctx, sync_all_streams(ctx));
  return JB_OK;
}

int jb_ctx_device(const jb_ctx *ctx) { return ctx ? ctx->device : -1; }

int jb_ctx_set_arithmetic(jb_ctx *ctx, int arith) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_ctx_set_arithmetic: ctx is NULL");
  if (arith != JB_ARITH_REFERENCE && arith != JB_ARITH_LIBJPEG) return fail(ctx, JB_ERR_GEOMETRY, "jb_ctx_set_arithmetic: unknown arithmetic %d", arith);
  // a submission of the ring that has not completed would change its arithmetic between its launches
  DeviceGuard guard(ctx->device);
  for (int i = 0; i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    if (!s.busy) continue;
    if (s.dl_pending.load(std::memory_order_acquire) || hipEventQuery(s.done) == hipErrorNotReady)
      return fail(ctx, JB_ERR_STATE, "jb_ctx_set_arithmetic: a submission is in flight (wait for it first)");
  }
  ctx->arithmetic = arith;
  return JB_OK;
}

int jb_ctx_arithmetic(const jb_ctx *ctx) { return ctx ? ctx->arithmetic : JB_ARITH_REFERENCE; }

int jb_ctx_set_orientation(jb_ctx *ctx, int orientation) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_ctx_set_orientation: ctx is NULL");
  if (orientation < 0 || orientation > 8) return fail(ctx, JB_ERR_GEOMETRY, "jb_ctx_set_orientation: %d is outside 0..8", orientation);
  // (as jb_ctx_set_arithmetic: not while a submission of the ring is in flight)
  DeviceGuard guard(ctx->device);
  for (int i = 0; i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    if (!s.busy) continue;
    if (s.dl_pending.load(std::memory_order_acquire) || hipEventQuery(s.done) == hipErrorNotReady)
      return fail(ctx, JB_ERR_STATE, "jb_ctx_set_orientation: a submission is in flight (wait for it first)");
  }
  ctx->orientation = orientation;
  return JB_OK;
}

int jb_ctx_orientation(const jb_ctx *ctx) { return ctx ? ctx->orientation : JB_ORIENT_STORED; }

int jb_ctx_set_draft(jb_ctx *ctx, int denom) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_ctx_set_draft: ctx is NULL");
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return fail(ctx, JB_ERR_GEOMETRY, "jb_ctx_set_draft: %d is not 1, 2, 4 or 8", denom);
  // (as jb_ctx_set_arithmetic: not while a submission of the ring is in flight)
  DeviceGuard guard(ctx->device);
  for (int i = 0; i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    if (!s.busy) continue;
    if (s.dl_pending.load(std::memory_order_acquire) || hipEventQuery(s.done) == hipErrorNotReady)
      return fail(ctx, JB_ERR_STATE, "jb_ctx_set_draft: a submission is in flight (wait for it first)");
  }
  ctx->draft = denom;
  return JB_OK;
}

int jb_ctx_draft(const jb_ctx *ctx) { return ctx ? ctx->draft : 1; }

long long jb_ctx_device_entropy_images(const jb_ctx *ctx) { return ctx ? ctx->n_device_entropy : 0; }

int jb_ctx_last_desc(const jb_ctx *ctx, jb_image_desc *out) {
  if (!ctx || !out) return fail(nullptr, JB_ERR_NULL, "jb_ctx_last_desc: NULL pointer");
  if (ctx->last_desc.width == 0) return fail(nullptr, JB_ERR_STATE, "jb_ctx_last_desc: nothing decoded on this context yet");
  *out = ctx->last_desc;
  return JB_OK;
}

int jb_ctx_reserve(jb_ctx *ctx, size_t max_coef_bytes, size_t max_rgb_bytes) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_ctx_reserve: ctx is NULL");
  if (max_coef_bytes == 0 || max_rgb_bytes == 0) return fail(ctx, JB_ERR_CAPACITY, "jb_ctx_reserve: sizes must be non-zero");
  if (ctx->n_slots > 0 && max_coef_bytes <= ctx->max_coef && max_rgb_bytes <= ctx->max_rgb) return JB_OK;
  DeviceGuard guard(ctx->device);
  // nothing may be in flight while the slots' buffers are replaced
  JB_HIP(ctx, sync_all_streams(ctx));
  if (max_coef_bytes < ctx->max_coef) max_coef_bytes = ctx->max_coef;
  if (max_rgb_bytes < ctx->max_rgb) max_rgb_bytes = ctx->max_rgb;
  const int n = ctx->n_slots > 0 ? ctx->n_slots : ctx->n_slots_req;
  for (int i = 0; i < n; i++) {
    Slot &s = ctx->slots[i];
    s.busy = false;
    if (s.d_coef) (void)hipFree(s.d_coef);
    if (s.d_rgb) (void)hipFree(s.d_rgb);
    s.d_coef = s.d_rgb = nullptr;
  }
  ctx->max_coef = max_coef_bytes;
  ctx->max_rgb = max_rgb_bytes;
  ctx->rgb_alloc = (size_t)round_up((int64_t)max_rgb_bytes, 256);
  ctx->n_slots = n;
  hipError_t e = build_ring(ctx);
  if (e != hipSuccess) {
    ctx->n_slots = 0;  // a half-built ring is not used; jb_ctx_destroy releases what exists
    ctx->max_coef = ctx->max_rgb = ctx->rgb_alloc = 0;
    return fail(ctx, JB_ERR_HIP, "jb_ctx_reserve(%zu, %zu): %s", max_coef_bytes, max_rgb_bytes, hipGetErrorString(e));
  }
  return JB_OK;
}

// Pinned host memory is pinned AGAINST a device: hipHostMalloc registers the pages with the
// calling thread's current device and (ROCm's default policy) takes them from the host NUMA node
// closest to that device.  Under one rank per GPU with every GPU visible, a fresh std::thread's
// current device is 0 -- so the device is always named explicitly here.
void *jb_pinned_alloc_on(int device_id, size_t bytes) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
    fail(nullptr, JB_ERR_HIP, "jb_pinned_alloc_on: device %d not available (%d HIP devices visible)", device_id, ndev);
    return nullptr;
  }
  DeviceGuard guard(device_id);
  void *p = nullptr;
  // portable: every device of the process may copy to / from it (a multi-device decoder's shared arena)
  hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
  if (e != hipSuccess) {
    fail(nullptr, JB_ERR_HIP, "hipHostMalloc(%zu) on device %d: %s", bytes, device_id, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

void *jb_pinned_alloc(size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    fail(nullptr, JB_ERR_HIP, "jb_pinned_alloc: no usable HIP device");
    return nullptr;
  }
  return jb_pinned_alloc_on(dev, bytes);
}

int jb_device_numa_node(int device_id) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return fail(nullptr, JB_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, JB_ERR_HIP, "device %d not available (%d HIP devices visible)", device_id, ndev);
  int node = -1;
  if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, device_id) == hipSuccess && node >= 0) return node;
  (void)hipGetLastError();  // a runtime without that attribute: not an error of the caller's next HIP call
  // fallback: the PCI function's numa_node in sysfs
  char bdf[32] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device_id) == hipSuccess) {
    for (char *c = bdf; *c; c++)
      if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    char path[96];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    if (FILE *f = fopen(path, "r")) {
      int v = -1;
      if (fscanf(f, "%d", &v) != 1) v = -1;
      fclose(f);
      if (v >= 0) return v;
    }
  }
  return fail(nullptr, JB_ERR_STATE, "NUMA node of device %d unknown", device_id);
}

void jb_pinned_free(void *p) {
  if (p) (void)hipHostFree(p);
}

}  // extern "C"

namespace {

constexpr int kMaxBatch = 256;  // images per submission (the slot's table block holds that many)

// What submit_impl and submit_jobs_impl have in common.  They differ on purpose in their streams, in how the download
// is issued and in the status words (see each); everything around that is here.
struct Submission {
  DeviceGuard guard;
  jb_geometry g;
  size_t coef_total = 0, rgb_total = 0;
  Slot *slot = nullptr;
  explicit Submission(jb_ctx *ctx) : guard(ctx->device) {}
};

// Prologue, first half: validation, capacity, and the ring slot (a full ring blocks here).  n_images images of one
// geometry; the caller's pixels have rows of rgb_stride bytes; plan: what they look like (rows on the device are tight:
// plan.row_stride).  dst_device: the pixels stay in DEVICE memory of ctx's device and nothing is downloaded.
int submit_begin(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const JbOutPlan &plan, int64_t rgb_stride, bool dst_device,
                 Submission &sub) {
  if (ctx->n_slots == 0) return fail(ctx, JB_ERR_CAPACITY, "context was created without staging buffers");
  int rc = check_desc(ctx, desc, &sub.g);
  if (rc) return rc;
  if (n_images < 1 || n_images > kMaxBatch) return fail(ctx, JB_ERR_GEOMETRY, "n_images = %d outside 1..%d", n_images, kMaxBatch);
  // "draft decode": the plan is the draft frame's, which exists only where the draft goes with everything else
  if (const char *why = jb_draft_refusal_(ctx->draft, ctx->arithmetic, plan.scale ? plan.scale : 1, plan.orient == JB_ORIENT_STORED ? ctx->orientation : plan.orient))
    return fail(ctx, JB_ERR_UNSUPPORTED, "submit: %s", why);
  if (plan.status != JB_OK) return fail(ctx, plan.status, "submit: %s", plan.why);
  if (ctx->arithmetic == JB_ARITH_LIBJPEG && plan.scale != 1) return fail(ctx, JB_ERR_UNSUPPORTED, "submit: %s", kJbArithScaleText);
  if (plan.orient == JB_ORIENT_EXIF) return fail(ctx, JB_ERR_STATE, "submit: %s", kJbOrientExifText);
  // tight rows on the device (12-byte stores need no alignment); a planar format: tight rows of a plane, tight planes
  if (plan.planar && rgb_stride != plan.row_stride) return fail(ctx, JB_ERR_GEOMETRY, "planar output has tight rows");
  if (rgb_stride < plan.row_stride) return fail(ctx, JB_ERR_GEOMETRY, "rgb_stride %lld < 3*width", (long long)rgb_stride);
  sub.coef_total = (size_t)sub.g.coef_bytes * (size_t)n_images, sub.rgb_total = (size_t)plan.image_bytes * (size_t)n_images;
  if (sub.coef_total > ctx->max_coef || (!dst_device && (sub.rgb_total > ctx->rgb_alloc || sub.rgb_total > ctx->max_rgb)))
    return fail(ctx, JB_ERR_CAPACITY, "%d image(s) of %dx%d exceed the capacity the context was created with", n_images,
                desc->width, desc->height);
  if (dst_device && rgb_stride != plan.row_stride) return fail(ctx, JB_ERR_GEOMETRY, "device output has tight rows");
  return take_slot(ctx, &sub.slot);
}

// Prologue, second half, once the caller has chosen its stream: the images' tables (jobs[i]->qtabs, or qtabs + i * 256)
// resolved into the slot's pinned block and uploaded
int submit_tables(jb_ctx *ctx, Slot &s, const jb_image_desc *desc, int n_images, const JbHuffJob *const *jobs, const uint16_t *qtabs,
                  hipStream_t up) {
  for (int i = 0; i < n_images; i++) {
    const int rc = jb_resolve_qtabs(desc, jobs ? jobs[i]->qtabs : qtabs + (size_t)i * 256, s.h_q + (size_t)i * 192);
    if (rc) return fail(ctx, rc, "bad quantisation table id");
  }
  JB_HIP(ctx, hipMemcpyAsync(s.d_q, s.h_q, 768u * (size_t)n_images, hipMemcpyHostToDevice, up));
  return JB_OK;
}

// The pixel kernel of a submission whose coefficients are (or will be, in stream order) in the slot: into the slot's
// pixel buffer, or (dst_device) straight into the caller's device memory
int submit_launch(jb_ctx *ctx, const Submission &sub, const jb_image_desc *desc, int n_images, const JbOutPlan &plan, uint8_t *rgb,
                  bool dst_device, hipStream_t up) {
  const Slot &s = *sub.slot;
  jb_device_batch b;
  memset(&b, 0, sizeof b);
  b.desc = *desc;
  b.n_images = n_images;
  b.d_coef = (const int16_t *)s.d_coef;
  b.coef_image_stride = sub.g.coef_bytes;  // a multiple of 128
  b.d_qtabs = s.d_q;
  b.qtab_image_stride = n_images > 1 ? 768 : 0;
  b.d_rgb = dst_device ? rgb : (uint8_t *)s.d_rgb;
  b.rgb_row_stride = plan.row_stride;
  // ("views": an image's outputs back to back; "view groups": the images' blocks, which the seam takes apart)
  b.rgb_image_stride = plan.views && plan.n_groups == 0 ? plan.view_bytes : plan.image_bytes;
  return seam_launch(ctx, &b, up, plan, "submit");
}

// Epilogue: the slot is in flight under the next ticket, and the ring moves on
void submit_end(jb_ctx *ctx, Slot &s, int *ticket) {
  s.busy = true;
  s.ticket = ctx->next_ticket++;
  if (ctx->next_ticket < 0) ctx->next_ticket = 1;
  *ticket = s.ticket;
  ctx->next_slot = (ctx->next_slot + 1) % ctx->n_slots;
}

// One submission of the staging ring: n_images images of one geometry, coefficients contiguous
// (image stride = coef_bytes), tables per image, pixels contiguous with tight rows -- or, for
// n_images == 1, any row stride.
// dst_device: `rgb` is DEVICE memory of ctx's device -- the kernel writes the pixels there and nothing
// is downloaded (jb_batch_decoder_set_device_output).
// plan: what the pixels look like (at scale 2, 4, 8 the area-reduced image); rgb / rgb_stride describe that output.
int submit_impl(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const int16_t *coef, const uint16_t *qtabs,
                uint8_t *rgb, int64_t rgb_stride, int *ticket, const JbOutPlan &plan, bool dst_device) {
  Submission sub(ctx);
  int rc = submit_begin(ctx, desc, n_images, plan, rgb_stride, dst_device, sub);
  if (rc) return rc;
  Slot &s = *sub.slot;
  // One image: upload + kernel on the primary stream, download on the second (ordered by an
  // event), so the link runs both ways even with a single submitter.  A group of small images
  // runs whole on one stream and consecutive groups alternate between the two streams: with many
  // submitters that overlaps uploads and downloads just as well, without a cross-stream event per
  // group (measured with 16 host threads on 679x451 images: 14,500 images/s with the event,
  // 24,700 with every group on one stream, 38,400 alternating).
  hipStream_t up = ctx->stream, down = ctx->stream2 ? ctx->stream2 : ctx->stream;
  if (n_images > 1) {
    if (ctx->stream2 && (ctx->n_group_submits++ & 1u)) up = ctx->stream2;
    down = up;
  } else if (ctx->stream2 && ctx->n_pairs > 1 && sub.coef_total + sub.rgb_total < jb_ctx::kLargeSubmission) {
    // one image: the next of the K (upload + kernel, download) stream pairs
    const int k = (int)(ctx->n_single_submits++ % (unsigned)ctx->n_pairs);
    if (k > 0) {
      if (!ctx->pair_up[k]) JB_HIP(ctx, hipStreamCreateWithFlags(&ctx->pair_up[k], hipStreamNonBlocking));
      if (!ctx->pair_down[k]) JB_HIP(ctx, hipStreamCreateWithFlags(&ctx->pair_down[k], hipStreamNonBlocking));
      up = ctx->pair_up[k];
      down = ctx->pair_down[k];
    }
  }
  rc = submit_tables(ctx, s, desc, n_images, nullptr, qtabs, up);
  if (rc) return rc;
  JB_HIP(ctx, hipMemcpyAsync(s.d_coef, coef, sub.coef_total, hipMemcpyHostToDevice, up));
  rc = submit_launch(ctx, sub, desc, n_images, plan, rgb, dst_device, up);
  if (rc) return rc;
  if (dst_device) {
    down = up;  // the pixels stay on the device: done when the kernel is
  } else {
    // the download runs on its own stream, after the kernel: it overlaps the next image's upload
    if (down != up) {
      JB_HIP(ctx, hipEventRecord(s.computed, up));
      JB_HIP(ctx, hipStreamWaitEvent(down, s.computed, 0));
    }
    if (rgb_stride == plan.row_stride)
      JB_HIP(ctx, hipMemcpyAsync(rgb, s.d_rgb, sub.rgb_total, hipMemcpyDeviceToHost, down));
    else  // (interleaved only: planar rows are tight)
      JB_HIP(ctx, hipMemcpy2DAsync(rgb, (size_t)rgb_stride, s.d_rgb, (size_t)plan.row_stride, (size_t)plan.row_stride,
                                   (size_t)plan.out_h, hipMemcpyDeviceToHost, down));
  }
  JB_HIP(ctx, hipEventRecord(s.done, down));
  submit_end(ctx, s, ticket);
  return JB_OK;
}

// ---- device-side entropy decoding (jb_huff.hip) -------------------------------------------------

// upload a packed submission (jb_huff_pack_) and launch the decoder: image i's coefficient blocks
// land at d_out + i * coef_stride bytes, its status word at s.d_status[i]
int huff_stage(jb_ctx *ctx, Slot &s, const uint8_t *h, const JbHuffLayout &lay, size_t zero_bytes, int16_t *d_out, hipStream_t up,
               int sync_launches = kJbSyncLaunches) {
  if (lay.device_total > s.blob_cap || !s.d_blob) {  // (the slot is idle: its previous submission has been waited for)
    // hipFree / hipMalloc stall the whole device: a slot that has to grow takes the largest size any slot of this
    // context has needed, so that a ring of 64 slots stops growing after the first full-size groups instead of
    // once per slot (which kept the first five or six runs of a fresh decoder slower than the rest)
    if (s.d_blob) (void)hipFree(s.d_blob);
    s.d_blob = nullptr, s.blob_cap = 0;
    size_t cap = lay.device_total + lay.device_total / 4 + 65536;
    if (cap < ctx->blob_hint) cap = ctx->blob_hint;
    JB_HIP(ctx, hipMalloc(&s.d_blob, cap));
    s.blob_cap = cap;
    ctx->blob_hint = cap;
  }
  if (!s.h_status) {
    JB_HIP(ctx, hipHostMalloc((void **)&s.h_status, 4 * 256, hipHostMallocDefault));
    JB_HIP(ctx, hipMalloc((void **)&s.d_status, 4 * 256));
  }
  // a small submission is fetched from the pinned blob by a kernel: nothing in front of the decoding kernels waits
  // for a copy engine
  if (lay.total <= ((size_t)4 << 20)) JB_HIP(ctx, jbk_huff_fetch(s.d_blob, h, lay.total, up));
  else JB_HIP(ctx, hipMemcpyAsync(s.d_blob, h, lay.total, hipMemcpyHostToDevice, up));
  // the decoder stores non-zero coefficients only
  JB_HIP(ctx, jbk_huff_zero(d_out, zero_bytes, up, s.d_status, 4 * (size_t)lay.n));  // (status words: 4 * 256 bytes are allocated)
  JbHuffLaunch p;
  memset(&p, 0, sizeof p);
  const uint8_t *d = (const uint8_t *)s.d_blob;
  uint8_t *dw = (uint8_t *)s.d_blob;
  p.scan = d + lay.off_scan;
  p.starts = (const uint32_t *)(d + lay.off_starts);
  p.tables = (const JbHuffTables *)(d + lay.off_tab);
  p.images = (const JbHuffImage *)(d + lay.off_img);
  p.wgs = (const JbHuffWg *)(d + lay.off_wg);
  p.sync_wgs = (const JbHuffWg *)(d + lay.off_sync_wg);
  p.coef = d_out;
  p.status = s.d_status;
  p.n_wgs = (int32_t)lay.n_wg;
  p.n_sync_wgs = (int32_t)lay.n_sync_wg;
  p.chunks = (const JbChunkDesc *)(d + lay.off_chunks);
  p.entry = (JbChunkState *)(dw + lay.off_entry);
  p.exit = (JbChunkState *)(dw + lay.off_exit);
  p.cps = (uint32_t *)(dw + lay.off_cps);
  p.chunk_dc = (JbChunkDc *)(dw + lay.off_chunk_dc);
  p.wgsum = (JbWgSum *)(dw + lay.off_wgsum);
  p.n_chunks_total = lay.n_chunks;
  // (one workgroup per image: its first chunk starts an interval, nothing to hand over between launches)
  p.sync_launches = lay.n_sync_wg > 0 && lay.n_wg == lay.n ? 1 : sync_launches;
  p.max_chunk_bytes = lay.max_chunk_bytes;
  p.max_tabs = lay.max_tabs;
  JB_HIP(ctx, jbk_huff_launch(p, up));
  return JB_OK;
}

// the slot's own pinned staging for callers that did not pack themselves (single images)
int pack_into_slot(jb_ctx *ctx, Slot &s, const JbHuffJob *const *jobs, int n, int64_t coef_stride, JbHuffLayout *lay) {
  const size_t need = jb_huff_pack_size_(jobs, n);
  if (need > s.h_blob_cap) {
    if (s.h_blob) (void)hipHostFree(s.h_blob);
    s.h_blob = nullptr, s.h_blob_cap = 0;
    const size_t cap = need + need / 4 + 65536;
    JB_HIP(ctx, hipHostMalloc((void **)&s.h_blob, cap, hipHostMallocDefault));
    s.h_blob_cap = cap;
  }
  const int rc = jb_huff_pack_(jobs, n, coef_stride, s.h_blob, lay);
  return rc ? fail(ctx, rc, "submission too large for the device entropy decoder") : JB_OK;
}

// One submission whose coefficients are produced ON the device: n images of one geometry, each a
// prepared JbHuffJob.  Same ring, same ordering and same download as submit_impl; what is uploaded
// is the compressed scan (a tenth of the coefficients), and the status words come back with the
// pixels.  jb_wait / jb_poll report JB_ERR_FORMAT when the decoder met corrupt data.
// Either `jobs` (packed here, into the slot's pinned staging) or a blob the caller packed itself
// (`packed` + `lay`, pinned, valid until the submission has completed) with the images' descriptor
// and tables (`desc`, `qtabs` = n x 4*64).
int submit_jobs_impl(jb_ctx *ctx, const JbHuffJob *const *jobs, const uint8_t *packed, const JbHuffLayout *lay_in,
                     const jb_image_desc *desc_in, const uint16_t *qtabs_in, int n_images, uint8_t *rgb, int64_t rgb_stride,
                     uint32_t *status_out, int *ticket, const JbOutPlan &plan, bool dst_device) {
  const jb_image_desc *desc = jobs ? &jobs[0]->desc : desc_in;
  Submission sub(ctx);
  int rc = submit_begin(ctx, desc, n_images, plan, rgb_stride, dst_device, sub);
  if (rc) return rc;
  Slot &s = *sub.slot;
  // the whole submission on one stream of the pool, consecutive submissions on different ones
  hipStream_t &ps = ctx->pool[ctx->n_group_submits++ % jb_ctx::kPool];
  if (!ps) JB_HIP(ctx, hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
  hipStream_t up = ps;
  rc = submit_tables(ctx, s, desc, n_images, jobs, qtabs_in, up);
  if (rc) return rc;
  const bool timing = ctx->knobs.timing == 2;
  const double tt0 = timing ? jb_now_s_() : 0;
  JbHuffLayout lay_own;
  if (jobs) {
    rc = pack_into_slot(ctx, s, jobs, n_images, sub.g.coef_bytes, &lay_own);
    if (rc) return rc;
    packed = s.h_blob;
    lay_in = &lay_own;
  }
  if (lay_in->n != n_images || lay_in->coef_stride != sub.g.coef_bytes) return fail(ctx, JB_ERR_STATE, "packed submission does not match its descriptor");
  const double tt1 = timing ? jb_now_s_() : 0;
  rc = huff_stage(ctx, s, packed, *lay_in, sub.coef_total, (int16_t *)s.d_coef, up);
  if (rc) return rc;
  const double tt2 = timing ? jb_now_s_() : 0;
  if (timing) (void)hipStreamSynchronize(up);
  const double tt3 = timing ? jb_now_s_() : 0;
  rc = submit_launch(ctx, sub, desc, n_images, plan, rgb, dst_device, up);
  if (rc) return rc;
  // the status words travel with the pixels: into the caller's (pinned) words when it keeps its own
  // -- many threads share this ring, a slot's words may be recycled before their owner looks -- else
  // into the slot's, which jb_wait / jb_poll check
  const double tt4 = timing ? jb_now_s_() : 0;
  if (dst_device) {
    // the pixels stay on the device; only the status words come back
    JB_HIP(ctx, hipMemcpyAsync(status_out ? status_out : s.h_status, s.d_status, 4 * (size_t)n_images, hipMemcpyDeviceToHost, up));
    JB_HIP(ctx, hipEventRecord(s.done, up));
  } else {
    // the download thread issues the copies once the kernels have finished (jb_ctx::dl_*; against the copies on the
    // submission's own stream: 1,024 1080p files 6,467-7,008 -> 7,742-7,815 images/s, 128 files 4,257-4,318 ->
    // 5,767-6,567, 64 8192x8192 files 227-238 -> 262: profiles/r03/ab_download_thread.txt)
    // (the status words travel on the submission's own stream, in front of `computed`: on the engine's stream the
    // small copy and its latency would sit between every two pixel copies of the device)
    JB_HIP(ctx, hipMemcpyAsync(status_out ? status_out : s.h_status, s.d_status, 4 * (size_t)n_images, hipMemcpyDeviceToHost, up));
    JB_HIP(ctx, hipEventRecord(s.computed, up));
    DlItem it;
    it.ctx = ctx;
    it.age = ctx->dl_age.load(std::memory_order_relaxed);
    it.slot = &s;
    it.dst = rgb, it.src = s.d_rgb, it.bytes = sub.rgb_total;
    it.rows = 0, it.dst_pitch = it.src_pitch = it.row_bytes = 0;
    if (rgb_stride != plan.row_stride)  // (interleaved only: planar rows are tight)
      it.rows = (size_t)plan.out_h, it.dst_pitch = (size_t)rgb_stride, it.src_pitch = it.row_bytes = (size_t)plan.row_stride;
    it.status_dst = nullptr;
    it.status_src = nullptr;
    it.status_bytes = 0;
    rc = dl_enqueue(ctx, it);
    if (rc) return rc;
  }
  if (timing)
    fprintf(stderr, "submit (device entropy): pack %.3f ms, upload + launches issued %.3f ms, entropy kernels done after %.3f ms more, pixel kernel + download call %.3f ms\n",
            (tt1 - tt0) * 1e3, (tt2 - tt1) * 1e3, (tt3 - tt2) * 1e3, (tt4 - tt3) * 1e3);
  ctx->n_device_entropy += n_images;
  s.n_status = status_out ? 0 : n_images;
  submit_end(ctx, s, ticket);
  return JB_OK;
}

// after a submission has completed: did the device entropy decoder flag any of its images?
int check_status(jb_ctx *ctx, Slot &s) {
  const int n = s.n_status;
  s.n_status = 0;
  for (int i = 0; i < n; i++)
    if (s.h_status[i])
      return fail(ctx, JB_ERR_FORMAT, "device entropy decoder: corrupt entropy-coded data in image %d of the submission (status %u)", i, s.h_status[i]);
  return JB_OK;
}

}  // namespace

extern "C" {

int jb_entropy_decode_device(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc, uint16_t *qtabs,
                             int16_t *d_coef, size_t coef_cap_bytes) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_entropy_decode_device: ctx is NULL");
  if (!jpeg || !desc || !d_coef) return fail(ctx, JB_ERR_NULL, "jb_entropy_decode_device: NULL pointer");
  JbHuffJob *job = new (std::nothrow) JbHuffJob();
  if (!job) return fail(ctx, JB_ERR_CAPACITY, "out of host memory");
  std::string err;
  int rc = jb_huff_prepare_(jpeg, jpeg_bytes, job, &err, ctx->knobs.chunk_bytes);
  if (rc == JB_OK && (size_t)job->geo.coef_bytes > coef_cap_bytes) rc = JB_ERR_CAPACITY, err = "coefficient buffer too small";
  if (rc == JB_OK && ((uintptr_t)d_coef & 15)) rc = JB_ERR_GEOMETRY, err = "coefficient pointer must be a multiple of 16 bytes";
  if (rc != JB_OK) {
    delete job;
    return fail(ctx, rc, "%s", err.c_str());
  }
  *desc = job->desc;
  if (qtabs) memcpy(qtabs, job->qtabs, sizeof job->qtabs);
  DeviceGuard guard(ctx->device);
  Slot &s = ctx->huff_aux;
  const JbHuffJob *jobs[1] = {job};
  JbHuffLayout lay;
  rc = pack_into_slot(ctx, s, jobs, 1, job->geo.coef_bytes, &lay);
  const size_t coef_bytes = (size_t)job->geo.coef_bytes;
  delete job;  // (everything it held is in the pinned blob now)
  if (rc) return rc;
  // The chunks fall into step within the launches of the first attempt on ordinary data; dense adversarial data
  // (hardly any EOB to meet at) can need a workgroup's state handed on more often -- kJbStatusNotInStep alone says "not
  // yet": a retry with kJbSyncLaunchesMax launches, and then one with as many as the image has workgroups -- a launch
  // reads the exit states its left neighbours wrote in the launch BEFORE (the workgroups of a launch run side by side),
  // so a correct state is sure to cross one workgroup boundary per launch and no more: codes on which lanes do not fall
  // into step by themselves (every code of one length, say) need that many.  A launch in which nothing changes costs a
  // workgroup two loads.  Then the caller is told (JB_ERR_FORMAT) and the host decoder (jb_entropy_decode) is the
  // authority.  While kJbStatusNotInStep is set the other bits say nothing: a lane of the writing pass that started from
  // a state that is not its left neighbour's decodes noise, and noise has impossible bits and overruns.  Corrupt data
  // (the other bits WITHOUT "not in step") is never retried.
  const int enough = lay.n_sync_wg + 1 < kJbSyncLaunchesCap ? lay.n_sync_wg + 1 : kJbSyncLaunchesCap;
  int launches = kJbSyncLaunches;
  for (;;) {
    rc = huff_stage(ctx, s, s.h_blob, lay, coef_bytes, d_coef, ctx->stream, launches);
    if (rc) return rc;
    JB_HIP(ctx, hipMemcpyAsync(s.h_status, s.d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!(s.h_status[0] & kJbStatusNotInStep)) break;
    const int next = launches < kJbSyncLaunchesMax ? kJbSyncLaunchesMax : enough;
    if (next <= launches) break;
    launches = next;
  }
  s.n_status = 1;
  return check_status(ctx, s);
}

int jb_submit(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef, const uint16_t *qtabs,
              uint8_t *rgb, int64_t rgb_stride, int *ticket) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_submit: ctx is NULL");
  if (!desc || !coef || !qtabs || !rgb || !ticket) return fail(ctx, JB_ERR_NULL, "jb_submit: NULL pointer");
  const jb_image_desc frame = jb_draft_desc_(desc, ctx->draft);  // ("draft decode": the output is the draft frame)
  return submit_impl(ctx, desc, 1, coef, qtabs, rgb, rgb_stride, ticket, jb_out_plan_(&frame, 1, nullptr, nullptr, nullptr, nullptr, 0, ctx->orientation), false);
}

int jb_submit_batch(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const int16_t *coef,
                    const uint16_t *qtabs, uint8_t *rgb, int *ticket) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_submit_batch: ctx is NULL");
  if (!desc || !coef || !qtabs || !rgb || !ticket) return fail(ctx, JB_ERR_NULL, "jb_submit_batch: NULL pointer");
  const jb_image_desc frame = jb_draft_desc_(desc, ctx->draft);
  const JbOutPlan plan = jb_out_plan_(&frame, 1, nullptr, nullptr, nullptr, nullptr, 0, ctx->orientation);
  return submit_impl(ctx, desc, n_images, coef, qtabs, rgb, plan.row_stride, ticket, plan, false);
}

int jb_wait(jb_ctx *ctx, int ticket) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_wait: ctx is NULL");
  DeviceGuard guard(ctx->device);
  for (int i = 0; i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    if (s.ticket == ticket) {
      if (s.busy) {
        const int rc = slot_finish(ctx, s);
        if (rc) return rc;
        s.busy = false;
      }
      return check_status(ctx, s);
    }
  }
  return fail(ctx, JB_ERR_STATE, "ticket %d is not in flight (already waited for and its slot reused?)", ticket);
}

int jb_poll(jb_ctx *ctx, int ticket) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_poll: ctx is NULL");
  DeviceGuard guard(ctx->device);
  for (int i = 0; i < ctx->n_slots; i++) {
    Slot &s = ctx->slots[i];
    if (s.ticket == ticket) {
      if (!s.busy) return JB_OK;
      if (s.dl_pending.load(std::memory_order_acquire)) return JB_PENDING;
      hipError_t e = hipEventQuery(s.done);
      if (e == hipErrorNotReady) return JB_PENDING;
      if (e != hipSuccess) return fail(ctx, JB_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
      s.busy = false;
      return check_status(ctx, s);
    }
  }
  return fail(ctx, JB_ERR_STATE, "ticket %d is not in flight (already waited for and its slot reused?)", ticket);
}

int jb_blocks_to_rgb(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef, const uint16_t *qtabs,
                     uint8_t *rgb, int64_t rgb_stride) {
  int ticket = -1;
  int rc = jb_submit(ctx, desc, coef, qtabs, rgb, rgb_stride, &ticket);
  if (rc) return rc;
  return jb_wait(ctx, ticket);
}

}  // extern "C"

// ---- what the other files call: each is described where it is declared, jb_internal.h ----

int jb_decode_job_(jb_ctx *ctx, const JbHuffJob *job, uint8_t *rgb, const JbOutPlan &plan) {
  const bool timing = ctx->knobs.timing == 1;
  const double t0 = timing ? jb_now_s_() : 0;
  if (plan.status != JB_OK) return fail(ctx, plan.status, "%s", plan.why);
  int rc = jb_ctx_reserve(ctx, (size_t)job->geo.coef_bytes, (size_t)plan.image_bytes);
  if (rc) return rc;
  const double t1 = timing ? jb_now_s_() : 0;
  int ticket = -1;
  const JbHuffJob *jobs[1] = {job};
  rc = submit_jobs_impl(ctx, jobs, nullptr, nullptr, nullptr, nullptr, 1, rgb, plan.row_stride, nullptr, &ticket, plan, false);
  if (rc) return rc;
  const double t2 = timing ? jb_now_s_() : 0;
  rc = jb_wait(ctx, ticket);
  if (timing) fprintf(stderr, "jb_decode_job_: reserve %.3f ms, pack + submit %.3f ms, wait %.3f ms\n", (t1 - t0) * 1e3, (t2 - t1) * 1e3, (jb_now_s_() - t2) * 1e3);
  return rc;
}

int jb_submit_packed_(jb_ctx *ctx, const jb_image_desc *desc, const uint16_t *qtabs, const uint8_t *packed, const JbHuffLayout *lay,
                      uint8_t *rgb, uint32_t *status_out, int *ticket, const JbOutPlan &plan, int dst_device) {
  return submit_jobs_impl(ctx, nullptr, packed, lay, desc, qtabs, lay->n, rgb, plan.row_stride, status_out, ticket, plan, dst_device != 0);
}

int jb_submit_group_(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const int16_t *coef, const uint16_t *qtabs,
                     uint8_t *rgb, int *ticket, const JbOutPlan &plan, int dst_device) {
  return submit_impl(ctx, desc, n_images, coef, qtabs, rgb, plan.row_stride, ticket, plan, dst_device != 0);
}

int jb_blocks_to_rgb_plan_(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef, const uint16_t *qtabs, uint8_t *rgb,
                           const JbOutPlan &plan) {
  if (!ctx) return fail(nullptr, JB_ERR_NULL, "jb_blocks_to_rgb: ctx is NULL");
  if (!desc || !coef || !qtabs || !rgb) return fail(ctx, JB_ERR_NULL, "jb_blocks_to_rgb: NULL pointer");
  int ticket = -1;
  int rc = submit_impl(ctx, desc, 1, coef, qtabs, rgb, plan.row_stride, &ticket, plan, false);
  if (rc) return rc;
  return jb_wait(ctx, ticket);
}

// jb_wait in two halves for jb_batch.cpp, where many host threads share one context: the lookup
// runs under the caller's lock, the blocking wait outside it.  The slot stays marked busy; the
// ring's own synchronisation on reuse (jb_submit) then returns at once.
void *jb_wait_begin_(jb_ctx *ctx, int ticket) {
  for (int i = 0; i < ctx->n_slots; i++)
    if (ctx->slots[i].ticket == ticket) return ctx->slots[i].busy ? (void *)&ctx->slots[i] : nullptr;
  return nullptr;  // the slot has been reused: that submission completed long ago
}
int jb_wait_block_(jb_ctx *ctx, void *slot) {
  DeviceGuard guard(ctx->device);
  return slot_finish(ctx, *(Slot *)slot);
}

int jb_check_device_region_(int device, const void *p, size_t bytes) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  DeviceGuard guard(device);
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, JB_ERR_GEOMETRY, "not a pointer the HIP runtime knows (%s): device output needs device memory", hipGetErrorString(e));
  }
  if (a.type != hipMemoryTypeDevice) return fail(nullptr, JB_ERR_GEOMETRY, "device output needs device memory (hipMalloc), not host or managed memory");
  if (a.device != device) return fail(nullptr, JB_ERR_GEOMETRY, "the region is memory of device %d, the decoder drives device %d", a.device, device);
  // the last byte must belong to the same allocation
  hipPointerAttribute_t b;
  memset(&b, 0, sizeof b);
  e = hipPointerGetAttributes(&b, (const uint8_t *)p + (bytes ? bytes - 1 : 0));
  if (e != hipSuccess || b.type != hipMemoryTypeDevice || b.device != device) {
    (void)hipGetLastError();
    return fail(nullptr, JB_ERR_GEOMETRY, "the region of %zu bytes reaches beyond its device allocation", bytes);
  }
  return JB_OK;
}

void jb_ctx_set_last_desc_(jb_ctx *ctx, const jb_image_desc *d) { ctx->last_desc = *d; }
void jb_ctx_set_arithmetic_(jb_ctx *ctx, int arith) {
  if (ctx) ctx->arithmetic = arith;
}
void jb_ctx_set_draft_(jb_ctx *ctx, int denom) {
  if (ctx) ctx->draft = denom;
}
const JbKnobs *jb_ctx_knobs_(const jb_ctx *ctx) { return &ctx->knobs; }

void jb_ctx_set_download_age_(jb_ctx *ctx, uint64_t age) {
  if (ctx) ctx->dl_age.store(age, std::memory_order_relaxed);
}

// the one place an error text is kept: every file reports through it (jb_ctx.h fail() formats for it)
int jb_fail_(jb_ctx *ctx, int code, const char *msg) {
  if (ctx) ctx->error = msg;
  g_tls_error = msg;
  return code;
}

