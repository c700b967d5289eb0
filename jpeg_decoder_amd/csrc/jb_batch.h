// jb_batch.h -- what crosses jb_batch.cpp (the decoder object and the C ABI) and jb_batch_run.cpp (one device's run):
// the decoder, the buffers of a host thread, the output arena, run_single.  Only those two files include it, as
// jb_ctx.h serves jb_api.cpp and jb_seam.cpp.
#pragma once
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_batch_request.h"
#include "jb_hostmem.h"
#include "jb_internal.h"

constexpr int kMaxSlots = 4;
// pinned buffers per host thread = its submissions in flight: decode group k while k-1 is on the device.  Two, whatever
// the output: with the host's entropy stage the second slot is what lets a thread decode while its last group uploads;
// with the device's, 16 threads x 1 already keep the device and the link busy, and more than two changes nothing
// (profiles/r03/ab_slots_per_thread.txt: 1 / 2 / 3 / 4 slots, 1,024 1080p files left in HBM 42.5-43.3 / 41.1-41.5 /
// 41.1-41.9 / 40.4-40.6 k images/s, to the arena 8,250 / 8,180-8,260 / 8,150-8,170 / 8,160-8,200; 32 8192x8192 files
// left in HBM 2,060-2,170 / 1,730-1,810 / 1,750-1,780 / 1,760-1,770).  (Round 2's kernels wanted four for
// device-resident output -- +35 % -- because a group's launches took milliseconds: profiles/r02b/ab_pipeline_depth.txt.)
constexpr int kLaneSlots = 2;

// Small images are submitted in GROUPS: consecutive images of one geometry share one upload, one
// launch and one download (jb_submit_batch).  A submission costs tens of microseconds of driver
// calls under the shared mutex; at one submission per 679x451 image that capped the decoder at
// 11,000 images/s whatever the thread count, five times below what the entropy stage delivers.
constexpr size_t kGroupBytes = (size_t)16 << 20;  // coefficient bytes per group (and per pinned buffer)
constexpr int kMaxGroup = 64;

// what one host thread owns across runs: the pinned buffers its Huffman stage decodes into and,
// when the caller's pixel buffers are pageable (no arena), pinned pixel staging -- a
// device-to-host copy into pageable memory would block the device thread until the kernel has run
struct Lane {
  int16_t *coef[kMaxSlots] = {};
  uint8_t *out[kMaxSlots] = {};
  uint32_t *status[kMaxSlots] = {};  // per image of a group decoded on the device: its status word
  uint8_t *blob[kMaxSlots] = {};     // pinned: a device-entropy group packed for upload (jb_huff_pack_)
  size_t blob_cap[kMaxSlots] = {};
  int device_of_blobs = 0;
  // `need` bytes now; `full` = what a group of the full size would need by this group's bytes per image (the first
  // groups of a thread are smaller: a blob sized for one of them would be re-pinned, milliseconds, when a full group
  // comes to the slot)
  uint8_t *ensure_blob(int device, int s, size_t need, size_t full) {
    if (need <= blob_cap[s]) return blob[s];
    jb_pinned_free(blob[s]);
    blob_cap[s] = 0;
    if (full < need) full = need;
    const size_t cap = full + full / 4 + 65536;
    blob[s] = (uint8_t *)jb_pinned_alloc_on(device, cap);
    if (blob[s]) blob_cap[s] = cap;
    return blob[s];
  }
  size_t cap_coef = 0, cap_rgb = 0;
  bool has_out = false;
  int n_alloc = 0;  // slots with buffers
  int device_of_bufs = 0;

  // `device`: the GPU this lane's decoder drives -- the buffers are pinned against it and come from
  // its NUMA node, whatever device the allocating thread has current (a fresh std::thread: 0)
  // The coefficient staging of a slot is only pinned when the HOST entropy decoder first needs it (host
  // mode, or an image the device decoder handed back): with the entropy stage on the device it is never
  // touched -- 16 threads x 4 slots x 100 MB for 8192x8192 files, most of a second of page pinning.
  int16_t *coef_at(int s) {
    if (!coef[s]) coef[s] = (int16_t *)jb_pinned_alloc_on(device_of_bufs, cap_coef);
    return coef[s];
  }
  bool satisfied(size_t need_coef, size_t need_rgb, bool with_out, int n_slots) const {
    return status[0] && need_coef <= cap_coef && need_rgb <= cap_rgb && (has_out || !with_out) && n_alloc >= n_slots;
  }
  int ensure(int device, size_t need_coef, size_t need_rgb, bool with_out, int n_slots) {
    if (satisfied(need_coef, need_rgb, with_out, n_slots)) return JB_OK;
    if (need_coef < cap_coef) need_coef = cap_coef;
    if (need_rgb < cap_rgb) need_rgb = cap_rgb;
    release();
    int rc = JB_OK;
    device_of_bufs = device;
    for (int s = 0; s < n_slots && rc == JB_OK; s++) {
      if (rc == JB_OK && !status[s]) {
        status[s] = (uint32_t *)jb_pinned_alloc_on(device, 4 * 256);
        if (!status[s]) rc = JB_ERR_HIP;
      }
      if (with_out && rc == JB_OK) {
        out[s] = (uint8_t *)jb_pinned_alloc_on(device, need_rgb);
        if (!out[s]) rc = JB_ERR_HIP;
      }
    }
    if (rc == JB_OK) {
      cap_coef = need_coef;
      cap_rgb = need_rgb;
      has_out = with_out;
      n_alloc = n_slots;
    } else {
      release();
    }
    return rc;
  }
  void drop_out() {
    for (int s = 0; s < kMaxSlots; s++) {
      jb_pinned_free(out[s]);
      out[s] = nullptr;
    }
    has_out = false;
  }
  void release() {
    for (int s = 0; s < kMaxSlots; s++) {
      jb_pinned_free(coef[s]);
      coef[s] = nullptr;
      jb_pinned_free(status[s]);
      status[s] = nullptr;
      jb_pinned_free(blob[s]);
      blob[s] = nullptr;
      blob_cap[s] = 0;
    }
    drop_out();
    cap_coef = cap_rgb = 0;
    n_alloc = 0;
  }
};

// Pinned output arena (optional, jb_batch_decoder_set_arena): images are placed by an atomic bump
// pointer, so the device writes every pixel straight to its final place.
struct Arena {
  uint8_t *base = nullptr;
  size_t bytes = 0;
  bool on_device = false;  // the caller's DEVICE memory (jb_batch_decoder_set_device_output): the pixels stay in HBM
  bool owned = true;       // pinned memory this decoder allocated
  std::atomic<size_t> used{0};
  uint8_t *take(size_t n) {
    n = (n + 255) & ~(size_t)255;
    size_t at = used.fetch_add(n);
    if (at + n > bytes) return nullptr;
    return base + at;
  }
  // none, and the next one this decoder's own (the memory itself is the caller's to release first)
  void reset() { borrow(nullptr, 0, false), owned = true; }
  // the caller's memory, empty
  void borrow(uint8_t *at, size_t n, bool device) {
    base = at, bytes = n, used = 0;
    on_device = device, owned = false;
  }
};

struct jb_batch_decoder {
  JbKnobs knobs = jb_knobs_read();  // the environment as it was when the decoder was created (jb_knobs.h)
  int device = 0;
  std::vector<Lane> lanes;
  Arena own_arena;
  Arena *arena = &own_arena;  // a part of a multi-device decoder points at its parent's arena
  jb_ctx *ctx = nullptr;      // the one context all host threads of this device submit to
  size_t ctx_coef = 0, ctx_rgb = 0;
  int ctx_ring = 0;
  // (never more submissions in flight than the context's ring of 64 slots holds: a thread that found the ring full
  // would wait for the oldest submission while holding the lock every other thread submits under)
  int slots() const {
    const int want = kLaneSlots, fit = lanes.empty() ? want : 64 / (int)lanes.size();
    return want < fit ? want : fit < 1 ? 1 : fit;
  }
  // the caller's device region as it was given (jb_batch_decoder_set_device_output[s]); submit / collect
  // split it between the two sides, run() uses all of it
  uint8_t *region_base = nullptr;
  size_t region_bytes = 0;
  // how this decoder was made: its twin (submit / collect) is made the same way
  std::vector<int> made_devices;
  bool made_multi = false;
  int made_threads = 0;
  size_t made_coef = 0, made_rgb = 0;
  OutputRequest out;  // scale and format of the output: on this decoder, its parts and its twin alike
  // jb_batch_decoder_submit / _collect: up to two batches in flight, batch k on side k & 1 -- side 0 is this
  // decoder, side 1 its twin (same devices, threads and sizes, its own ring, staging and arena) -- so that the
  // start-up of one batch (headers, first groups) runs under the tail of the other (last kernels, last downloads)
  struct Flight {
    std::thread th;
    bool busy = false;
    int ticket = -1;
    int rc = JB_OK;
    std::string text;
    double times[4] = {0, 0, 0, 0};
    std::vector<std::string> path_text;  // the batch's paths, copied: the caller's array need not outlive submit
    std::vector<const char *> path_ptr;
    PerFileOwned per;  // the batch's rectangles, views and chains, copied like the paths
  };
  Flight flights[2];
  int tickets = 0;
  jb_batch_decoder *twin = nullptr;
  bool split_for_sides = false;  // the outputs are arranged for submit / collect (twin arena, halves of the regions)
  bool in_flight() const { return flights[0].busy || flights[1].busy; }
  // multi-device decoder (jb_batch_decoder_create_multi): one single-device decoder per listed
  // device; this object then only deals the files out and owns the shared arena
  std::vector<jb_batch_decoder *> parts;

  // (jb_batch.cpp) the context, then everything, sized for images of up to (coef, rgb) bytes
  int ensure_ctx(size_t need_coef, size_t need_rgb);
  int ensure_all(size_t need_coef, size_t need_rgb, int n_lanes, size_t ring_coef = 0, size_t ring_rgb = 0);
};

// one device's share of a run; `top` = this decoder owns the arena (and recycles it)
int run_single(jb_batch_decoder *d, const char *const *paths, int n_paths, const PerFile &per, uint8_t **rgb, int32_t *widths,
               int32_t *heights, int *statuses, double *times, bool top);
