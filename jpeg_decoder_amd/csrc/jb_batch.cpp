// jb_batch.cpp -- multi-threaded decode(path) over a batch of files (include/jpegblk.h,
// jb_decode_batch / jb_batch_decoder_*).  The reference decodes one file per process,
// single-threaded (jpeg.cpp:916-929); images are independent, so the batch parallelises by image.
//
// This file is the decoder object and the C ABI: create / destroy, the arena and the device regions, the two sides of
// submit / collect, the deal of a multi-device run, the entry points and the setters.  What a decoder is asked for and
// the rules of it: jb_batch_request.h.  One device's run (N host threads feeding ONE shared jb_ctx): jb_batch_run.cpp.
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "jb_batch.h"

int jb_batch_decoder::ensure_ctx(size_t need_coef, size_t need_rgb) {
  // ring depth = everything the host threads can have in flight, so that a submission never blocks a
  // thread that could be decoding; device memory is not the scarce resource here (32 slots of
  // 8192x8192 4:2:0 are 13 GB of 288)
  int ring = slots() * (int)lanes.size();
  if (ring > 64) ring = 64;
  if (ctx && need_coef <= ctx_coef && need_rgb <= ctx_rgb && ring <= ctx_ring) return JB_OK;
  if (need_coef < ctx_coef) need_coef = ctx_coef;
  if (need_rgb < ctx_rgb) need_rgb = ctx_rgb;
  jb_ctx_destroy(ctx);
  ctx = nullptr;
  ctx_coef = ctx_rgb = 0;
  ctx_ring = 0;
  int rc = jb_ctx_create(device, need_coef, need_rgb, ring, &ctx);
  if (rc == JB_OK) {
    ctx_coef = need_coef;
    ctx_rgb = need_rgb;
    ctx_ring = ring;
  }
  return rc;
}
// size everything for images of up to (coef, rgb) bytes; page pinning is slow, so the host
// threads' buffers are created in parallel
int jb_batch_decoder::ensure_all(size_t need_coef, size_t need_rgb, int n_lanes, size_t ring_coef, size_t ring_rgb) {
  // (the ring slots may be larger than the lanes' pinned buffers: groups decoded on the device)
  int rc = ensure_ctx(ring_coef > need_coef ? ring_coef : need_coef, ring_rgb > need_rgb ? ring_rgb : need_rgb);
  if (rc != JB_OK) return rc;
  const bool with_out = !arena->base;
  {
    // nothing to make (every run after the first): no threads either -- sixteen of them started and joined for
    // nothing took half a millisecond of every run
    bool all = true;
    const int n_slots_now = slots();
    for (int i = 0; i < n_lanes && all; i++) all = lanes[(size_t)i].satisfied(need_coef, need_rgb, with_out, n_slots_now);
    if (all) return JB_OK;
  }
  std::vector<std::thread> th;
  std::vector<int> rcs((size_t)n_lanes, JB_OK);
  const int dev = device;
  const int n_slots = slots();
  for (int i = 0; i < n_lanes; i++)
    th.emplace_back([&, i, n_slots] { rcs[(size_t)i] = lanes[(size_t)i].ensure(dev, need_coef, need_rgb, with_out, n_slots); });
  for (auto &x : th) x.join();
  for (int r : rcs)
    if (r != JB_OK) return jb_fail_(nullptr, r, "pinned host allocation failed");
  return JB_OK;
}

namespace {

int clamp_threads(int n_threads, const JbKnobs &knobs) {
  if (n_threads < 1) n_threads = 1;
  if (n_threads > 64) n_threads = 64;  // one ring slot each at least (64 host threads decode 30 Gpixel/s: far beyond the link)
  // no more entropy threads than CPUs this process may use (JPEGBLK_OVERSUBSCRIBE=1 lifts that)
  if (!knobs.oversubscribe && n_threads > jb_available_cpus_()) n_threads = jb_available_cpus_();
  return n_threads;
}

int create_single(int device_id, int n_threads, size_t max_coef_bytes, size_t max_rgb_bytes, jb_batch_decoder **out) {
  jb_batch_decoder *d = new jb_batch_decoder();
  d->device = device_id;
  d->lanes.resize((size_t)n_threads);
  // the context exists from the start (also when the buffers are sized lazily), so that a
  // missing or unusable device is reported here
  // With sizes given, everything a batch of such images needs is built HERE -- the staging of the host path
  // (groups of kGroupBytes) and, where the entropy stage runs on the device, ring slots for groups of
  // JPEGBLK_DEV_GROUP_MB -- so that the first run does not spend 45-120 ms growing them (a decoder created
  // with (0, 0) sizes itself from its first batch instead).
  int rc;
  if (max_coef_bytes && max_rgb_bytes) {
    size_t group = kGroupBytes;
    if (d->knobs.group_mb >= 0) group = (size_t)d->knobs.group_mb << 20;
    const size_t mc = max_coef_bytes < group ? group : max_coef_bytes, mr = max_rgb_bytes < group ? group : max_rgb_bytes;
    size_t ring = 0;
    if (d->knobs.gpu_huffman != 0) {
      ring = (size_t)(d->knobs.dev_group_mb >= 0 ? d->knobs.dev_group_mb : 96) << 20;
      if (ring > (size_t)kMaxGroup * mc) ring = (size_t)kMaxGroup * mc;
    }
    rc = d->ensure_all(mc, mr, n_threads, ring, ring);
  } else {
    rc = d->ensure_ctx(128, 192);
  }
  if (rc != JB_OK) {
    std::string text = jb_last_error(nullptr);
    jb_batch_decoder_destroy(d);
    return jb_fail_(nullptr, rc, text.c_str());
  }
  *out = d;
  return JB_OK;
}

}  // namespace

extern "C" int jb_batch_decoder_create(int device_id, int n_threads, size_t max_coef_bytes,
                                       size_t max_rgb_bytes, jb_batch_decoder **out) {
  if (!out) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_create: out is NULL");
  *out = nullptr;
  int rc = create_single(device_id, clamp_threads(n_threads, jb_knobs_read()), max_coef_bytes, max_rgb_bytes, out);
  if (rc == JB_OK) {
    (*out)->made_devices.assign(1, device_id);
    (*out)->made_threads = n_threads;
    (*out)->made_coef = max_coef_bytes;
    (*out)->made_rgb = max_rgb_bytes;
  }
  return rc;
}

extern "C" int jb_batch_decoder_create_multi(const int *device_ids, int n_devices, int n_threads,
                                             size_t max_coef_bytes, size_t max_rgb_bytes, jb_batch_decoder **out) {
  if (!out || !device_ids) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_create_multi: NULL pointer");
  *out = nullptr;
  if (n_devices < 1 || n_devices > 64) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_create_multi: 1..64 devices");
  n_threads = clamp_threads(n_threads, jb_knobs_read());
  if (n_threads < n_devices) n_threads = n_devices;  // every device needs a host thread to feed it
  jb_batch_decoder *top = new jb_batch_decoder();
  top->device = device_ids[0];
  top->made_devices.assign(device_ids, device_ids + n_devices);
  top->made_multi = true;
  top->made_threads = n_threads;
  top->made_coef = max_coef_bytes;
  top->made_rgb = max_rgb_bytes;
  for (int k = 0; k < n_devices; k++) {
    // host threads are dealt out evenly; the first (n_threads % n_devices) devices get one more
    const int share = n_threads / n_devices + (k < n_threads % n_devices ? 1 : 0);
    jb_batch_decoder *part = nullptr;
    int rc = create_single(device_ids[k], share, max_coef_bytes, max_rgb_bytes, &part);
    if (rc != JB_OK) {
      std::string text = jb_last_error(nullptr);
      jb_batch_decoder_destroy(top);
      return jb_fail_(nullptr, rc, text.c_str());
    }
    part->arena = &top->own_arena;
    top->parts.push_back(part);
  }
  *out = top;
  return JB_OK;
}

extern "C" void jb_batch_decoder_destroy(jb_batch_decoder *d) {
  if (!d) return;
  for (auto &f : d->flights)
    if (f.th.joinable()) f.th.join();  // batches still in flight finish first (their results are dropped)
  jb_batch_decoder_destroy(d->twin);
  for (jb_batch_decoder *p : d->parts) jb_batch_decoder_destroy(p);
  for (auto &l : d->lanes) l.release();
  jb_ctx_destroy(d->ctx);
  if (d->own_arena.owned) jb_pinned_free(d->own_arena.base);
  delete d;
}

extern "C" int jb_batch_decoder_set_arena(jb_batch_decoder *d, size_t bytes) {
  if (!d) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_set_arena: decoder is NULL");
  if (d->arena != &d->own_arena) return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_set_arena: set the arena on the multi-device decoder, not on one of its parts");
  if (d->in_flight()) return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_set_arena: batches are in flight (collect them first)");
  d->split_for_sides = false;  // the next submit arranges the two sides' outputs again
  if (d->twin) (void)jb_batch_decoder_set_arena(d->twin, 0);  // (its arena or region halves go as well; the next submit gives it new ones)
  d->region_base = nullptr;
  d->region_bytes = 0;
  for (jb_batch_decoder *part : d->parts) part->region_base = nullptr, part->region_bytes = 0;
  if (d->own_arena.owned) jb_pinned_free(d->own_arena.base);
  d->own_arena.reset();
  for (jb_batch_decoder *part : d->parts)  // (device regions of a multi-device decoder are forgotten as well)
    if (part->arena == &part->own_arena) {
      part->own_arena.reset();
      part->arena = &d->own_arena;
    }
  if (bytes) {
    // pinned against the (first) device of the decoder; portable, so every device copies into it
    d->own_arena.base = (uint8_t *)jb_pinned_alloc_on(d->device, bytes);
    if (!d->own_arena.base) return jb_fail_(nullptr, JB_ERR_HIP, "jb_batch_decoder_set_arena: pinned allocation failed");
    d->own_arena.bytes = bytes;
    // no pixel staging while an arena takes the pixels
    for (auto &l : d->lanes) l.drop_out();
    for (jb_batch_decoder *p : d->parts)
      for (auto &l : p->lanes) l.drop_out();
  }
  return JB_OK;
}

extern "C" int jb_batch_decoder_set_device_output(jb_batch_decoder *d, void *d_base, size_t bytes) {
  if (!d) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_set_device_output: decoder is NULL");
  if (!d->parts.empty() || d->arena != &d->own_arena)
    return jb_fail_(nullptr, JB_ERR_UNSUPPORTED, "jb_batch_decoder_set_device_output: a multi-device decoder takes one region per device (jb_batch_decoder_set_device_outputs)");
  if ((d_base == nullptr) != (bytes == 0)) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_set_device_output: pointer and size must both be given or both be zero");
  if ((uintptr_t)d_base & 255) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_set_device_output: the region must be 256-byte aligned");
  if (d->in_flight()) return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_set_device_output: batches are in flight (collect them first)");
  int rc = d_base ? jb_check_device_region_(d->device, d_base, bytes) : (int)JB_OK;
  if (rc != JB_OK) return rc;
  rc = jb_batch_decoder_set_arena(d, 0);  // releases a pinned arena, forgets an earlier device region
  if (rc != JB_OK) return rc;
  if (d_base) {
    d->own_arena.borrow((uint8_t *)d_base, bytes, true);
    d->region_base = (uint8_t *)d_base;
    d->region_bytes = bytes;
    for (auto &l : d->lanes) l.drop_out();  // no pixel staging: nothing is downloaded
  }
  return JB_OK;
}

// the multi-device form: one region per listed device, in the order of jb_batch_decoder_create_multi
extern "C" int jb_batch_decoder_set_device_outputs(jb_batch_decoder *d, void *const *d_bases, const size_t *bytes, int n) {
  if (!d) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_set_device_outputs: decoder is NULL");
  if (d->parts.empty()) {
    if (n != 1 || !d_bases || !bytes) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_set_device_outputs: a single-device decoder takes one region");
    return jb_batch_decoder_set_device_output(d, d_bases[0], bytes[0]);
  }
  if (d->in_flight()) return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_set_device_outputs: batches are in flight (collect them first)");
  const bool off = n == 0;
  if (!off && (n != (int)d->parts.size() || !d_bases || !bytes))
    return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_set_device_outputs: one region per listed device (or n = 0: host output again)");
  if (!off)
    for (int k = 0; k < n; k++)
      if (!d_bases[k] || !bytes[k] || ((uintptr_t)d_bases[k] & 255))
        return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_set_device_outputs: every region needs a 256-byte aligned pointer and a size");
  int rc = JB_OK;
  for (int k = 0; !off && k < n && rc == JB_OK; k++) rc = jb_check_device_region_(d->parts[(size_t)k]->device, d_bases[k], bytes[k]);
  if (rc != JB_OK) return rc;
  rc = jb_batch_decoder_set_arena(d, 0);  // a shared pinned arena and device regions exclude each other
  if (rc != JB_OK) return rc;
  for (size_t k = 0; k < d->parts.size(); k++) {
    jb_batch_decoder *part = d->parts[k];
    if (off) part->own_arena.reset();
    else part->own_arena.borrow((uint8_t *)d_bases[k], bytes[k], true);
    part->region_base = part->own_arena.base;
    part->region_bytes = part->own_arena.bytes;
    part->arena = off ? &d->own_arena : &part->own_arena;  // (host output: the parts share the top decoder's arena, if any)
    if (!off)
      for (auto &l : part->lanes) l.drop_out();
  }
  return JB_OK;
}

namespace {

// the decoder, its parts and its twin (with the twin's parts) deliver the same output
void set_output_all(jb_batch_decoder *d, const OutputRequest &out) {
  if (!d) return;
  d->out = out;
  for (jb_batch_decoder *p : d->parts) set_output_all(p, out);
  set_output_all(d->twin, out);
}

// the single-device decoders a decoder consists of
std::vector<jb_batch_decoder *> singles_of(jb_batch_decoder *d) {
  if (d->parts.empty()) return std::vector<jb_batch_decoder *>(1, d);
  return d->parts;
}

// Where the pixels of the two sides go.  for_sides = false (jb_batch_decoder_run): this decoder has all of the
// caller's device region(s).  for_sides = true (submit / collect): side 0 writes into the first half of every
// region and the twin into the second; with a pinned arena (or none) the twin has one of the same size of its own.
int arrange_outputs(jb_batch_decoder *d, bool for_sides) {
  std::vector<jb_batch_decoder *> mine = singles_of(d), theirs;
  if (d->twin) theirs = singles_of(d->twin);
  bool any_region = false;
  for (jb_batch_decoder *m : mine) any_region = any_region || m->region_base;
  if (for_sides && d->twin) {
    bool twin_on_device = false;
    for (jb_batch_decoder *t : theirs) twin_on_device = twin_on_device || t->own_arena.on_device;
    const size_t want = (!any_region && d->own_arena.base && d->own_arena.owned) ? d->own_arena.bytes : 0;
    const size_t have = (d->twin->own_arena.base && d->twin->own_arena.owned) ? d->twin->own_arena.bytes : 0;
    if (want != have || twin_on_device) {
      int rc = jb_batch_decoder_set_arena(d->twin, want);
      if (rc != JB_OK) return rc;
    }
  }
  for (size_t k = 0; k < mine.size(); k++) {
    jb_batch_decoder *m = mine[k];
    if (!m->region_base) continue;
    const size_t half = (m->region_bytes / 2) & ~(size_t)255;
    m->own_arena.bytes = for_sides ? half : m->region_bytes;
    if (for_sides && d->twin) {
      jb_batch_decoder *t = theirs[k];
      t->own_arena.borrow(m->region_base + half, half, true);
      t->arena = &t->own_arena;
      for (auto &l : t->lanes) l.drop_out();
    }
  }
  d->split_for_sides = for_sides;
  return JB_OK;
}

int run_impl(jb_batch_decoder *d, const char *const *paths, int n_paths, const PerFile &per, uint8_t **rgb, int32_t *widths,
             int32_t *heights, int *statuses, double *times) {
  if (d->parts.empty()) return run_single(d, paths, n_paths, per, rgb, widths, heights, statuses, times, d->arena == &d->own_arena);
  // multi-device: file i -> part i % n_parts (images are independent: nothing crosses devices);
  // every part runs its share on its own host threads, concurrently with the others
  const int np = (int)d->parts.size();
  d->own_arena.used = 0;
  for (jb_batch_decoder *part : d->parts)
    if (part->arena == &part->own_arena) part->own_arena.used = 0;  // device regions: recycled by every run
  const double t0 = jb_now_s_();
  struct Share {
    std::vector<const char *> paths;
    PerFileOwned per;  // (rectangle i, file i's k views and their chains go where file i goes)
    std::vector<uint8_t *> rgb;
    std::vector<int32_t> w, h;
    std::vector<int> st;
    double times[4] = {0, 0, 0, 0};
    int rc = JB_OK;
    std::string text;
  };
  std::vector<Share> sh((size_t)np);
  for (int i = 0; i < n_paths; i++) sh[(size_t)(i % np)].paths.push_back(paths[i]);
  std::vector<std::thread> th;
  for (int k = 0; k < np; k++) {
    Share &s = sh[(size_t)k];
    const size_t n = s.paths.size();
    s.rgb.assign(n, nullptr);
    s.w.assign(n, 0);
    s.h.assign(n, 0);
    s.st.assign(n, JB_OK);
    s.per.copy(per, n_paths, k, np);
    th.emplace_back([&, k] {
      Share &m = sh[(size_t)k];
      m.rc = run_single(d->parts[(size_t)k], m.paths.data(), (int)m.paths.size(), m.per.get(), m.rgb.data(),
                        m.w.data(), m.h.data(), m.st.data(), m.times, false);
      if (m.rc != JB_OK) m.text = jb_last_error(nullptr);  // thread-local text: fetch it on this thread
    });
  }
  for (auto &x : th) x.join();
  int rc = JB_OK;
  std::string text;
  for (int i = 0; i < n_paths; i++) {
    Share &s = sh[(size_t)(i % np)];
    const size_t j = (size_t)(i / np);
    rgb[i] = s.rgb[j];
    widths[i] = s.w[j];
    heights[i] = s.h[j];
    statuses[i] = s.st[j];
  }
  for (int k = 0; k < np; k++)
    if (rc == JB_OK && sh[(size_t)k].rc != JB_OK) {
      rc = sh[(size_t)k].rc;
      text = sh[(size_t)k].text;
    }
  if (times) {
    times[0] = jb_now_s_() - t0;
    times[1] = times[2] = times[3] = 0;
    for (int k = 0; k < np; k++)
      for (int j = 1; j < 4; j++) times[j] += sh[(size_t)k].times[j];
  }
  return rc == JB_OK ? JB_OK : jb_fail_(nullptr, rc, text.c_str());
}

// what a refused call reports: "<entry point>: <why>"
int refuse(const char *fn, int status, const char *why) { return jb_fail_(nullptr, status, (std::string(fn) + ": " + why).c_str()); }
const char *const kInFlightText = "batches are in flight (collect them first)";

// every jb_batch_decoder_run*: `per` is what the entry point's builder made of its own arguments (jb_batch_request.h)
int run_checked(jb_batch_decoder *d, const char *const *paths, int n_paths, const PerFile &per, uint8_t **rgb, int32_t *widths,
                int32_t *heights, int *statuses, double *times, const char *fn) {
  if (per.bad.status != JB_OK) return refuse(fn, per.bad.status, per.bad.why);
  if (!d || !paths || !rgb || !widths || !heights || !statuses) return refuse(fn, JB_ERR_NULL, "NULL pointer");
  if (n_paths < 0) return refuse(fn, JB_ERR_GEOMETRY, "negative count");
  if (d->in_flight()) return refuse(fn, JB_ERR_STATE, kInFlightText);
  int rc = per.check(d->out, n_paths, fn);
  if (rc == JB_OK && d->split_for_sides) rc = arrange_outputs(d, false);
  if (rc != JB_OK) return rc;
  return run_impl(d, paths, n_paths, per, rgb, widths, heights, statuses, times);
}

// every jb_batch_decoder_submit*
int submit_checked(jb_batch_decoder *d, const char *const *paths, int n_paths, const PerFile &per, uint8_t **rgb, int32_t *widths,
                   int32_t *heights, int *statuses, int *ticket, const char *fn) {
  if (per.bad.status != JB_OK) return refuse(fn, per.bad.status, per.bad.why);
  if (!d || !paths || !rgb || !widths || !heights || !statuses || !ticket)
    return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_submit: NULL pointer");
  if (n_paths < 0) return jb_fail_(nullptr, JB_ERR_GEOMETRY, "jb_batch_decoder_submit: negative count");
  if (d->arena != &d->own_arena && d->parts.empty())
    return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_submit: submit to the multi-device decoder, not to one of its parts");
  for (int i = 0; i < n_paths; i++)
    if (!paths[i]) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_submit: NULL path");
  // (what the request refuses of the per-file arrays carries the name of the entry point without its _color)
  int rc = per.check(d->out, n_paths, per.rois ? "jb_batch_decoder_submit_crops" : per.n_groups > 0 ? "jb_batch_decoder_submit_view_groups"
                                                                                                      : "jb_batch_decoder_submit_views");
  if (rc != JB_OK) return rc;
  const int side = d->tickets & 1;
  jb_batch_decoder::Flight &f = d->flights[side];
  if (f.busy) return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_submit: two batches are in flight: collect the older one first");
  if (!d->twin) {
    jb_batch_decoder *t = nullptr;
    rc = d->made_multi ? jb_batch_decoder_create_multi(d->made_devices.data(), (int)d->made_devices.size(), d->made_threads,
                                                       d->made_coef, d->made_rgb, &t)
                       : jb_batch_decoder_create(d->made_devices.empty() ? d->device : d->made_devices[0],
                                                 d->made_threads > 0 ? d->made_threads : (int)d->lanes.size(), d->made_coef,
                                                 d->made_rgb, &t);
    if (rc != JB_OK) return rc;
    d->twin = t;
    d->split_for_sides = false;
    set_output_all(t, d->out);
  }
  if (!d->split_for_sides) {  // (only ever the case with nothing in flight: every call that clears it refuses otherwise)
    rc = arrange_outputs(d, true);
    if (rc != JB_OK) return rc;
  }
  f.path_text.assign(paths, paths + n_paths);
  f.path_ptr.resize((size_t)n_paths);
  for (int i = 0; i < n_paths; i++) f.path_ptr[(size_t)i] = f.path_text[(size_t)i].c_str();
  f.per.copy(per, n_paths);
  f.busy = true;
  f.ticket = d->tickets++;
  f.rc = JB_OK;
  f.text.clear();
  jb_batch_decoder *const target = side == 0 ? d : d->twin;
  jb_batch_decoder::Flight *const fp = &f;
  try {
    f.th = std::thread([=] {
      fp->rc = run_impl(target, fp->path_ptr.data(), n_paths, fp->per.get(), rgb, widths, heights, statuses, fp->times);
      if (fp->rc != JB_OK) fp->text = jb_last_error(nullptr);  // thread-local text: fetch it on this thread
    });
  } catch (const std::exception &e) {  // no thread to be had: nothing is in flight
    f.busy = false;
    d->tickets--;
    return jb_fail_(nullptr, JB_ERR_CAPACITY, "jb_batch_decoder_submit: cannot start a thread");
  }
  *ticket = f.ticket;
  return JB_OK;
}

}  // namespace

// The twelve entry points: the builder of the shape of the per-file arguments (jb_batch_request.h), and the call.

extern "C" int jb_batch_decoder_run(jb_batch_decoder *d, const char *const *paths, int n_paths,
                                    uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile{}, rgb, widths, heights, statuses, times, "jb_batch_decoder_run");
}

extern "C" int jb_batch_decoder_run_crops(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_roi *rois,
                                          uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile::of_crops(rois), rgb, widths, heights, statuses, times, "jb_batch_decoder_run_crops");
}

extern "C" int jb_batch_decoder_run_views(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, int views_per_image,
                                          uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile::of_views(views, views_per_image), rgb, widths, heights, statuses, times, "jb_batch_decoder_run_views");
}

extern "C" int jb_batch_decoder_run_views_color(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, int views_per_image, const jb_color_chain *colors,
                                                uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile::of_views(views, views_per_image, colors), rgb, widths, heights, statuses, times, "jb_batch_decoder_run_views_color");
}

extern "C" int jb_batch_decoder_run_view_groups(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, const jb_view_group *groups, int n_groups,
                                                uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile::of_groups(views, groups, n_groups), rgb, widths, heights, statuses, times, "jb_batch_decoder_run_view_groups");
}

extern "C" int jb_batch_decoder_run_view_groups_color(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, const jb_view_group *groups, int n_groups, const jb_color_chain *colors,
                                                      uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times) {
  return run_checked(d, paths, n_paths, PerFile::of_groups(views, groups, n_groups, colors), rgb, widths, heights, statuses, times, "jb_batch_decoder_run_view_groups_color");
}

extern "C" int jb_batch_decoder_submit(jb_batch_decoder *d, const char *const *paths, int n_paths,
                                       uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile{}, rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit");
}

extern "C" int jb_batch_decoder_submit_crops(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_roi *rois,
                                             uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile::of_crops(rois), rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit_crops");
}

extern "C" int jb_batch_decoder_submit_views(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, int views_per_image,
                                             uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile::of_views(views, views_per_image), rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit_views");
}

extern "C" int jb_batch_decoder_submit_views_color(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, int views_per_image, const jb_color_chain *colors,
                                                   uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile::of_views(views, views_per_image, colors), rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit_views_color");
}

extern "C" int jb_batch_decoder_submit_view_groups(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, const jb_view_group *groups, int n_groups,
                                                   uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile::of_groups(views, groups, n_groups), rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit_view_groups");
}

extern "C" int jb_batch_decoder_submit_view_groups_color(jb_batch_decoder *d, const char *const *paths, int n_paths, const jb_view *views, const jb_view_group *groups, int n_groups, const jb_color_chain *colors,
                                                         uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket) {
  return submit_checked(d, paths, n_paths, PerFile::of_groups(views, groups, n_groups, colors), rgb, widths, heights, statuses, ticket, "jb_batch_decoder_submit_view_groups_color");
}

extern "C" int jb_batch_decoder_collect(jb_batch_decoder *d, int ticket, double *times) {
  if (!d) return jb_fail_(nullptr, JB_ERR_NULL, "jb_batch_decoder_collect: decoder is NULL");
  jb_batch_decoder::Flight &f = d->flights[ticket & 1];
  if (ticket < 0 || !f.busy || f.ticket != ticket)
    return jb_fail_(nullptr, JB_ERR_STATE, "jb_batch_decoder_collect: no such batch in flight");
  f.th.join();
  f.busy = false;
  if (times)
    for (int j = 0; j < 4; j++) times[j] = f.times[j];
  return f.rc == JB_OK ? JB_OK : jb_fail_(nullptr, f.rc, f.text.c_str());
}

namespace {

// The shell of every setter of the output request: the decoder, the setter's own look at its argument (`arg`: in front
// of or behind the look at what is in flight -- the setters differ, and callers see which refusal comes first), then
// the edit of ONE field of a copy of the request, THE rule (OutputRequest::verdict, with the setter's own words for
// what the plan refuses) and the request to the decoder, its parts and its twin.
constexpr JbVerdict kFine = {JB_OK, nullptr};
template <class Edit>
int set_request(jb_batch_decoder *d, const char *fn, bool arg_first, JbVerdict arg, Edit edit, const char *combined = nullptr,
                const char *other = nullptr) {
  if (!d) return refuse(fn, JB_ERR_NULL, "decoder is NULL");
  if (arg_first && arg.status != JB_OK) return refuse(fn, arg.status, arg.why);
  if (d->in_flight()) return refuse(fn, JB_ERR_STATE, kInFlightText);
  if (arg.status != JB_OK) return refuse(fn, arg.status, arg.why);
  OutputRequest out = d->out;
  edit(out);
  const JbVerdict v = out.verdict(combined, other);
  if (v.status != JB_OK) return refuse(fn, v.status, v.why);
  set_output_all(d, out);
  return JB_OK;
}

JbVerdict denom_check(int denom) {
  return denom == 1 || denom == 2 || denom == 4 || denom == 8 ? kFine : JbVerdict{JB_ERR_GEOMETRY, "denom is not 1, 2, 4 or 8"};
}

// the plan function decides what a filter and a fit are: here with a target of one pixel
bool plan_takes(int filter, const jb_fit *fit) {
  const jb_image_desc one = {1, 1, 1, 1, {0, 0, 0}, 0};
  const JbTarget probe = {1, 1, filter, 0};
  return jb_out_plan_(&one, 1, nullptr, nullptr, &probe, nullptr, 0, 1, fit).status == JB_OK;
}

}  // namespace

extern "C" int jb_batch_decoder_set_scale(jb_batch_decoder *d, int denom) {
  return set_request(d, "jb_batch_decoder_set_scale", true, denom_check(denom), [=](OutputRequest &out) { out.scale = denom; },
                     "a planar output format, a rectangle or a target size is set: it cannot be combined with a scale");
}

extern "C" int jb_batch_decoder_set_output_format(jb_batch_decoder *d, const jb_output_spec *spec) {
  const JbVerdict arg = !spec                                ? JbVerdict{JB_ERR_NULL, "spec is NULL"}
                        : jb_tight_spec_check_(spec) != JB_OK ? JbVerdict{JB_ERR_GEOMETRY, &JB_TIGHT_SPEC_TEXT[2]}  // (without its ": ")
                                                              : kFine;
  return set_request(d, "jb_batch_decoder_set_output_format", true, arg, [=](OutputRequest &out) { out.spec = *spec; },
                     "the decoder's scale is not 1: a planar output format cannot be combined with it");
}

extern "C" int jb_batch_decoder_set_roi(jb_batch_decoder *d, const jb_roi *roi) {
  return set_request(d, "jb_batch_decoder_set_roi", false, kFine, [=](OutputRequest &out) { out.has_roi = roi != nullptr, out.roi = roi ? *roi : jb_roi{}; },
                     "the decoder's scale is not 1: a rectangle cannot be combined with it", "no frame can hold this rectangle");
}

extern "C" int jb_batch_decoder_set_resize(jb_batch_decoder *d, int32_t out_w, int32_t out_h) {
  auto edit = [=](OutputRequest &out) {
    out.has_resize = !(out_w == 0 && out_h == 0);
    out.target = JbTarget{out_w, out_h, out.target.filter, 0};  // ((0, 0): none; the filter stays)
  };
  return set_request(d, "jb_batch_decoder_set_resize", false, kFine, edit, "the decoder's scale is not 1: a target size cannot be combined with it",
                     "the target size is outside 1..65535");
}

extern "C" int jb_batch_decoder_set_filter(jb_batch_decoder *d, int filter) {
  const JbVerdict arg = plan_takes(filter, nullptr) ? kFine : JbVerdict{JB_ERR_GEOMETRY, "unknown resampling filter"};
  return set_request(d, "jb_batch_decoder_set_filter", false, arg, [=](OutputRequest &out) { out.target.filter = filter; });
}

extern "C" int jb_batch_decoder_set_fit(jb_batch_decoder *d, const jb_fit *fit) {
  const JbVerdict arg = plan_takes(0, fit) ? kFine : JbVerdict{JB_ERR_GEOMETRY, "unknown mode or anchor (or a reserved field is not 0)"};
  return set_request(d, "jb_batch_decoder_set_fit", false, arg, [=](OutputRequest &out) { out.fit = fit ? *fit : jb_fit{}; });
}

extern "C" int jb_batch_decoder_set_arithmetic(jb_batch_decoder *d, int arith) {
  const JbVerdict arg = arith == JB_ARITH_REFERENCE || arith == JB_ARITH_LIBJPEG ? kFine : JbVerdict{JB_ERR_GEOMETRY, "unknown arithmetic"};
  return set_request(d, "jb_batch_decoder_set_arithmetic", true, arg, [=](OutputRequest &out) { out.arith = arith; });
}

extern "C" int jb_batch_decoder_set_orientation(jb_batch_decoder *d, int orientation) {
  const JbVerdict arg = orientation >= 0 && orientation <= 8 ? kFine : JbVerdict{JB_ERR_GEOMETRY, "outside 0..8"};
  return set_request(d, "jb_batch_decoder_set_orientation", true, arg, [=](OutputRequest &out) { out.orient = orientation; });
}

extern "C" int jb_batch_decoder_set_draft(jb_batch_decoder *d, int denom) {
  return set_request(d, "jb_batch_decoder_set_draft", true, denom_check(denom), [=](OutputRequest &out) { out.draft = denom; });
}

extern "C" long long jb_batch_decoder_device_entropy_images(const jb_batch_decoder *d) {
  if (!d) return 0;
  long long n = d->ctx ? jb_ctx_device_entropy_images(d->ctx) : 0;
  for (const jb_batch_decoder *p : d->parts) n += jb_batch_decoder_device_entropy_images(p);
  if (d->twin) n += jb_batch_decoder_device_entropy_images(d->twin);  // (the second side of submit / collect)
  return n;
}

extern "C" int jb_decode_batch(int device_id, const char *const *paths, int n_paths, int n_threads,
                               uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses,
                               double *times) {
  if (!paths || !rgb || !widths || !heights || !statuses)
    return jb_fail_(nullptr, JB_ERR_NULL, "jb_decode_batch: NULL pointer");
  if (n_threads > n_paths && n_paths > 0) n_threads = n_paths;
  jb_batch_decoder *d = nullptr;
  int rc = jb_batch_decoder_create(device_id, n_threads, 0, 0, &d);  // buffers size themselves
  if (rc) return rc;
  rc = jb_batch_decoder_run(d, paths, n_paths, rgb, widths, heights, statuses, times);
  jb_batch_decoder_destroy(d);
  return rc;
}
