// jb_batch_run.cpp -- the engine of one device's run of the batch decoder: the two passes over the files, the host
// threads' work on their groups, run_single (jb_batch.h).  The decoder object and the C ABI are jb_batch.cpp's, the
// request and its rules jb_batch_request.h's.
//
// Structure: N host threads run the entropy decoder (the end-to-end bottleneck), each into its
// own pinned coefficient buffers, and submit to ONE shared jb_ctx (under a mutex) whose staging
// ring uploads + computes on one stream and downloads on another, so the link runs full duplex
// (97 GB/s instead of 57).  One context for all host threads rather than one per thread: 16 x 2
// streams on the few hardware queues of a process block each other (measured on 8192x8192 4:2:0:
// 65 images/s, against 120 for one single-stream context per thread).  There is no device
// thread: the host thread that finished an image is running by definition, so a submission never
// waits for the scheduler; a full ring blocks the submitter (back-pressure), and every thread
// waits for its own images outside the mutex.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "jb_batch.h"

namespace {

struct Parsed {
  std::vector<uint8_t> bytes;
  bool loaded = false;  // `bytes` is the whole file (pass 1 reads only the head of a large file)
  jb_image_desc desc;
  jb_geometry geo;         // (geo.rgb_bytes: the bytes of the OUTPUT image, plan.image_bytes)
  JbOutPlan plan = {};     // the output image: size, element size, bytes (jb_plan.h)
  uint16_t qtabs[256];
  int status = JB_OK;
  std::string error;
  bool have = true;  // headers parsed (false: a run without pass 1 parses a file when its group is formed)
};

// the one context all host threads submit to
struct Shared {
  std::mutex mu;
  jb_ctx *ctx = nullptr;
};

struct Totals {
  std::mutex mu;
  double t_entropy = 0, t_device = 0, t_read = 0;
  double first_submit = 1e30, last_submit = 0, first_back = 1e30, first_thread_done = 1e30;  // JPEGBLK_TIMING=3
  int first_error = JB_OK;
  std::string first_error_text;
};

struct Run {
  int device;
  size_t dev_cap_coef, dev_cap_rgb;  // ring-slot capacity: bounds a group whose entropy stage runs on the device
  int n_slots;                       // submissions a host thread keeps in flight (kLaneSlots)
  const char *const *paths;
  int n_paths, n_threads, inner_threads;
  const std::vector<std::vector<int>> *lists;  // which files each host thread owns (indices into paths)
  uint8_t **rgb;
  int32_t *widths, *heights;
  int *statuses;
  Arena *arena;
  Shared *dev;
  Totals *tot;
  const JbKnobs *knobs;  // the decoder's (jb_knobs.h)
  // no pass 1: every file is read and parsed when its group is formed; an image the decoder's buffers do not hold
  // is left for a second, classic round (deferred[t]: positions in thread t's list)
  bool lazy = false;
  std::vector<std::vector<int>> *deferred = nullptr;
  size_t slot_coef = 0, slot_rgb = 0;  // what a ring slot holds (one image may be larger than a group's bound, not than this)
  OutputRequest out;  // the decoder's
  PerFile per;  // "per-image rectangles" (jb_batch_decoder_run_crops) and "views" (_run_views): what belongs to paths[i]
};

// pass 1 (per host thread): parse the headers of its files, so that the buffers can be sized once for
// the whole batch.  Only the head of a file is read here (kHeadBytes: the tables and the frame header
// of an ordinary file come long before that); the rest is read in pass 2, group by group, while the
// device works on the groups before -- reading a batch of 1,024 one-megabyte files whole took 30 ms
// of a 200 ms batch during which the device had nothing to do, and held every file in memory at once.
// A head that does not parse cleanly (headers longer than the head, progressive and multi-scan files,
// errors) is settled on the whole file, so every status is the one the whole file gives.
// (Two head sizes: the headers of a plain baseline file end within a few hundred bytes, so 4 KB are read first --
// 3 us instead of 5 per file on one thread; files with large APPn segments -- EXIF, ICC profiles -- get the 64 KB,
// then the whole file.  What pass 1 costs in a batch is opening and closing the files, not reading them: 1,024 files
// on 16 threads take 3.6-4.0 ms with either head size when the batch repeats eight files, as the benches do, every
// thread opening the same inodes -- 59 us per file against 12 us for one thread alone.)
constexpr size_t kHeadBytes[2] = {(size_t)4 << 10, (size_t)64 << 10};

// every size of the pixels that this file takes downstream -- staging, arena, ring slots, copies -- is the output's:
// geo.rgb_bytes is set to the bytes of the plan's image: the reduced one at scale > 1, the format's with a planar format
// (i: file i of the run -- its rectangle or its views are planned as those of a batch of one, PerFile::plan; the arrays
// are the run's and outlive the plan)
void parse_one(Parsed &p, const OutputRequest &out, const PerFile &per, int i) {
  p.status = jb_entropy_decode(p.bytes.data(), p.bytes.size(), &p.desc, p.qtabs, nullptr, 0);
  if (p.status == JB_OK) p.status = jb_geometry_of(&p.desc, &p.geo);
  if (p.status != JB_OK) {
    p.error = jb_last_error(nullptr);
    return;
  }
  // "orientation": the decoder's, or this file's own tag (the Exif segment lies in front of the frame header that
  // has just been parsed, so a head that parses holds it)
  int orient = out.orient;
  if (orient == JB_ORIENT_EXIF && jb_exif_orientation(p.bytes.data(), p.bytes.size(), &orient) != JB_OK) orient = JB_ORIENT_STORED;
  const jb_image_desc frame = jb_draft_desc_(&p.desc, out.draft);  // ("draft decode": every size downstream is the draft frame's)
  p.plan = per.plan(out, frame, orient, 1, per.views_of(i), per.roi_of(i));
  p.status = p.plan.status;
  if (p.status == JB_OK) p.geo.rgb_bytes = p.plan.image_bytes;
  else p.error = p.plan.why;
}

void parse_pass(const Run &r, int t, std::vector<Parsed> &parsed, size_t *max_coef, size_t *max_rgb, double *t_read) {
  jb_bind_thread_near_device_(r.device, r.knobs->numa);  // the file bytes are first touched here: keep them on the GPU's node
  for (size_t k = 0; k < parsed.size(); k++) {
    const int i = (*r.lists)[(size_t)t][k];
    Parsed &p = parsed[k];
    bool ok = true;
    p.status = JB_ERR_FORMAT;
    p.loaded = false;
    for (int level = 0; level < 3 && ok && p.status != JB_OK && !p.loaded; level++) {  // heads, then the whole file decides
      const double a = jb_now_s_();
      ok = level < 2 ? jb_read_prefix_(r.paths[i], kHeadBytes[level], p.bytes, &p.loaded) : jb_read_file_(r.paths[i], p.bytes);
      *t_read += jb_now_s_() - a;
      if (level == 2) p.loaded = ok;
      if (ok) parse_one(p, r.out, r.per, i);
    }
    if (!ok) {
      p.status = JB_ERR_FORMAT;
      p.error = "cannot read file";
      p.bytes.clear();
      continue;
    }
    if (p.status != JB_OK) continue;
    if (!p.loaded) {
      p.bytes.clear();
      p.bytes.shrink_to_fit();
    }
    if ((size_t)p.geo.coef_bytes > *max_coef) *max_coef = (size_t)p.geo.coef_bytes;
    if ((size_t)p.geo.rgb_bytes > *max_rgb) *max_rgb = (size_t)p.geo.rgb_bytes;
  }
}

bool same_geometry(const Parsed &a, const Parsed &b) {
  return a.desc.width == b.desc.width && a.desc.height == b.desc.height && a.desc.hs == b.desc.hs &&
         a.desc.vs == b.desc.vs && a.desc.qtab_id[0] == b.desc.qtab_id[0] &&
         a.desc.qtab_id[1] == b.desc.qtab_id[1] && a.desc.qtab_id[2] == b.desc.qtab_id[2] &&
         a.plan.orient == b.plan.orient;  // (a group is one launch, a launch one orientation)
}

// a group in flight in one of the thread's slots
struct Group {
  int ticket = -1, first = -1, n = 0;  // images first .. first+n-1 of this thread's list
  bool on_device = false;              // the group's entropy stage ran on the device (jb_huff.hip)
};

// how many images of the head's geometry a group may hold: decoded on the host, on the device, and on the device
// without the ramp of the first groups (what the pinned blob is sized for)
struct Rooms {
  int host, dev, dev_full;
};

// the group being formed, from step to step: images k .. k+n-1 of the thread's list, for slot s
struct Forming {
  int k, s;
  int n = 0;
  bool on_device = false;
  std::vector<std::unique_ptr<JbHuffJob>> jobs;  // on_device: the prepared images
  uint8_t *dst = nullptr;                        // where the group's pixels go
  int st = JB_OK;                                // what place / pack / submit made of it
  std::string text;
  JbHuffLayout lay;
};

// pass 2 (per host thread): decode a group of images into pinned slot g%2 and submit it; before a
// slot is reused, the group that used it two steps ago is finished (it has long been through the
// device by then: entropy decoding takes ~10x the transfers)
struct LaneWorker {
  const Run &r;
  Lane *lane;
  int t;
  std::vector<Parsed> &parsed;
  int setup_rc;
  const std::string &setup_text;
  const bool use_arena = r.arena && r.arena->base;
  const bool to_device = use_arena && r.arena->on_device;
  // Where the entropy stage runs.  The batch decoder's default is the DEVICE for every baseline image
  // the device decoders take (restart intervals: one lane per interval; none: the self-synchronising
  // decoder), 16 intervals / chunks or more: measured against 16 host threads it is 1.06x (8,192 small
  // images) to 2.6x (4096x4096 files) as fast end to end for a tenth of the host CPU time (DESIGN.md
  // section 9); this thread then only parses, removes the byte stuffing and packs.  What the device
  // decoders refuse or flag goes through the host decoder, image by image.  JPEGBLK_GPU_HUFFMAN=0
  // keeps the entropy stage on the host threads (north_star's split), =2 drops the 16-interval
  // threshold.  A group is all-device or all-host.
  // (A hybrid -- a quarter of the threads feeding the device decoder with 60 % of the files, the rest
  // decoding on the host -- was measured and is slower than either pure mode: 1,885 images/s against
  // 2,681 host / 2,498 device on PIL 1080p files; large group downloads and many small uploads and
  // downloads at once share the link badly.  Removed.)
  const bool dev_entropy = r.knobs->gpu_huffman != 0;
  const uint32_t min_intervals = r.knobs->gpu_huffman == 2 ? 1u : 16u;
  const int dev_max_group = kMaxGroup;  // images per device-entropy group
  double t_entropy = 0, t_wait = 0, t_read = 0;
  double first_submit = 1e30, last_submit = 0, first_back = 1e30;  // (JPEGBLK_TIMING=3)
  Group grp[kMaxSlots];
  int slot = 0;
  int dev_groups = 0;  // device-entropy groups this thread has submitted
  std::vector<uint16_t> qtabs;

  // the rest of a file whose head was parsed in pass 1
  void load(Parsed &p, int i) {
    if (p.loaded || p.status != JB_OK) return;
    const double a = jb_now_s_();
    if (jb_read_file_(r.paths[i], p.bytes)) {
      p.loaded = true;
    } else {
      p.status = JB_ERR_FORMAT;
      p.error = "cannot read file";
      p.bytes.clear();
    }
    t_read += jb_now_s_() - a;
  }

  // (a run without pass 1) headers of file k of this thread's list, from the whole file; -> false: the image does
  // not fit the buffers this decoder has (it waits for the second round)
  bool ready(int k) {
    Parsed &p = parsed[(size_t)k];
    if (!p.have) {
      const int i = (*r.lists)[(size_t)t][(size_t)k];
      const double a = jb_now_s_();
      const bool ok = jb_read_file_(r.paths[i], p.bytes);
      t_read += jb_now_s_() - a;
      p.have = true;
      p.loaded = ok;
      if (ok) {
        parse_one(p, r.out, r.per, i);
      } else {
        p.status = JB_ERR_FORMAT;
        p.error = "cannot read file";
        p.bytes.clear();
      }
    }
    if (!r.lazy || p.status != JB_OK) return true;
    const size_t c = (size_t)p.geo.coef_bytes, x = (size_t)p.geo.rgb_bytes;
    return c <= lane->cap_coef && x <= lane->cap_rgb && c <= r.slot_coef && x <= r.slot_rgb;
  }

  int index_of(int k) const { return (*r.lists)[(size_t)t][(size_t)k]; }

  void report(int i, int st, const std::string &text) {
    r.statuses[i] = st;
    if (st == JB_OK) return;
    if (!use_arena) jb_free(r.rgb[i]);
    r.rgb[i] = nullptr;
    std::lock_guard<std::mutex> g(r.tot->mu);
    if (r.tot->first_error == JB_OK) {
      r.tot->first_error = st;
      r.tot->first_error_text = std::string(r.paths[i]) + ": " + text;
    }
  }

  // the device decoder met data it calls corrupt: the host decoder is the authority -- image j of the group in slot
  // s again, entropy stage on the host (the slot's coefficient buffer is free: the group is done)
  int redo_on_host(int s, int j, uint8_t *staged, std::string &text_j) {
    Parsed &p = parsed[(size_t)(grp[s].first + j)];
    int16_t *const cbuf = lane->coef_at(s);
    int st_j = cbuf ? jb_entropy_decode(p.bytes.data(), p.bytes.size(), &p.desc, p.qtabs, cbuf, lane->cap_coef) : (int)JB_ERR_HIP;
    if (st_j == JB_OK) {
      int ticket = -1;
      void *ev2 = nullptr;
      {
        std::lock_guard<std::mutex> lk(r.dev->mu);
        st_j = jb_submit_group_(r.dev->ctx, &p.desc, 1, cbuf, p.qtabs, staged, &ticket, p.plan, to_device);
        if (st_j == JB_OK) ev2 = jb_wait_begin_(r.dev->ctx, ticket);
        else text_j = jb_last_error(r.dev->ctx);
      }
      if (st_j == JB_OK && ev2) st_j = jb_wait_block_(r.dev->ctx, ev2);
    } else {
      text_j = jb_last_error(nullptr);
    }
    return st_j;
  }

  // the group in slot s has come back: its images are reported, the slot is free
  void finish_slot(int s) {
    Group &g = grp[s];
    if (g.n == 0) return;
    double a = jb_now_s_();
    void *ev;
    {
      std::lock_guard<std::mutex> lk(r.dev->mu);
      ev = jb_wait_begin_(r.dev->ctx, g.ticket);
    }
    const int st = ev ? jb_wait_block_(r.dev->ctx, ev) : JB_OK;
    const std::string text = st == JB_OK ? "" : jb_last_error(nullptr);
    const size_t rgb_bytes = (size_t)parsed[(size_t)g.first].geo.rgb_bytes;
    for (int j = 0; j < g.n; j++) {
      const int i = index_of(g.first + j);
      Parsed &p = parsed[(size_t)(g.first + j)];
      int st_j = st;
      std::string text_j = text;
      uint8_t *const staged = use_arena ? r.rgb[i] : lane->out[s] + (size_t)j * rgb_bytes;
      if (st == JB_OK && g.on_device && lane->status[s][j] != 0) st_j = redo_on_host(s, j, staged, text_j);
      if (g.on_device) {
        p.bytes.clear();
        p.bytes.shrink_to_fit();
      }
      if (st_j == JB_OK && !use_arena)  // pinned staging -> the caller's (pageable) buffer
        memcpy(r.rgb[i], staged, rgb_bytes);
      report(i, st_j, text_j);
    }
    t_wait += jb_now_s_() - a;
    if (first_back > 1e29) first_back = jb_now_s_();
    g.n = 0;
  }

  Rooms group_room(const Parsed &head) const {
    const size_t coef_bytes = (size_t)head.geo.coef_bytes, rgb_bytes = (size_t)head.geo.rgb_bytes;
    // a group must fit the coefficient AND the pixel capacity (pinned lane buffers and ring slots are
    // sized from the batch's largest image: rgb/coef is 0.5 for 4:4:4 and 1.0 for 4:2:0, so many
    // small 4:2:0 images next to one large 4:4:4 image are bounded by the pixel side)
    size_t room_c = lane->cap_coef / coef_bytes, room_p = lane->cap_rgb / rgb_bytes;
    int room = (int)(room_c < room_p ? room_c : room_p);
    if (room > kMaxGroup) room = kMaxGroup;
    if (room < 1) room = 1;  // (cannot happen: the capacities cover the largest single image)
    // a group decoded on the device does not pass through this thread's pinned coefficient buffer:
    // it is bounded by the ring slot (and, without an arena, by the pinned pixel staging)
    size_t droom_c = r.dev_cap_coef / coef_bytes, droom_p = (use_arena ? r.dev_cap_rgb : lane->cap_rgb) / rgb_bytes;
    int room_dev = (int)(droom_c < droom_p ? droom_c : droom_p);
    if (room_dev > dev_max_group) room_dev = dev_max_group;
    const int room_dev_full = room_dev < 1 ? 1 : room_dev;
    // (JPEGBLK_GROUP_RAMP=1: the thread's first two device groups a quarter and a half of the full size, so that the
    // device gets its first work sooner.  It paid while every run began with a pass over all headers; since files
    // are parsed as their groups are formed the first submission leaves after 1 ms anyway, and fewer, larger groups
    // win: 1,024 1080p files left in HBM 33-35 k -> 41.6-42.1 k images/s, 128 files 21 k -> 26 k, 128 files to the
    // arena 6,700 -> 7,240, interleaved on one box.  Off by default.)
    if (dev_groups < 2 && r.knobs->group_ramp) room_dev = room_dev >> (2 - dev_groups);
    if (room_dev < 1) room_dev = 1;
    return Rooms{room, room_dev, room_dev_full};
  }

  // entropy-decode consecutive images of the head's geometry into the slot, back to back -- or,
  // for files with restart intervals, only ready them for the device decoder.  f.n == 0: the head's scan is corrupt
  // (reported here; nothing else ends a group before its first image)
  void form_group(Forming &f, const Rooms &rooms) {
    const int k = f.k, s = f.s, n_mine = (int)parsed.size();
    Parsed &head = parsed[(size_t)k];
    const size_t coef_bytes = (size_t)head.geo.coef_bytes;
    int &n = f.n;
    bool &on_device = f.on_device;
    while (n < (on_device ? rooms.dev : rooms.host) && k + n < n_mine) {
      Parsed &p = parsed[(size_t)(k + n)];
      if (n > 0 && !ready(k + n)) break;  // (the next group's head: it is set aside there)
      if (n > 0 && (p.status != JB_OK || !same_geometry(head, p))) break;
      load(p, index_of(k + n));
      if (p.status != JB_OK) break;  // (n > 0: the head was loaded above; the next group reports it)
      double a = jb_now_s_();
      std::unique_ptr<JbHuffJob> job;
      bool eligible = false;
      if (dev_entropy) {
        job.reset(new JbHuffJob());
        eligible = jb_huff_prepare_(p.bytes.data(), p.bytes.size(), job.get(), nullptr, r.knobs->chunk_bytes) == JB_OK && jb_huff_worth_it_(*job, min_intervals);
        // the frame this pass reads must be the frame pass 1 sized the group for (a file that changed in between):
        // else the host path below settles the image, with its own capacity checks
        if (eligible && (job->desc.width != p.desc.width || job->desc.height != p.desc.height || job->desc.hs != p.desc.hs ||
                         job->desc.vs != p.desc.vs || memcmp(job->desc.qtab_id, p.desc.qtab_id, sizeof p.desc.qtab_id) != 0))
          eligible = false;
      }
      if (n == 0) on_device = eligible;
      else if (eligible != on_device) break;  // the next group starts with this image
      if (on_device) {
        memcpy(p.qtabs, job->qtabs, sizeof p.qtabs);
        f.jobs.push_back(std::move(job));
        t_entropy += jb_now_s_() - a;
        n++;  // (the file bytes stay until the group has come back clean)
        continue;
      }
      // fewer files than host threads: the spare threads split each image's restart intervals
      int16_t *const cbuf = lane->coef_at(s);
      int st = cbuf ? jb_entropy_decode_mt(p.bytes.data(), p.bytes.size(), &p.desc, p.qtabs,
                                           cbuf + (size_t)n * (coef_bytes / 2), coef_bytes, r.inner_threads)
                    : (int)JB_ERR_HIP;
      t_entropy += jb_now_s_() - a;
      p.bytes.clear();
      p.bytes.shrink_to_fit();
      if (st != JB_OK) {  // a corrupt scan: it leaves the group, the group ends before it
        p.status = st;
        p.error = jb_last_error(nullptr);
        if (n == 0) {
          r.rgb[index_of(k)] = nullptr;
          report(index_of(k), st, p.error);
        }
        break;
      }
      n++;
    }
  }

  // where the pixels go
  void place_outputs(Forming &f) {
    const int k = f.k, n = f.n;
    const Parsed &head = parsed[(size_t)k];
    const size_t rgb_bytes = (size_t)head.geo.rgb_bytes;
    f.dst = use_arena ? r.arena->take((size_t)n * rgb_bytes) : lane->out[f.s];
    if (!f.dst) {
      f.st = JB_ERR_CAPACITY;
      f.text = "output arena exhausted";
    } else if ((uintptr_t)f.dst & (uintptr_t)(head.plan.esize - 1)) {
      // (groups start on 256-byte steps of the arena / region and an image is a whole number of elements, so every image
      // is element-aligned unless the region itself is not: checked, not assumed -- the kernel's f32 / f16 stores need it)
      f.st = JB_ERR_GEOMETRY;
      f.text = "output region is not aligned to the format's element size";
    }
    qtabs.resize((size_t)n * 256);
    for (int j = 0; j < n; j++) {
      const int i = index_of(k + j);
      Parsed &p = parsed[(size_t)(k + j)];
      memcpy(&qtabs[(size_t)j * 256], p.qtabs, sizeof p.qtabs);
      r.widths[i] = p.plan.out_w;
      r.heights[i] = p.plan.out_h;
      r.rgb[i] = nullptr;
      if (f.st == JB_OK) {
        r.rgb[i] = use_arena ? f.dst + (size_t)j * rgb_bytes : jb_alloc_pixels_(rgb_bytes);
        if (!r.rgb[i]) {
          f.st = JB_ERR_CAPACITY;
          f.text = "out of memory";
        }
      }
    }
  }

  // pack the group into this thread's pinned blob -- outside the shared lock
  void pack_group(Forming &f, int room_dev_full) {
    if (f.st != JB_OK || !f.on_device) return;
    const int n = f.n;
    std::vector<const JbHuffJob *> ptrs;
    for (auto &j : f.jobs) ptrs.push_back(j.get());
    const size_t blob_bytes = jb_huff_pack_size_(ptrs.data(), n);
    uint8_t *blob = lane->ensure_blob(r.device, f.s, blob_bytes, blob_bytes / (size_t)n * (size_t)room_dev_full);
    if (!blob) {
      f.st = JB_ERR_HIP;
      f.text = "pinned host allocation failed";
    } else if ((f.st = jb_huff_pack_(ptrs.data(), n, (int64_t)parsed[(size_t)f.k].geo.coef_bytes, blob, &f.lay)) != JB_OK) {
      f.text = "submission too large for the device entropy decoder";
    }
    f.jobs.clear();  // (everything the jobs held is in the blob now)
  }

  void submit_group(Forming &f) {
    if (f.st != JB_OK) return;
    const int s = f.s;
    Parsed &head = parsed[(size_t)f.k];
    // per-image rectangles: the group's members have one geometry and one target, and each its own rectangle -- the
    // head's plan with the members' rectangles next to it (the array is read before the submission returns)
    JbOutPlan plan = head.plan;
    std::vector<jb_roi> crops;
    std::vector<jb_view> views;  // "views": the members' views, k each, in the group's order
    std::vector<jb_color_chain> colors;  // "colour chains": and their chains, parallel to them
    const jb_image_desc frame = jb_draft_desc_(&head.desc, r.out.draft);
    for (int j = 0; j < f.n && r.per.views; j++) {
      views.insert(views.end(), parsed[(size_t)(f.k + j)].plan.views, parsed[(size_t)(f.k + j)].plan.views + r.per.k);
      if (r.per.colors) colors.insert(colors.end(), r.per.colors_of(index_of(f.k + j)), r.per.colors_of(index_of(f.k + j)) + r.per.k);
    }
    for (int j = 0; j < f.n && r.per.rois; j++) crops.push_back(parsed[(size_t)(f.k + j)].plan.roi);
    if (r.per.views || r.per.rois) {
      plan = r.per.plan(r.out, frame, head.plan.orient, f.n, r.per.views ? views.data() : nullptr, nullptr, r.per.rois ? crops.data() : nullptr);
      if (r.per.colors) plan.colors = colors.data();
    }
    double a = jb_now_s_();
    // every copy of the submission is pinned <-> device, so this returns at once and the
    // transfers and the kernel run while this thread decodes its next group
    std::lock_guard<std::mutex> lk(r.dev->mu);
    if (f.on_device) {
      f.st = jb_submit_packed_(r.dev->ctx, &head.desc, qtabs.data(), lane->blob[s], &f.lay, f.dst, lane->status[s], &grp[s].ticket, plan,
                               to_device);
    } else {
      f.st = jb_submit_group_(r.dev->ctx, &head.desc, f.n, lane->coef[s], qtabs.data(), f.dst, &grp[s].ticket, plan, to_device);
    }
    if (f.st != JB_OK) f.text = jb_last_error(r.dev->ctx);
    t_wait += jb_now_s_() - a;
    last_submit = jb_now_s_();
    if (first_submit > 1e29) first_submit = last_submit;
  }

  void run() {
    jb_bind_thread_near_device_(r.device, r.knobs->numa);
    const int kSlots = r.n_slots;
    const int n_mine = (int)parsed.size();
    int k = 0;
    while (k < n_mine) {
      Parsed &head = parsed[(size_t)k];
      if (!ready(k)) {  // (a run without pass 1) larger than anything this decoder is sized for: the second round's
        (*r.deferred)[(size_t)t].push_back(k);
        head.bytes.clear();
        head.bytes.shrink_to_fit();
        k++;
        continue;
      }
      load(head, index_of(k));
      r.rgb[index_of(k)] = nullptr;
      r.widths[index_of(k)] = r.heights[index_of(k)] = 0;
      if (head.status != JB_OK || setup_rc != JB_OK) {  // rejected in pass 1, or nothing could be set up
        report(index_of(k), head.status != JB_OK ? head.status : setup_rc, head.status != JB_OK ? head.error : setup_text);
        head.bytes.clear();
        head.bytes.shrink_to_fit();
        k++;
        continue;
      }
      const int s = slot;
      finish_slot(s);
      const Rooms rooms = group_room(head);
      Forming f{k, s};
      form_group(f, rooms);
      if (f.n == 0) {  // (the head left the list)
        k++;
        continue;
      }
      place_outputs(f);
      pack_group(f, rooms.dev_full);
      submit_group(f);
      if (f.st != JB_OK) {
        for (int j = 0; j < f.n; j++) report(index_of(k + j), f.st, f.text);
      } else {
        grp[s].first = k;
        grp[s].n = f.n;
        grp[s].on_device = f.on_device;
        if (f.on_device) dev_groups++;
        slot = (slot + 1) % kSlots;
      }
      k += f.n;
    }
    for (int j = 0; j < kSlots; j++) finish_slot((slot + j) % kSlots);  // oldest first
    std::lock_guard<std::mutex> g(r.tot->mu);
    r.tot->t_entropy += t_entropy;
    r.tot->t_device += t_wait;
    r.tot->t_read += t_read;
    if (first_submit < r.tot->first_submit) r.tot->first_submit = first_submit;
    if (last_submit > r.tot->last_submit) r.tot->last_submit = last_submit;
    if (first_back < r.tot->first_back) r.tot->first_back = first_back;
    const double done = jb_now_s_();
    if (done < r.tot->first_thread_done) r.tot->first_thread_done = done;
  }
};

}  // namespace

// one device's share of a run; `top` = this decoder owns the arena (and recycles it)
int run_single(jb_batch_decoder *d, const char *const *paths, int n_paths, const PerFile &per, uint8_t **rgb, int32_t *widths,
               int32_t *heights, int *statuses, double *times, bool top) {
  Totals tot;
  Shared dev;
  if (top) d->arena->used = 0;  // the previous run's images are released
  const double t0 = jb_now_s_();
  // every pinned buffer and ring slot holds one large image or a group of small ones: the group
  // figure bounds the coefficient and the pixel side alike (rgb_bytes <= coef_bytes in every layout)
  size_t group_bytes = kGroupBytes;
  if (d->knobs.group_mb >= 0) group_bytes = (size_t)d->knobs.group_mb << 20;  // (JPEGBLK_GROUP_MB; 0 = one image per submission)
  // Groups whose entropy stage runs on the device hold about 100 MB of coefficients (JPEGBLK_DEV_GROUP_MB;
  // 8 1080p images, one 8192x8192 image, at most 64 images).  (With the first versions of the device decoder,
  // whose launches took milliseconds whatever their size, large groups paid -- 2,626 images/s in groups of
  // 20, 3,947 in groups of 64 -- and the default was a thread's whole share up to 512 MB.  With today's
  // kernels many small groups in flight are as fast or faster with host output (medians of six runs:
  // 0.171 s against 0.18 s for 1,024 1080p files; 8192x8192 +5 %) and much faster with device-resident
  // output, and the ring slots are a fifth of the size: profiles/r02b/ab_group_size_final.txt.)
  size_t dev_group_bytes = 0;
  if (d->knobs.gpu_huffman != 0) {
    const long mb = d->knobs.dev_group_mb >= 0 ? d->knobs.dev_group_mb : 96;
    dev_group_bytes = mb > 0 ? (size_t)mb << 20 : 0;
  }
  // One round over `files` (indices into paths).  Classic: pass 1 reads every file's headers so that the buffers
  // can be sized once for the round, then pass 2 decodes.  Lazy (a decoder whose buffers exist already: created
  // with sizes, or after an earlier run): no pass 1 -- a file is read once and parsed when its group is formed, so
  // the device has its first work after two files' worth of host time instead of after every header of the batch
  // (1,024 files: 5 ms -> 1 ms to the first submission) -- and an image larger than the buffers is handed back in
  // `left_over` for a classic round.
  auto round = [&](const std::vector<int> &files, bool lazy, std::vector<int> *left_over) {
    int nt = (int)d->lanes.size();
    if (nt > (int)files.size()) nt = (int)files.size();
    if (nt < 1) return;
    std::vector<std::vector<int>> lists((size_t)nt);
    for (size_t j = 0; j < files.size(); j++) lists[j % (size_t)nt].push_back(files[j]);  // file j -> thread j % nt
    std::vector<std::vector<int>> deferred((size_t)nt);
    Run r{d->device, 0, 0, d->slots(), paths, n_paths, nt, (int)d->lanes.size() / nt,
          &lists, rgb, widths, heights, statuses, d->arena, &dev, &tot, &d->knobs};
    r.lazy = lazy;
    r.deferred = &deferred;
    r.out = d->out;
    r.per = per;
    const double tr0 = jb_now_s_();
    std::vector<std::vector<Parsed>> parsed((size_t)nt);
    for (int t = 0; t < nt; t++) parsed[(size_t)t].resize(lists[(size_t)t].size());
    int setup_rc = JB_OK;
    std::string setup_text;
    size_t ring_bytes = dev_group_bytes;
    double t_parsed = tr0;
    if (!lazy) {
      // pass 1: headers, in parallel
      std::vector<size_t> mc((size_t)nt, 0), mr((size_t)nt, 0);
      std::vector<double> tr((size_t)nt, 0.0);
      {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
          th.emplace_back([&, t] { parse_pass(r, t, parsed[(size_t)t], &mc[(size_t)t], &mr[(size_t)t], &tr[(size_t)t]); });
        for (auto &x : th) x.join();
      }
      size_t max_coef = 0, max_rgb = 0;
      for (int t = 0; t < nt; t++) {
        if (mc[(size_t)t] > max_coef) max_coef = mc[(size_t)t];
        if (mr[(size_t)t] > max_rgb) max_rgb = mr[(size_t)t];
        tot.t_read += tr[(size_t)t];
      }
      if (max_coef && max_coef < group_bytes) max_coef = group_bytes;
      if (max_rgb && max_rgb < group_bytes) max_rgb = group_bytes;
      if (ring_bytes) {
        size_t share = (files.size() + (size_t)nt - 1) / (size_t)nt;
        if (share > (size_t)kMaxGroup) share = (size_t)kMaxGroup;
        if (ring_bytes > share * max_coef) ring_bytes = share * max_coef;
      }
      t_parsed = jb_now_s_();
      setup_rc = max_coef ? d->ensure_all(max_coef, max_rgb, nt, ring_bytes, ring_bytes) : JB_OK;
      // a device group is bounded by this round's group size (the ring slots may be larger: an earlier run's)
      const size_t group_cap = ring_bytes > max_coef ? ring_bytes : max_coef;
      r.dev_cap_coef = (ring_bytes && group_cap < d->ctx_coef) ? group_cap : d->ctx_coef;
      r.dev_cap_rgb = (ring_bytes && group_cap < d->ctx_rgb) ? group_cap : d->ctx_rgb;
    } else {
      for (auto &list : parsed)
        for (Parsed &p : list) p.have = false;
      // the buffers as they are (this call only re-makes what a change of output mode or ring depth asks for)
      size_t lc = 0, lr = 0;
      for (const Lane &l : d->lanes) {
        if (l.cap_coef > lc) lc = l.cap_coef;
        if (l.cap_rgb > lr) lr = l.cap_rgb;
      }
      setup_rc = d->ensure_all(lc, lr, nt, d->ctx_coef, d->ctx_rgb);
      r.dev_cap_coef = (ring_bytes && ring_bytes < d->ctx_coef) ? ring_bytes : d->ctx_coef;
      r.dev_cap_rgb = (ring_bytes && ring_bytes < d->ctx_rgb) ? ring_bytes : d->ctx_rgb;
    }
    r.slot_coef = d->ctx_coef;
    r.slot_rgb = d->ctx_rgb;
    const double t_setup = jb_now_s_();
    if (setup_rc != JB_OK) setup_text = jb_last_error(nullptr);
    // pass 2: entropy decoding on the host threads, all submitting to the shared context
    dev.ctx = d->ctx;
    jb_ctx_set_arithmetic_(d->ctx, d->out.arith);  // (nothing of this decoder is in flight here)
    jb_ctx_set_draft_(d->ctx, d->out.draft);
    {
      // of two batches in flight on one device (submit / collect, or two decoders) the older one's downloads go first
      static std::atomic<uint64_t> run_seq{0};
      jb_ctx_set_download_age_(d->ctx, ++run_seq);
    }
    tot.first_submit = tot.first_back = tot.first_thread_done = 1e30;
    tot.last_submit = 0;
    {
      std::vector<std::thread> th;
      for (int t = 0; t < nt; t++)
        th.emplace_back([&, t] { LaneWorker{r, &d->lanes[(size_t)t], t, parsed[(size_t)t], setup_rc, setup_text}.run(); });
      for (auto &x : th) x.join();
    }
    if (left_over)
      for (int t = 0; t < nt; t++)
        for (int k : deferred[(size_t)t]) left_over->push_back(lists[(size_t)t][(size_t)k]);
    if (d->knobs.timing == 3)
      fprintf(stderr, "run_single %zu files%s: headers %.2f ms, setup %.2f, first submit at %.2f, first group back at %.2f, last submit at %.2f, "
              "first thread done at %.2f, all done at %.2f\n", files.size(), lazy ? " (no pass 1)" : "", (t_parsed - tr0) * 1e3, (t_setup - t_parsed) * 1e3,
              (tot.first_submit - tr0) * 1e3, (tot.first_back - tr0) * 1e3, (tot.last_submit - tr0) * 1e3, (tot.first_thread_done - tr0) * 1e3,
              (jb_now_s_() - tr0) * 1e3);
  };
  std::vector<int> all((size_t)(n_paths > 0 ? n_paths : 0));
  for (int i = 0; i < n_paths; i++) all[(size_t)i] = i;
  // without pass 1 when every buffer exists: the ring, and the staging of every lane this run uses
  bool lazy = !d->knobs.pass1 && d->ctx && d->ctx_coef > 0 && d->ctx_rgb > 0;
  for (size_t t = 0; lazy && t < d->lanes.size() && t < all.size(); t++) lazy = d->lanes[t].cap_coef > 0 && d->lanes[t].cap_rgb > 0;
  if (lazy) {
    std::vector<int> left;
    round(all, true, &left);
    if (!left.empty()) {
      std::sort(left.begin(), left.end());
      round(left, false, nullptr);
    }
  } else {
    round(all, false, nullptr);
  }
  if (d->ctx) jb_ctx_synchronize(d->ctx);
  if (times) {
    times[0] = jb_now_s_() - t0;
    times[1] = tot.t_entropy;
    times[2] = tot.t_device;
    times[3] = tot.t_read;
  }
  if (tot.first_error != JB_OK) return jb_fail_(nullptr, tot.first_error, tot.first_error_text.c_str());
  return JB_OK;
}
