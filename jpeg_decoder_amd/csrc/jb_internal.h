// jb_internal.h -- the ONE declaration of every internal function that is defined in one .cpp and used in another
// (the names with a trailing underscore; those of the device entropy decoder's host side are in jb_huff.h, the plan
// function in jb_plan.h).  Host-only, no HIP types: tools/fuzz builds the front end against it for the CPU alone and
// stubs what needs a device.  Every defining file and every using file includes it, so a signature that changes in
// one place and not the other fails to compile or to link.  Not part of the public ABI (include/jpegblk.h).
#pragma once
#include <string>
#include <vector>

#include "../../include/jpegblk.h"
#include "jb_huff.h"
#include "jb_knobs.h"
#include "jb_plan.h"

struct jb_ctx;

// ---- jb_api.cpp: the context ---------------------------------------------------------------------------------------
// the error channel of jb_last_error: the context's text (ctx may be null) and the calling thread's
int jb_fail_(jb_ctx *ctx, int code, const char *msg);
// the environment as it was when the context was created (jb_knobs.h)
const JbKnobs *jb_ctx_knobs_(const jb_ctx *ctx);
// the frame of the last jb_decode_file / jb_decode_memory, for jb_ctx_last_desc
void jb_ctx_set_last_desc_(jb_ctx *ctx, const jb_image_desc *d);
// (jb_batch.cpp) the rank of this context's downloads among those of the other contexts on its device
void jb_ctx_set_download_age_(jb_ctx *ctx, uint64_t age);
// "decoder arithmetic": the context's setting without jb_ctx_set_arithmetic's look at the ring (jb_batch.cpp sets it
// between its own runs, when the slots' busy marks are stale and nothing is in flight)
void jb_ctx_set_arithmetic_(jb_ctx *ctx, int arith);
// "draft decode": the same for the context's draft
void jb_ctx_set_draft_(jb_ctx *ctx, int denom);
#define kJbArithScaleText "JB_ARITH_LIBJPEG cannot be combined with a scale other than 1"
// JB_OK when [p, p + bytes) is device memory of `device` (jb_batch_decoder_set_device_output: a host pointer or
// another GPU's memory would fault in the pixel kernel instead of failing here)
int jb_check_device_region_(int device, const void *p, size_t bytes);

// ---- jb_api.cpp: submissions ---------------------------------------------------------------------------------------
// device-side entropy decoding: several prepared images of ONE geometry in one submission, pixels contiguous; the
// images' status words (0 = decoded cleanly) are copied to `status_out` (pinned) with the pixels
// (plan: what the pixels look like -- jb_plan.h; tight rows, and tight planes with a planar format)
// (dst_device: `rgb` is device memory of the context's device, nothing is downloaded)
int jb_submit_packed_(jb_ctx *ctx, const jb_image_desc *desc, const uint16_t *qtabs, const uint8_t *packed, const JbHuffLayout *lay,
                      uint8_t *rgb, uint32_t *status_out, int *ticket, const JbOutPlan &plan, int dst_device);
// a group of the batch decoder: jb_submit_batch (dst_device = 0) or its device-output form (1) in the plan's output;
// tight rows
int jb_submit_group_(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const int16_t *coef, const uint16_t *qtabs, uint8_t *rgb,
                     int *ticket, const JbOutPlan &plan, int dst_device);
// jb_wait in two halves, so that many threads can wait on one shared context: under the caller's lock, the ring slot
// to block on (nullptr: the submission has completed) ...
void *jb_wait_begin_(jb_ctx *ctx, int ticket);
// ... and the blocking part, without the lock
int jb_wait_block_(jb_ctx *ctx, void *slot);
// the two routes of decode(bytes) into the pixel kernel, tight rows, `plan` (jb_plan.h) says which pixels, rgb holds
// plan.image_bytes: the entropy stage on the device (a prepared job; the staging ring follows the frame) ...
int jb_decode_job_(jb_ctx *ctx, const JbHuffJob *job, uint8_t *rgb, const JbOutPlan &plan);
// ... or on the host (its coefficients): jb_blocks_to_rgb with any output plan
int jb_blocks_to_rgb_plan_(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef, const uint16_t *qtabs, uint8_t *rgb,
                           const JbOutPlan &plan);

// ---- jb_frontend.cpp, jb_frontend_ext.cpp: the front end in steps, on the shared header (jb_markers.h) --------------
namespace jbe {
struct Header;
struct Ext;
struct Err;
}  // namespace jbe
// the baseline rules: the header and where the one scan begins (gray: one-component frames too, for the device decoder) ...
int jb_parse_baseline_(const uint8_t *jpeg, size_t n, jbe::Header &h, bool gray, jbe::Err &e);
// ... the scan of such a header (three components) into `coef` on n_threads host threads ...
int jb_decode_baseline_(const jbe::Header &h, int16_t *coef, size_t coef_cap_bytes, int n_threads, jbe::Err &e);
// ... or a device job from it (jb_huff_prepare_(bytes, ...) of jb_huff.h is the two together); *why: a refusal's text
int jb_huff_prepare_header_(const jbe::Header &h, JbHuffJob *job, uint32_t chunk_knob, const char **why);
// the general rules (progressive, grayscale, multi-scan files): the header up to the first scan, and the scans into `coef`
int jb_ext_parse_(const uint8_t *jpeg, size_t n, jbe::Ext &x, jbe::Err &e);
int jb_ext_scans_(jbe::Ext &x, int16_t *coef, size_t coef_cap_bytes, jbe::Err &e);
// both in one walk; coef == nullptr: the header only
int jb_ext_decode_(const uint8_t *jpeg, size_t n, jb_image_desc *desc, uint16_t *qtabs, int16_t *coef, size_t coef_cap_bytes,
                   std::string *err);

// ---- jb_color_host.cpp: "colour chains" -----------------------------------------------------------------------------
// What jb_color_check cannot know: the geometric operations of n CHECKED chains on views of w x h -- jb_warp_params' refusals
// that depend on the size.  JB_OK, or the status with *bad (may be null) the first such chain's index and *why the reason.
int jb_color_check_size_(const jb_color_chain *chains, int64_t n, int32_t w, int32_t h, int64_t *bad, const char **why);

// ---- jb_hostutil.cpp: host helpers without HIP ---------------------------------------------------------------------
// seconds on the steady clock
double jb_now_s_();
// the whole file into buf; false: it cannot be opened or read
bool jb_read_file_(const char *path, std::vector<uint8_t> &buf);
// The first `limit` bytes of a file (all of it when it is no longer than that); *whole says which.
bool jb_read_prefix_(const char *path, size_t limit, std::vector<uint8_t> &buf, bool *whole);
// the cgroup CPU quota of this process in whole CPUs, rounded down (cgroup v2 cpu.max, then v1 cpu.cfs_quota_us /
// cpu.cfs_period_us); 0: none.  *fraction (may be null): the quota has a part of a CPU beyond that
int jb_cpu_quota_(bool *fraction = nullptr);
// CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota
int jb_available_cpus_();
// binds the calling thread to the CPUs of the NUMA node closest to a device (numa_knob: JbKnobs::numa of the calling
// decoder); returns the CPUs in the new mask, 0 = left as it was
int jb_bind_thread_near_device_(int device, int numa_knob);
// "a spec for tight output" (no plane stride to check against a row stride yet): JB_OK or JB_ERR_GEOMETRY, which every
// entry point reports as its own name followed by JB_TIGHT_SPEC_TEXT
int jb_tight_spec_check_(const jb_output_spec *spec);
#define JB_TIGHT_SPEC_TEXT ": bad output spec (unknown format, reserved or plane_stride not 0, scale / bias not finite)"
