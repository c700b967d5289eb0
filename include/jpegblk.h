/* jpegblk.h -- C ABI of the MI355X-native JPEG block pipeline
 *             (dequantize -> 8x8 inverse DCT -> YCbCr->RGB).
 *
 * This library replaces ONE seam of the reference decoder (aswanthabam/JPEG_Decoder): the
 * three consecutive calls
 *
 *     this->mcus = decodeHuffman();
 *     dequantize();  inverseDCT();  YCbCrToRGB();        reference jpeg.cpp:785-788
 *
 * inside Image::process_image_data (jpeg.cpp:755-789).  Everything before the seam (marker
 * parsing, Huffman decoding) runs on the host; everything behind this ABI runs as
 * hand-written HIP kernels on gfx950.  There is no CPU fallback in this library: if no HIP
 * device is usable every compute entry point returns JB_ERR_HIP.
 *
 * DATA CONTRACT (what the seam carries)
 *   coefficients  int16, natural (de-zigzagged) order, 64 per 8x8 block (128 B), blocks in
 *                 decode order = the order decodeHuffman() visits them (jpeg.cpp:415-443):
 *                 MCUs in raster order; per MCU hs*vs luma blocks (v-major, h-minor), then
 *                 one Cb block, then one Cr block.  The reference stores them as
 *                 MCU::y/cb/cr int[64] (include/types.hpp:32-67).
 *   quant tables  up to 4 tables x 64 entries, natural order, uint16.  (The reference keeps
 *                 one byte per entry -- jpeg.cpp:216,223, types.hpp:86-92 -- so parity with it
 *                 is defined for entries <= 255.)
 *   geometry      jb_image_desc; derived sizes as read_sof computes them (jpeg.cpp:77-80,
 *                 118-127) are returned by jb_geometry().
 *   pixels        uint8 R,G,B interleaved, row stride given in bytes, cropped to
 *                 width x height: rgb[y*stride + 3*x + c] =
 *                 mcus[(y/8)*mcuWidthReal + x/8].{r,g,b}[(y%8)*8 + x%8], the linearisation
 *                 both reference sinks use (include/display.hpp:19-34, jpeg.cpp:488-499).
 *
 * ARITHMETIC CONTRACT: bit-exact with the reference CPU path (int32 dequantize, the float AAN
 * butterfly network of jpeg.cpp:594-732 with truncation toward zero after each 1-D pass, the
 * float colour transform of jpeg.cpp:521-535 with truncation then clamp) for every int16
 * coefficient and every table entry <= 255.
 *
 * OWNERSHIP: all buffers are caller-owned; the library never frees or retains caller pointers
 * past the call (async: past jb_wait).  ERRORS: every function returns a jb_status, never
 * calls exit() (the reference logs and exit(1)s, e.g. jpeg.cpp:71-72,85-86).
 * THREADING: a jb_ctx is bound to one device and its own HIP streams; calls on one ctx must be
 * serialised by the caller, different contexts may be used concurrently from different threads.
 *
 * ENVIRONMENT.  None of these is needed for normal use: they select a path for tests and A/B
 * measurements, or adapt the host side to its machine.  Each is read ONCE PER OBJECT -- when a
 * context (jb_ctx_create) or a batch decoder (jb_batch_decoder_create*, jb_decode_batch) is created
 * -- and kept there (csrc/jb_knobs.h is the one place that reads them):
 *   JPEGBLK_GPU_HUFFMAN    where the entropy stage runs: unset = batch decoders on the device for files
 *                          of 16 chunks (2 KB of scan) or more, single images from 128 KB of scan on;
 *                          0 = always the host threads (north_star's split); 1 = the device for every
 *                          file of 16 chunks or more; 2 = the device for every file it takes
 *   JPEGBLK_CHUNK_BYTES    64 | 128: scan bytes per lane of the device entropy decoder (default 128)
 *   JPEGBLK_BYTE_STORE     1 = every pixel through byte stores (the second store implementation)
 *   JPEGBLK_ROW_TILING     1 = the row-bound tiling for every image
 *   JPEGBLK_PASS1          1 = a batch run always reads every file's headers first (default: only while the decoder's
 *                          buffers do not exist yet; otherwise a file is parsed when its group is formed)
 *   JPEGBLK_GROUP_RAMP     1 = a host thread's first two device groups are a quarter and a half of the full size
 *   JPEGBLK_GROUP_MB       MB of coefficients per group of small images on the host path (16; 0 = one image per submission)
 *   JPEGBLK_DEV_GROUP_MB   MB of coefficients per group whose entropy stage runs on the device (96)
 *   JPEGBLK_NUMA           0 = leave the host threads' CPU affinity alone, 1 = always bind them to the GPU's node
 *   JPEGBLK_OVERSUBSCRIBE  1 = allow more host threads than CPUs the process may use
 *   JPEGBLK_STAGED_STORE   1 = (measurement builds of the kernels only, tools/build_variant.sh; the product ignores it) the
 *                          staged, line-aligned store stage for every image that takes the linear tiling
 *   JPEGBLK_SMALL_GRID     1 = always the one-wave kernels (every layout has one), 0 = never (default: launches of
 *                          up to 8 workgroups per CU of the 192-lane kernel, e.g. one to four 1080p images, one 4096x4096 4:2:0)
 *   JPEGBLK_FLAT_FRONT     0 = never the flat entry of the 4:4:4 pixel kernel (default: every launch whose tiles are all
 *                          full and whose images' coefficients lie densely takes it; see jb_ctx_last_front)
 *   JPEGBLK_TIMING         1 | 2 | 3 = where one decode(bytes) / one device-entropy submission / one batch run spends its time (stderr)
 *   JPEGBLK_RESIZE_TMP_BYTES  bytes of full-size intermediates one launch pair of a decode to a fixed output size may
 *                          hold (default 128 MiB; more runs as sub-batches of whole images, one image at the least;
 *                          with per-image rectangles a sub-batch also ends after 32 images)
 *   JPEGBLK_HW_QUEUES      read when the library is LOADED: hardware queues to ask the HIP runtime for
 *                          (GPU_MAX_HW_QUEUES; default 16, 0 = the runtime's default).  Process-wide, and only
 *                          effective before HIP initialises: an application that initialises HIP first sets
 *                          GPU_MAX_HW_QUEUES=16 itself (batch decoders: +13 % host path, +13-40 % device path).
 */
#ifndef JPEGBLK_H
#define JPEGBLK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JB_ABI_VERSION 1

typedef enum jb_status {
  JB_OK = 0,
  JB_ERR_NULL = -1,        /* a required pointer is NULL                                   */
  JB_ERR_GEOMETRY = -2,    /* width/height/stride out of range                             */
  JB_ERR_SAMPLING = -3,    /* luma factors not in {1,2}x{1,2} (reference jpeg.cpp:110-136) */
  JB_ERR_QTAB = -4,        /* qtab_id outside 0..3 (reference jpeg.cpp:205-209)            */
  JB_ERR_CAPACITY = -5,    /* image larger than the context / buffer was created for       */
  JB_ERR_HIP = -6,         /* HIP runtime error; text via jb_last_error()                  */
  JB_ERR_STATE = -7,       /* bad ticket / nothing in flight / context busy                */
  JB_ERR_FORMAT = -8,      /* front end: not a JPEG / corrupt segment                      */
  JB_ERR_UNSUPPORTED = -9  /* front end: a frame type it does not decode (12-bit, arithmetic, 4 components ...) */
} jb_status;

/* What Image state the seam reads: image_width/height (jpeg.cpp:792-793), the luma sampling
 * factors (jpeg.cpp:32-33) and color_components[i].quantizationTableID (jpeg.cpp:23). */
typedef struct jb_image_desc {
  int32_t width;      /* pixels, 1..65535 */
  int32_t height;     /* pixels, 1..65535 */
  int32_t hs;         /* luma horizontal sampling factor, 1 or 2; chroma is always 1x1 */
  int32_t vs;         /* luma vertical sampling factor, 1 or 2 */
  int32_t qtab_id[3]; /* quantisation table of Y, Cb, Cr: 0..3 */
  int32_t reserved;   /* must be 0 */
} jb_image_desc;

/* Sizes derived from a descriptor (read_sof, jpeg.cpp:77-80 and 118-127). */
typedef struct jb_geometry {
  int32_t mcu_w, mcu_h;           /* 8x8 block columns/rows covering the image: (W+7)/8, (H+7)/8 */
  int32_t mcu_w_real, mcu_h_real; /* rounded up to a multiple of hs / vs                         */
  int32_t mcus_x, mcus_y;         /* coded MCUs per row / column                                 */
  int32_t blocks_per_mcu;         /* hs*vs + 2                                                   */
  int32_t reserved;
  int64_t n_coded_blocks;         /* mcus_x*mcus_y*blocks_per_mcu                                */
  int64_t coef_bytes;             /* n_coded_blocks * 128                                        */
  int64_t rgb_bytes;              /* width*height*3 (tight rows)                                 */
} jb_geometry;

typedef struct jb_ctx jb_ctx;

/* ---- library / context --------------------------------------------------------------- */
int jb_abi_version(void);
/* Number of HIP devices visible, or a negative jb_status. */
int jb_device_count(void);
/* Validate a descriptor and derive its sizes.  Pure host code, no device needed. */
int jb_geometry_of(const jb_image_desc *desc, jb_geometry *out);
/* Create a context on `device_id` with its own stream.  `max_coef_bytes`/`max_rgb_bytes`
 * size the per-slot device and pinned staging buffers used by the host-buffer entry points
 * (0,0: device-pointer entry points only).  `n_slots` (1..64) = depth of the staging ring
 * (each slot holds one image's coefficients and pixels in device memory). */
int jb_ctx_create(int device_id, size_t max_coef_bytes, size_t max_rgb_bytes, int n_slots,
                  jb_ctx **out);
void jb_ctx_destroy(jb_ctx *ctx);
/* Grow the staging ring of a context to images of up to (max_coef_bytes, max_rgb_bytes); a
 * context created with (0,0) gets its ring (of the depth given at creation) here.  Waits for
 * everything in flight first; never shrinks.  jb_decode_file / jb_decode_memory call this with the
 * parsed frame's sizes, so a context need not know its largest image in advance (the reference's
 * Image allocates `new MCU[...]` per file from the SOF sizes, jpeg.cpp:407). */
int jb_ctx_reserve(jb_ctx *ctx, size_t max_coef_bytes, size_t max_rgb_bytes);
/* The HIP device a context lives on. */
int jb_ctx_device(const jb_ctx *ctx);
/* Text of the last error on this context (or of the last context-less error on this thread
 * when ctx is NULL).  Never NULL. */
const char *jb_last_error(const jb_ctx *ctx);
/* The context's primary HIP stream (hipStream_t): what device-resident launches with a NULL
 * stream argument run on, so callers can order their own work against them.  (The staging ring
 * of jb_submit uploads and computes on this stream and downloads on a second one, so that the
 * device->host copy of image i overlaps the host->device copy of image i+1; order against the
 * downloads with jb_wait.) */
void *jb_ctx_stream(jb_ctx *ctx);
/* Block until everything submitted to the context (either stream) has finished. */
int jb_ctx_synchronize(jb_ctx *ctx);

/* ---- the seam: host buffers (drop-in for jpeg.cpp:786-788) ----------------------------- */
/* Synchronous: copies coefficients to the device, runs the fused kernel, copies pixels back.
 * `qtabs` = 4*64 uint16 natural order (tables not referenced by desc->qtab_id may be 0). */
int jb_blocks_to_rgb(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef,
                     const uint16_t *qtabs, uint8_t *rgb, int64_t rgb_stride);
/* Asynchronous flavour over the staging ring, so the host Huffman stage of image i+1 overlaps
 * the device work of image i.  `coef`/`rgb` should come from jb_pinned_alloc for true overlap
 * and must stay valid until jb_wait(ticket) returns.  Blocks only when all slots are busy.
 * Submissions may complete out of order (small ones run on several stream pairs in turn): wait
 * for the ticket, or jb_ctx_synchronize for everything. */
int jb_submit(jb_ctx *ctx, const jb_image_desc *desc, const int16_t *coef,
              const uint16_t *qtabs, uint8_t *rgb, int64_t rgb_stride, int *ticket);
/* Several images of ONE geometry in one submission (one upload, one launch, one download): for
 * small images, where the per-submission cost (tens of microseconds of driver calls) would
 * otherwise bound the rate.  coef = n_images consecutive images (coef_bytes each), qtabs =
 * n_images x 4*64 uint16, rgb = n_images consecutive images with tightly packed rows.
 * n_images <= 256 and n_images x (coef_bytes, rgb_bytes) within the context's capacity. */
int jb_submit_batch(jb_ctx *ctx, const jb_image_desc *desc, int n_images, const int16_t *coef,
                    const uint16_t *qtabs, uint8_t *rgb, int *ticket);
int jb_wait(jb_ctx *ctx, int ticket);
/* Non-blocking jb_wait: JB_OK once the submission has completed, JB_PENDING (> 0, not an error)
 * while it is still in flight. */
#define JB_PENDING 1
int jb_poll(jb_ctx *ctx, int ticket);
/* Pinned host memory for the coefficient / pixel buffers handed to jb_submit (the reference's
 * `new MCU[...]`, jpeg.cpp:407, is the buffer this replaces).  Pinned memory is pinned against a
 * device and placed on the host NUMA node closest to it: jb_pinned_alloc_on names the device --
 * use it with the device of the context the buffer will be submitted to, above all from threads
 * that never called hipSetDevice (their current device is 0 whatever GPU the process drives).
 * jb_pinned_alloc = jb_pinned_alloc_on(the calling thread's current device). */
void *jb_pinned_alloc_on(int device_id, size_t bytes);
void *jb_pinned_alloc(size_t bytes);
void jb_pinned_free(void *p);
/* Host NUMA node closest to a device (>= 0), or a negative jb_status when unknown.  One process
 * per GPU (the reference decodes one image per process, jpeg.cpp:916-929): a rank keeps its
 * entropy threads and its staging on this node. */
int jb_device_numa_node(int device_id);

/* ---- the seam: device-resident buffers (what bench.py and multi-image batches use) ------ */
/* A batch = n_images images of identical geometry, processed by ONE kernel launch on `stream`
 * (NULL = the context's stream).  Every pointer is a device pointer.  d_qtabs holds, per image
 * (or once, when qtab_image_stride == 0), three tables int32[3][64] already resolved per
 * component (Y, Cb, Cr) in natural order; build them with jb_resolve_qtabs(). */
typedef struct jb_device_batch {
  jb_image_desc desc;
  int32_t n_images;
  int32_t reserved;
  const int16_t *d_coef;
  int64_t coef_image_stride; /* bytes between images, multiple of 16 */
  const int32_t *d_qtabs;
  int64_t qtab_image_stride; /* bytes between images' [3][64] tables; 0 = shared */
  uint8_t *d_rgb;
  int64_t rgb_image_stride; /* bytes between images */
  int64_t rgb_row_stride;   /* bytes between pixel rows, >= 3*width; any value works (lanes store 12 bytes
                             * at byte-aligned addresses), multiples of 64 are fastest: on small images
                             * a tightly packed odd stride costs about ten points of roofline (partial
                             * lines at the ends of every 768-byte wave store) */
} jb_device_batch;

int jb_blocks_to_rgb_device(jb_ctx *ctx, const jb_device_batch *batch, void *stream);
/* Host helper: expand (qtabs uint16[4][64], qtab_id[3]) into the int32[3][64] the kernel reads. */
int jb_resolve_qtabs(const jb_image_desc *desc, const uint16_t *qtabs, int32_t *out192);
/* Name of the kernel jb_blocks_to_rgb_device launches for this descriptor (for profilers): the 192 / 256-lane
 * kernel of the layout.  Launches of up to 8 of its workgroups per CU (one to four 1080p images, one 4096x4096
 * 4:2:0) run as jb_small_kernel_444 / _420 / _16<2,1> / _16<1,2> instead (JPEGBLK_SMALL_GRID): four entry points
 * of one kernel body, one per layout. */
const char *jb_kernel_name(const jb_image_desc *desc);
/* Which front end the context's last launch of that kernel took, for tests and profilers: JB_FRONT_FLAT when every
 * workgroup's coefficients start at d_coef + workgroup * tile bytes -- 4:4:4 at full size, the whole image, every tile
 * full (64 MCUs) and the images coef_image_stride = their own length apart -- so that the kernel issues its loads before it
 * has read anything else of its arguments; JB_FRONT_GENERAL otherwise; JB_FRONT_NONE before the first such launch.  The
 * output's pitch, strides and width play no part, and the pixels are the same either way.  A profiler sees a flat launch
 * as jb_tile_kernel_flat<LINEAR, FORMAT>: the body of jb_kernel_name's kernel behind a second entry.  *linear (may be NULL): 1 when
 * that launch's tiles followed the MCU stream across MCU rows, 0 when each was a run of one MCU row. */
#define JB_FRONT_NONE 0
#define JB_FRONT_GENERAL 1
#define JB_FRONT_FLAT 2
int jb_ctx_last_front(const jb_ctx *ctx, int *linear);
/* The geometry behind JB_FRONT_FLAT, a pure host function: would n_images images of mcus_x x mcus_y MCUs with luma
 * sampling (hs, vs), coef_image_stride bytes apart, tiled along the MCU stream (linear = 1) or per MCU row (0), be such a
 * launch?  1 or 0; 0 for arguments outside their range. */
int jb_flat_front_geometry(int hs, int vs, int linear, int32_t mcus_x, int32_t mcus_y, int32_t n_images, int64_t coef_image_stride);

/* ---- scaled output: decode at 1/2, 1/4 or 1/8 size ---------------------------------------
 * For denom K in {1, 2, 4, 8} an image of W x H decodes to ceil(W/K) x ceil(H/K) RGB pixels (interleaved
 * uint8, the layout above), each the rounded mean of its K x K box of the full-size output:
 *
 *     out[y][x][c] = floor((S + n/2) / n),  S = sum of full[yy][xx][c] over yy in [K*y, min(K*y+K, H)),
 *                                               xx in [K*x, min(K*x+K, W)),  n = number of such (yy, xx)
 *
 * where `full` is what the entry points above return for the image, bit for bit (so n = K*K inside the image and
 * fewer in the last column / row; the MCU padding beyond W x H never enters a sum).  This is an AREA (box) filter on
 * the decoded pixels, computed in the pixel kernel from the very samples it would have stored -- NOT the DCT-domain
 * reduced IDCT of libjpeg's scale_denom, whose output differs; inside the image it equals PIL's Image.reduce(K).
 * What is saved is output bytes (HBM writes, and the device-to-host link on the host-output forms): K^2 fewer.
 * K = 1 is the full-size path, unchanged.  A denom outside {1, 2, 4, 8} is JB_ERR_GEOMETRY everywhere.
 * The scaled launches use the row-bound tiling and ignore JPEGBLK_SMALL_GRID and JPEGBLK_BYTE_STORE. */
/* Output size of a W x H image at 1/denom.  Pure host code. */
int jb_scaled_size(int32_t width, int32_t height, int denom, int32_t *out_w, int32_t *out_h);
/* jb_blocks_to_rgb_device at 1/denom: d_rgb receives n_images images of jb_scaled_size(desc) pixels,
 * rgb_row_stride >= 3 * out_w, rgb_image_stride >= rgb_row_stride * out_h (n_images > 1).  denom = 1 is
 * jb_blocks_to_rgb_device. */
int jb_blocks_to_rgb_device_scaled(jb_ctx *ctx, const jb_device_batch *batch, int denom, void *stream);
/* jb_decode_memory / jb_decode_file at 1/denom: *rgb holds out_w x out_h pixels (tight rows), *width / *height
 * report the OUTPUT size.  Both entropy paths take the scale (the same rule picks the device entropy stage). */
int jb_decode_memory_scaled(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, int denom, uint8_t **rgb,
                            int32_t *width, int32_t *height);
int jb_decode_file_scaled(jb_ctx *ctx, const char *path, int denom, uint8_t **rgb, int32_t *width, int32_t *height);

/* ---- tensor-ready output: planar u8, or normalised f32 / f16, written by the pixel kernel ----
 * An OUTPUT FORMAT says what the pixel kernel stores.  With `full` = what the entry points above return for the
 * image, bit for bit (interleaved uint8):
 *
 *     JB_FMT_RGB_U8_HWC   uint8    interleaved R,G,B -- the default: this value takes exactly the old code paths
 *     JB_FMT_RGB_U8_CHW   uint8    three planes R, G, B of `height` rows:  plane[c][y][x] = full[y][x][c]
 *     JB_FMT_RGB_F32_CHW  float    the same planes:  (float)full[y][x][c] * scale[c] + bias[c]
 *     JB_FMT_RGB_F16_CHW  half     the f32 value above converted to IEEE binary16, round to nearest even
 *
 * i.e. one image is a [3, H, W] tensor, a batch of equal images [N, 3, H, W]: what a model reads, without a
 * permute / convert / normalise pass over HBM behind the decoder.  The float value is defined operation by
 * operation -- uint8 -> f32 (exact), ONE f32 multiply, then ONE f32 add (not fused), then for f16 one conversion --
 * so NumPy's (u.astype(float32) * float32(s) + float32(b)) [.astype(float16)] reproduces it bit for bit.  ImageNet
 * normalisation is scale[c] = 1 / (255 * std[c]), bias[c] = -mean[c] / std[c].
 * Not combined with scaled output: a format other than JB_FMT_RGB_U8_HWC together with denom != 1 is
 * JB_ERR_UNSUPPORTED on every route.  The host-buffer seam (jb_blocks_to_rgb, jb_submit, jb_submit_batch) stays
 * interleaved.  An unknown format, reserved != 0, a plane_stride smaller than row stride * height, or a scale / bias
 * that is not finite is JB_ERR_GEOMETRY.  The planar launches use the row-bound tiling and ignore JPEGBLK_SMALL_GRID
 * and JPEGBLK_BYTE_STORE. */
enum { JB_FMT_RGB_U8_HWC = 0, JB_FMT_RGB_U8_CHW = 1, JB_FMT_RGB_F32_CHW = 2, JB_FMT_RGB_F16_CHW = 3 };
typedef struct jb_output_spec {
  int32_t format;       /* JB_FMT_* */
  int32_t reserved;     /* 0 */
  int64_t plane_stride; /* device seam only: bytes between the planes of one image; 0 = rgb_row_stride * height */
  float scale[3];       /* float formats only (ignored otherwise) */
  float bias[3];
} jb_output_spec;
/* Bytes of one W x H image in `format` with tight rows and planes: 3 * W * H * element size.  Pure host code. */
int jb_output_bytes(int32_t width, int32_t height, int format, int64_t *bytes);
/* Validate a spec against planes of `height` rows, `row_stride` bytes apart (the rules above).  Pure host code. */
int jb_output_spec_check(const jb_output_spec *spec, int32_t height, int64_t row_stride);
/* jb_blocks_to_rgb_device in spec->format.  For a planar format batch->rgb_row_stride is the bytes between the rows
 * OF A PLANE (>= width * element size), spec->plane_stride between the planes, batch->rgb_image_stride between the
 * images (>= 3 planes).  uint8 planes may start anywhere and take any strides; f32 / f16 want d_rgb and all three
 * strides to be multiples of the element size (else JB_ERR_GEOMETRY).  format 0 is jb_blocks_to_rgb_device. */
int jb_blocks_to_rgb_device_fmt(jb_ctx *ctx, const jb_device_batch *batch, const jb_output_spec *spec, void *stream);
/* jb_decode_memory / jb_decode_file in spec->format: *out is malloc'ed (jb_free), tight rows and planes
 * (jb_output_bytes), elements of the format's type.  Both entropy paths take the format (the same rule picks the
 * device entropy stage); spec->plane_stride must be 0 here. */
int jb_decode_memory_fmt(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_output_spec *spec, void **out,
                         int32_t *width, int32_t *height);
int jb_decode_file_fmt(jb_ctx *ctx, const char *path, const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);

/* ---- region of interest: decode a rectangle of the image, cropped by the pixel kernel ----
 * With `full` = what the entry points above return for the image in the same format, bit for bit, a decode with the
 * rectangle (x, y, width, height) returns full[y : y + height, x : x + width] (of every plane, for a planar format): the
 * pixel kernel launches only the MCUs the rectangle touches and stores only the pixels inside it, so the output -- HBM
 * writes, and the device-to-host link on the host-output forms -- is the rectangle's.  The entropy stage still decodes
 * the whole image.  Every output format takes a rectangle; a scale other than 1 does not (the seam and jb_decode_*_roi
 * cannot express the pair; the batch decoder refuses it with JB_ERR_UNSUPPORTED).  The ROI launches use the row-bound
 * tiling and ignore JPEGBLK_SMALL_GRID and JPEGBLK_BYTE_STORE. */
typedef struct jb_roi {
  int32_t x, y, width, height; /* pixels of the full-size image */
} jb_roi;
/* JB_OK when x, y >= 0, width, height >= 1, x + width <= desc->width and y + height <= desc->height (sums that do not
 * wrap); JB_ERR_NULL for a null argument; the descriptor's own errors (jb_geometry_of) first; else JB_ERR_GEOMETRY.
 * Pure host code. */
int jb_roi_check(const jb_image_desc *desc, const jb_roi *roi);
/* jb_blocks_to_rgb_device_fmt for one rectangle shared by the batch's images: d_rgb and the strides describe images of
 * roi->width x roi->height (every alignment and stride that is legal for a full-size image of that size is legal here;
 * the spec is checked against the rectangle's height).  spec == NULL: interleaved uint8.  roi == NULL: exactly
 * jb_blocks_to_rgb_device_fmt (jb_blocks_to_rgb_device when spec is NULL too). */
int jb_blocks_to_rgb_device_roi(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *roi, const jb_output_spec *spec,
                                void *stream);
/* jb_decode_memory_fmt / jb_decode_file_fmt of a rectangle: *out holds jb_output_bytes(roi->width, roi->height, format)
 * bytes (jb_free), *width / *height report the rectangle's size.  spec == NULL: interleaved uint8.  A rectangle that does
 * not fit the file's frame is JB_ERR_GEOMETRY (jb_last_error names both sizes). */
int jb_decode_memory_roi(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_output_spec *spec,
                         void **out, int32_t *width, int32_t *height);
int jb_decode_file_roi(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_output_spec *spec, void **out,
                       int32_t *width, int32_t *height);

/* ---- fixed output size: decode to out_w x out_h, an exact area resize on the device ----
 * With `src` = the full-size uint8 decode (iw x ih), or with a rectangle full[y : y + h, x : x + w], the result is defined
 * on a common grid of iw * out_w units per axis: source column i covers [i * out_w, (i + 1) * out_w), output column j
 * covers [j * iw, (j + 1) * iw), wx[j][i] is the integer length of their overlap (sum over i = iw); rows the same with
 * wy, ih, out_h.  Per channel
 *     S = sum_r sum_i wy[k][r] * wx[j][i] * src[r][i][c]      (an exact integer)
 *     out_u8[k][j][c] = floor((S + floor(D / 2)) / D),  D = iw * ih
 * -- one rounding, half up.  The same formula reduces, enlarges (a box filter: blocky) and mixes the two per axis;
 * out_w = iw, out_h = ih gives src bit for bit; iw = k * out_w, ih = k * out_h with k = 2, 4, 8 gives the scaled output
 * of scale k bit for bit; a constant image stays constant.  The planar formats apply to out_u8 exactly as they apply
 * to a full-size decode (value = (float)u8 * scale[c] + bias[c]).  Any format, with or without a rectangle, never with
 * a scale other than 1 (JB_ERR_UNSUPPORTED); out_w, out_h in 1..65535 (else JB_ERR_GEOMETRY).
 * Two launches in stream order: the pixel kernel writes src as tight interleaved uint8 into a scratch the context
 * owns (it grows on demand, which allocates: not inside a graph capture; one per stream that is used, each at most
 * JPEGBLK_RESIZE_TMP_BYTES or one image), a second kernel reads it and writes the caller's buffer.  A batch whose
 * intermediates exceed the cap runs as consecutive sub-batches of whole images.  The entropy stage still decodes the
 * whole image. */
/* JB_OK when the rectangle (NULL: the whole image) lies in the image and out_w, out_h are in 1..65535; JB_ERR_NULL for
 * a null descriptor; the descriptor's own errors (jb_geometry_of) first, then the rectangle's, then the target's (both
 * JB_ERR_GEOMETRY).  Pure host code. */
int jb_resize_check(const jb_image_desc *desc, const jb_roi *roi, int32_t out_w, int32_t out_h);
/* jb_blocks_to_rgb_device_roi at a fixed output size: d_rgb and the strides describe images of out_w x out_h (every
 * alignment and stride that is legal for a full-size image of that size is legal here; nothing outside the out_w x
 * out_h elements is written).  roi == NULL: the whole image.  spec == NULL: interleaved uint8. */
int jb_blocks_to_rgb_device_resized(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *roi, int32_t out_w, int32_t out_h,
                                    const jb_output_spec *spec, void *stream);
/* jb_decode_memory_roi / jb_decode_file_roi at a fixed output size: *out holds jb_output_bytes(out_w, out_h, format)
 * bytes (jb_free), *width / *height report out_w / out_h.  roi == NULL: the whole image.  spec == NULL: interleaved uint8. */
int jb_decode_memory_resized(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, int32_t out_w, int32_t out_h,
                             const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);
int jb_decode_file_resized(jb_ctx *ctx, const char *path, const jb_roi *roi, int32_t out_w, int32_t out_h,
                           const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);

/* ---- per-image rectangles: a different rectangle for every image of a batch, all at one output size ----
 * The random-resized-crop of a training pipeline in one call.  For image i of the call, with rectangle r_i = (x, y, w, h)
 * in pixels of that image's full-size decode and ONE target out_w x out_h for the call,
 *     out_i = format(area_resize(full_i[y : y + h, x : x + w], out_w, out_h))
 * -- bit for bit what jb_blocks_to_rgb_device_resized writes for a batch of that one image with &r_i, in every format
 * (no new arithmetic: "fixed output size" above).  out_w = w_i, out_h = h_i gives the slice itself.  A target size is
 * required (it is what makes the outputs one size); never with a scale other than 1 (JB_ERR_UNSUPPORTED).
 * Still two launches in stream order per sub-batch: consecutive images share a launch pair while their tight
 * intermediates (3 * w_i * h_i bytes each, back to back) fit the stream's scratch (JPEGBLK_RESIZE_TMP_BYTES; a larger
 * image runs alone) and there are at most 32 of them.  The rectangles of a sub-batch travel in the kernels' arguments:
 * nothing is uploaded, and the caller's array is not needed once the call has returned. */
/* JB_OK when every one of the n rectangles lies in the image and out_w, out_h are in 1..65535 (n = 0: only the target is
 * checked); else the status of the first rectangle that fails (JB_ERR_GEOMETRY) with its index in *bad_index (may be
 * NULL; -1 when no rectangle is to blame: a bad target, a bad descriptor).  JB_ERR_NULL for a null descriptor or array;
 * the descriptor's own errors first, then the rectangles', then the target's.  Pure host code. */
int jb_crops_check(const jb_image_desc *desc, const jb_roi *rois, int n, int32_t out_w, int32_t out_h, int *bad_index);
/* jb_blocks_to_rgb_device_resized with a rectangle per image: rois is a HOST array of batch->n_images rectangles, read
 * before the call returns (the caller may reuse it at once).  d_rgb and the strides describe images of out_w x out_h,
 * exactly as for _resized.  rois == NULL: JB_ERR_NULL.  A rectangle outside the frame: JB_ERR_GEOMETRY, jb_last_error
 * names the image's index and both sizes; nothing is launched and nothing is written.  The target's checks are those
 * of _resized.  spec == NULL: interleaved uint8. */
int jb_blocks_to_rgb_device_crops(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *rois, int32_t out_w, int32_t out_h,
                                  const jb_output_spec *spec, void *stream);

/* ---- resampling filters: Pillow-exact bilinear and bicubic for the fixed output size and the per-image rectangles ----
 * The two sections above resize with an exact AREA filter.  A `filter` chooses what gets to the target instead:
 *
 *     JB_FILTER_AREA      the arithmetic and the code paths of the two sections above, untouched
 *     JB_FILTER_BILINEAR  support S = 1:  f(x) = 1 - |x| for |x| < 1, else 0
 *     JB_FILTER_BICUBIC   support S = 2, a = -0.5, with x = |x|:  ((a + 2) x - (a + 3)) x x + 1 for x < 1,
 *                         (((x - 5) x + 8) x - 4) a for x < 2, else 0
 *
 * and the result is, bit for bit, what Pillow's 8-bit resampling gives: Image.resize((out_w, out_h), BILINEAR / BICUBIC,
 * box=(x, y, x + w, y + h)) of the full-size decode (what torchvision's antialiased Resize computes on PIL images).
 * The RESIZE is Pillow's; the full-size DECODE it is applied to is Pillow's own -- Image.open(f).convert("RGB") -- only
 * under JB_ARITH_LIBJPEG ("decoder arithmetic" below), and the reference program's otherwise.
 * The weights of one axis -- frame extent in_size (the WHOLE image, not the rectangle), rectangle [in0, in1), n outputs --
 * are computed on IEEE doubles, every operation in exactly this order and none fused:
 *
 *     scale = (in1 - in0) / n;   fs = scale < 1.0 ? 1.0 : scale;   sup = S * fs;   inv = 1.0 / fs
 *     for j in 0..n-1:
 *         center = in0 + (j + 0.5) * scale
 *         lo = (int)(center - sup + 0.5);  if lo < 0: lo = 0                  ((int) truncates toward zero)
 *         hi = (int)(center + sup + 0.5);  if hi > in_size: hi = in_size
 *         for t in 0..hi-lo-1:  w[t] = f((t + lo - center + 0.5) * inv)
 *         ww = 0.0;  for t in order: ww += w[t]                               (a SEQUENTIAL sum, in tap order)
 *         if ww != 0.0:  w[t] = w[t] / ww  for every t
 *         k[t] = (int)(w[t] * 4194304.0 + 0.5)  if w[t] >= 0  else  (int)(w[t] * 4194304.0 - 0.5)
 *
 * With `full` the full-size uint8 decode (W x H) and the rectangle (x, y, w, h) (none: the whole image):
 *     horizontal, for every frame row r:  T[r][j][c] = clip8((2^21 + sum_t kx_j[t] * full[r][lo_j + t][c]) >> 22)
 *                                         (columns: in_size = W, in0 = x, in1 = x + w, n = out_w)
 *     vertical:                      out_u8[k][j][c] = clip8((2^21 + sum_t ky_k[t] * T[lo_k + t][j][c]) >> 22)
 *                                         (rows: in_size = H, in0 = y, in1 = y + h, n = out_h)
 * `>>` is the arithmetic shift of a signed 32-bit sum, clip8 clamps to 0..255, and T is rounded to uint8 between the
 * passes.  Formats 1-3 apply to out_u8 exactly as everywhere else.  What follows from the definition:
 *   - THE FILTER READS PIXELS OUTSIDE THE RECTANGLE: lo and hi are clamped to the frame, not to the rectangle, so a crop's
 *     edge pixels depend on their neighbours outside it.  That is Pillow's box=, and it is NOT what cropping first and
 *     resizing the crop (torchvision's RandomResizedCrop on a tensor) computes.
 *   - out_w = w, out_h = h reproduces the slice bit for bit under both filters (weights 1 and 0).
 *   - the order of the ww sum is part of the definition.
 * The cap: an axis counts floor(2 * sup) + 2 taps (an upper bound of hi - lo), and more than 160 on either axis is
 * JB_ERR_UNSUPPORTED (jb_last_error names the cap): bicubic reduces up to 39x per axis, bilinear up to 79x.
 * The source window -- per axis the union of [lo, hi) over all outputs: the rectangle grown by the filter's reach and
 * clamped to the frame -- is what the pixel kernel writes into the stream's scratch in the rectangle's place; the
 * intermediates, the sub-batches and JPEGBLK_RESIZE_TMP_BYTES work as in the two sections above with the window's size.
 * A jb_resize names the target and the filter; out_w = out_h = 0 means "no target size", which only filter 0 goes with.
 * Refusals, behind those of the sections above and in this order: an unknown filter or reserved != 0 JB_ERR_GEOMETRY; a
 * filter other than JB_FILTER_AREA without a target size JB_ERR_STATE; the cap JB_ERR_UNSUPPORTED. */
enum { JB_FILTER_AREA = 0, JB_FILTER_BILINEAR = 1, JB_FILTER_BICUBIC = 2 };
typedef struct jb_resize {
  int32_t out_w, out_h; /* the target size */
  int32_t filter;       /* JB_FILTER_* */
  int32_t reserved;     /* 0 */
} jb_resize;
/* jb_resize_check with a filter: JB_ERR_NULL for a null descriptor or jb_resize; the descriptor's own errors first, then
 * the rectangle's (NULL: the whole image), the target's, the filter's (above).  Pure host code. */
int jb_filter_check(const jb_image_desc *desc, const jb_roi *roi, const jb_resize *rs);
/* The source window of the request (jb_filter_check's statuses first): the pixels of the frame the filter reads.  With
 * JB_FILTER_AREA the rectangle itself.  Pure host code. */
int jb_filter_window(const jb_image_desc *desc, const jb_roi *roi, const jb_resize *rs, jb_roi *window);
/* jb_blocks_to_rgb_device_resized / _crops with rs->filter: everything said there about d_rgb, the strides, the spec
 * and the rectangles holds.  rs->filter = JB_FILTER_AREA gives exactly what those entry points give.  rs == NULL:
 * JB_ERR_NULL. */
int jb_blocks_to_rgb_device_filtered(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *roi, const jb_resize *rs,
                                     const jb_output_spec *spec, void *stream);
int jb_blocks_to_rgb_device_crops_filtered(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *rois, const jb_resize *rs,
                                           const jb_output_spec *spec, void *stream);
/* jb_decode_memory_resized / jb_decode_file_resized with rs->filter. */
int jb_decode_memory_filtered(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_resize *rs,
                              const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);
int jb_decode_file_filtered(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_resize *rs, const jb_output_spec *spec,
                            void **out, int32_t *width, int32_t *height);

/* ---- views: several rectangles per image, each optionally mirrored, from one decode ----
 * The K random crops of a multi-view training pipeline, and the random horizontal flip, in one call.  A call has
 * views_per_image = K in 1..16 and a HOST array of n_images * K views; view v of image i is views[i * K + v].  One
 * jb_resize holds the target and the filter (JB_FILTER_AREA is allowed).  Output number i * K + v is
 *     u   = what "per-image rectangles" gives for image i with the rectangle views[i * K + v] and the same jb_resize
 *     out = format(flags & JB_VIEW_MIRROR ? u[:, ::-1, :] : u)
 * -- no new arithmetic: the definitions, the refusals, the tap cap and the frame-clamped filter bounds are those of "fixed
 * output size", "per-image rectangles" and "resampling filters".  THE MIRROR IS APPLIED LAST, on the uint8 result
 * (torchvision's order: RandomResizedCrop, then RandomHorizontalFlip): Pillow's normalised weights are not mirror-
 * symmetric in general, so mirroring the source first gives other bits.  Formats 0-3, the context's arithmetic and its
 * orientation compose unchanged: rectangles are in oriented coordinates, and the mirror is still last.
 * The entropy stage and the pixel kernel run ONCE per image: the pixel kernel writes the image's UNION -- the bounding
 * rectangle of its K rectangles, with a filter of their K source windows -- into the stream's scratch, and the resample
 * or filter kernel reads K sub-rectangles of it; a mirrored view differs in the store address alone.  A union can be
 * larger than the sum of its views (two small rectangles in opposite corners: nearly the frame); that is accepted, the
 * pixel kernel is cheap next to the entropy stage.  Sub-batches pack images while their unions fit
 * JPEGBLK_RESIZE_TMP_BYTES (a larger one runs alone), at most 32 images each.
 * Refusals: K outside 1..16, unknown flag bits or reserved != 0 JB_ERR_GEOMETRY; a rectangle outside the frame
 * JB_ERR_GEOMETRY (jb_last_error names the image's and the view's index); no target size (out_w = out_h = 0)
 * JB_ERR_STATE; then the target's and the filter's own.  The batch decoder refuses views together with a scale other
 * than 1 or a decoder-wide rectangle with JB_ERR_UNSUPPORTED.  In every refusal nothing is launched or written. */
enum { JB_VIEW_MIRROR = 1 }; /* flags bit 0: mirror the OUTPUT left-right */
typedef struct jb_view {
  int32_t x, y, width, height; /* as jb_roi */
  int32_t flags;               /* JB_VIEW_* */
  int32_t reserved;            /* 0 */
} jb_view;
enum { JB_VIEWS_MAX = 16 };
/* JB_OK when the call can be had.  JB_ERR_NULL for a null descriptor, jb_resize or (n_images * views_per_image > 0)
 * array; the descriptor's own errors; JB_ERR_GEOMETRY for n_images < 0 or views_per_image outside 1..16; then the
 * first view that fails -- flags or reserved, else its rectangle: JB_ERR_GEOMETRY -- with its index in the FLAT array in
 * *bad_index (may be NULL; -1 when no view is to blame); then JB_ERR_STATE without a target size, the target's and the
 * filter's statuses as jb_filter_check gives them (the tap cap: *bad_index names the view).  Pure host code. */
int jb_views_check(const jb_image_desc *desc, const jb_view *views, int n_images, int views_per_image, const jb_resize *rs,
                   int *bad_index);
/* d_rgb and its strides describe batch->n_images * views_per_image outputs of out_w x out_h, rgb_image_stride apart
 * (checked whenever there is more than one output); output i * K + v is at index i * K + v.  Everything else about the
 * batch is as for jb_blocks_to_rgb_device_crops_filtered.  The array is read before the call returns.  views or rs ==
 * NULL: JB_ERR_NULL.  spec == NULL: interleaved uint8. */
int jb_blocks_to_rgb_device_views(jb_ctx *ctx, const jb_device_batch *batch, const jb_view *views, int views_per_image,
                                  const jb_resize *rs, const jb_output_spec *spec, void *stream);

/* ---- view groups: several output sizes per image from one decode ----
 * The multi-crop pipelines (DINO, DINOv2, iBOT, SwAV: 2 "global" crops at 224 x 224 and 6-10 "local" crops at 96 x 96 of the
 * same file), "the training crop and a thumbnail" and "one crop at three resolutions" in one call.  A call has G = n_groups
 * in 1..4 (JB_VIEW_GROUPS_MAX).  Group g has its own jb_resize -- target and filter; the filters of the groups may differ --
 * and a count K_g >= 1; K = the sum of the K_g lies in 1..JB_VIEWS_MAX.  The HOST array holds n_images * K views,
 * image-major, and within an image group-major: with s_g = the sum of K_h over h < g, the views [i * K + s_g, i * K + s_g +
 * K_g) are group g's of image i.
 * DEFINITION: group g's outputs are what jb_blocks_to_rgb_device_views writes for the same batch with group g's views
 * alone (views_per_image = K_g) and groups[g].rs -- bit for bit, in every format 0-3, under either arithmetic, any
 * orientation of the context and any draft.  No new arithmetic; the mirror stays last; G = 1 is "views".
 * ONE DECODE: per image the pixel kernel writes ONE union -- the bounding rectangle of all K source rectangles, each taken
 * under its own group's resize (with a filter: jb_filter_window at that group's target).  Sub-batches pack images while
 * their unions fit JPEGBLK_RESIZE_TMP_BYTES, at most 32 images each, as for views; per sub-batch every group then takes
 * ceil(images * K_g / 32) resample or filter launches.
 * A jb_view_output says where group g's outputs go: output (i, v) of the group -- v in 0..K_g-1 -- lies at d_out +
 * i * image_stride + v * view_stride, its rows row_stride apart and, for the planar formats, its planes plane_stride apart
 * (0: tight, row_stride * out_h).  The groups' buffers may be one allocation (the batch decoder's layout below) or
 * separate ones; overlap between different groups' outputs is the caller's business. */
enum { JB_VIEW_GROUPS_MAX = 4 };
typedef struct jb_view_group {
  jb_resize rs;     /* the group's target and filter */
  int32_t n_views;  /* K_g >= 1 */
  int32_t reserved; /* 0 */
} jb_view_group;    /* 24 bytes */
typedef struct jb_view_output {
  void *d_out;      /* device */
  int64_t image_stride, view_stride, row_stride, plane_stride; /* bytes */
} jb_view_output;   /* 40 bytes */
/* Can the call be had?  The first failing check in this order decides: NULLs (descriptor, groups, the array when n_images
 * > 0) JB_ERR_NULL; the descriptor's own errors; JB_ERR_GEOMETRY with *bad_index = -1 for n_images < 0, n_groups outside
 * 1..4, a group with n_views < 1 or reserved != 0, K > 16; every view in flat order -- flags and reserved, then the
 * rectangles -- JB_ERR_GEOMETRY with the flat index i * K + v in *bad_index (may be NULL); then every group in order what
 * jb_views_check answers for that group's views with its rs: no target JB_ERR_STATE, the target's and the filter's
 * statuses (the tap cap: *bad_index names the view's flat index in the caller's array).  With G = 1 status and
 * *bad_index are jb_views_check's.  Pure host code. */
int jb_view_groups_check(const jb_image_desc *desc, const jb_view *views, int n_images, const jb_view_group *groups, int n_groups,
                         int *bad_index);
/* The tight layout of one image's block: group 0's K_0 outputs, then group 1's, ..., each output jb_output_bytes of its
 * target in `format`.  group_offsets (may be NULL; n_groups entries): where group g starts; *image_bytes: the block.
 * JB_ERR_NULL, JB_ERR_GEOMETRY for the counts as above, a target outside 1..65535 or an unknown format.  Pure host code. */
int jb_view_groups_bytes(const jb_view_group *groups, int n_groups, int format, int64_t *group_offsets, int64_t *image_bytes);
/* jb_blocks_to_rgb_device_views with groups: outputs[g] describes group g's buffer; batch->d_rgb and its three rgb
 * strides are NOT READ, and spec->plane_stride must be 0 (the planes' stride is the output's own; anything else is
 * JB_ERR_GEOMETRY).  Per group the strides are checked as those of a batch are: row_stride against the width,
 * plane_stride against the rows, view_stride when K_g > 1 against one output, image_stride when n_images > 1 against the
 * image's K_g outputs; the float formats want pointer and strides to be multiples of the element size.  Any refusal
 * launches nothing and writes nothing.  JB_ORIENT_EXIF on the context: JB_ERR_STATE.  The arrays are read before the call
 * returns.  views, groups or outputs == NULL: JB_ERR_NULL.  spec == NULL: interleaved uint8. */
int jb_blocks_to_rgb_device_view_groups(jb_ctx *ctx, const jb_device_batch *batch, const jb_view *views, const jb_view_group *groups,
                                        const jb_view_output *outputs, int n_groups, const jb_output_spec *spec, void *stream);

/* ---- colour chains: per-view colour jitter, grayscale and solarize on the device, Pillow-exact ----
 * What a self-supervised pipeline does behind the flip -- ColorJitter, RandomGrayscale, Solarize -- on the uint8 pixels of
 * every view, in front of the output format (Normalize is the format's scale / bias).  The bits are those of torchvision's
 * PIL backend: ImageEnhance.Brightness / Contrast / Color, the convert("HSV") hue shift, convert("L"), ImageOps.solarize.
 * A CHAIN is 0..JB_COLOR_OPS_MAX operations applied in order, each (op, value) with a float32 value; an empty chain is the
 * identity.  With u an [h, w, 3] uint8 view:
 *   L(p) = (19595 R + 38470 G + 7471 B + 32768) >> 16.
 *   blend(d, v, a), d and v integers in 0..255: t = (float)d + a * (float)(v - d) in float32, product and sum rounded
 *     separately; 0 <= a <= 1: trunc(t); else 0 for t <= 0, 255 for t >= 255, else trunc(t).
 *   JB_COLOR_BRIGHTNESS a: every channel blend(0, v, a).         JB_COLOR_SATURATION a: every channel blend(L(p), v, a).
 *   JB_COLOR_CONTRAST a: S = the sum of L over the view AS IT STANDS when the op is reached, N = w * h,
 *     m = (2 S + N) div (2 N) in 64-bit integers (Pillow's int(mean + 0.5)); every channel blend(m, v, a).
 *   JB_COLOR_GRAYSCALE (value 0): R = G = B = L(p).              JB_COLOR_SOLARIZE t, t integral in 0..256: v < t ? v : 255 - v.
 *   JB_COLOR_HUE d, d integral in 0..255: RGB -> HSV, H = (H + d) & 255, HSV -> RGB, Pillow's two conversions
 *     (csrc/jb_color_core.h states them operation by operation: which steps are float32 and which double decides bits).
 * A chain may hold ONE JB_COLOR_CONTRAST: each costs a reduction pass over the view.
 *
 * NEIGHBOURHOOD operations are numbered from 16 (1..15 are pointwise).  JB_COLOR_BLUR radius is Pillow's
 * ImageFilter.GaussianBlur(radius) -- torchvision's PIL-backend GaussianBlur, DINO's own -- on the view AS IT STANDS when the
 * op is reached: the blur's edges are the view's own edges, nothing from outside the view's rectangle enters.  Pillow does
 * not convolve with a Gaussian: it runs an "extended box blur" three times along every row, then three times along every
 * column, and rounds to uint8 after every pass.  With the float32 radius (jb_blur_params is the one text of this):
 *   sigma2 = radius * radius / 3 (float32);  L = (float32)sqrt(12.0 * (double)sigma2 + 1.0);
 *   l = (float32)floor(((double)L - 1.0) / 2.0);  a = (2 l + 1) * (l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1)(l + 1))),
 *   every operation a float32 one, rounded, none contracted;  fr = l + a.
 *   r = (int)fr;  ww = (uint32)((float32)16777216 / (fr * 2 + 1));  fw = (16777216 - (2 r + 1) ww) / 2  (integers).
 *   one pass along a line of n samples, per channel, c(i) = min(max(i, 0), n - 1):
 *     out[x] = (ww * sum_{k = -r..r} in[c(x + k)] + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + (1 << 23)) >> 24
 *   in unsigned 32-bit integers (the bracket never exceeds 255 * 2^24 + 2^23).  The clamp c() applies to the input of EVERY
 *   pass.  Radius 0 is the identity.
 * A chain may hold ONE JB_COLOR_BLUR (each costs a tile pass), its box radius r at most JB_COLOR_BLUR_BOX_MAX (Gaussian radii
 * up to about 8.4; the published pipelines draw from [0.1, 2.0]: r <= 1), and no JB_COLOR_CONTRAST BEHIND it (the mean would
 * be that of the blurred view, which the reduction pass cannot see; a contrast in front of the blur is DINO's order).  A
 * chain is thus: pointwise operations, at most one blur, pointwise operations without a contrast.
 *
 * The colour operations of RandAugment / AutoAugment / TrivialAugmentWide (torchvision's PIL backend: ImageOps.posterize /
 * invert / autocontrast / equalize, ImageEnhance.Sharpness).  Numbers 0, 7, 9 and 99 stay unassigned.
 *   JB_COLOR_POSTERIZE bits, bits integral in 0..8: every channel v & ~((1 << (8 - bits)) - 1).
 *   JB_COLOR_INVERT (value 0): every channel 255 - v.
 *   JB_COLOR_AUTOCONTRAST (value 0; cutoff 0): per channel, from the histogram of the view AS IT STANDS when the op is reached,
 *     lo / hi = the first / last non-empty bin; hi <= lo: the channel is unchanged; else in fp64, one operation per statement,
 *     scale = 255.0 / (hi - lo), offset = -lo * scale, t = ix * scale, t = t + offset; v becomes lut[v], lut[ix] = t truncated
 *     toward zero and clamped to 0..255.
 *   JB_COLOR_EQUALIZE (value 0): per channel, with counts h[0..255] of the view as it stands: fewer than two non-empty bins:
 *     unchanged; step = (N - h[last non-empty bin]) div 255, step == 0: unchanged; else n = step div 2 and for i = 0..255:
 *     lut[i] = min(n div step, 255), n += h[i].  Integers; counts fit uint32 (w, h <= 65535), n wants 64 bits.
 *   JB_COLOR_SHARPNESS a, finite and >= 0 (a neighbourhood operation): every channel blend(S(p), v, a), S = ImageFilter.SMOOTH:
 *     float32, k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f, acc = 0.5f, acc += (p[y+1][x-1] k1 + p[y+1][x] k1) + p[y+1][x+1] k1, then
 *     row y with k1, k5, k1, then row y - 1, every product and every sum rounded separately;
 *     S = acc <= 0 ? 0 : acc >= 255 ? 255 : (int)acc.  The view's outermost rows and columns are not filtered (S = p there:
 *     the blend leaves them alone); a view narrower or lower than 3 is unchanged.
 * STATISTICS operations are CONTRAST, AUTOCONTRAST and EQUALIZE (each costs a reduction pass): a chain may hold
 * JB_COLOR_STATS_MAX of them, at most one of them a CONTRAST.  NEIGHBOURHOOD operations are BLUR and SHARPNESS (each costs a
 * tile pass): a chain may hold one in all, and no statistics operation behind it.  jb_color_lut is the one text of the two
 * tables.
 *
 * GEOMETRIC operations are numbered from 32: the five affine entries of RandAugment / TrivialAugmentWide / AutoAugment at
 * torchvision's default interpolation (NEAREST) and fill (None: black), with Pillow's bits.  Numbers 0, 7, 9, 14, 15, 18 and
 * 99 stay unassigned.  The value is the float32 torchvision passes: a shear (the tangent), a translation in pixels
 * (integral), a rotation in degrees.  The result has the view's size w x h.  jb_warp_params is the one text of what follows.
 *   1. The inverse matrix a[0..5] in doubles, one operation per statement, nothing contracted.  torchvision's
 *      _get_inverse_affine_matrix(center (cx, cy), angle 0, translate (tx, ty), scale 1, shear (sx, sy) in radians), rot = 0:
 *        A = cos(rot - sy) / cos(sy);  B = -cos(rot - sy) * tan(sx) / cos(sy) - sin(rot);
 *        C = sin(rot - sy) / cos(sy);  D = -sin(rot - sy) * tan(sx) / cos(sy) + cos(rot);
 *        m = [D, -B, 0, -C, A, 0];  m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty);  m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty);
 *        m[2] += cx;  m[5] += cy.
 *      JB_COLOR_SHEAR_X v: sx = radians(degrees(atan((double)v))), sy = 0, centre and translate (0, 0); degrees(x) =
 *        x * (180.0 / pi), radians(x) = x * (pi / 180.0).  JB_COLOR_SHEAR_Y v: sx and sy exchanged.
 *      JB_COLOR_TRANSLATE_X t, t integral with |t| <= 65535: centre (w * 0.5, h * 0.5), translate (t, 0), no shear: exactly
 *        [1, 0, -t, 0, 1, 0].  JB_COLOR_TRANSLATE_Y t: translate (0, t).
 *      JB_COLOR_ROTATE deg: Pillow's Image.rotate(deg, NEAREST): g = -radians(deg mod 360.0) (Python's %: the divisor's sign),
 *        m = [round15(cos g), round15(sin g), 0, round15(-sin g), round15(cos g), 0], round15 = Python's round(x, 15);
 *        c = (w / 2.0, h / 2.0);  m[2] = m[0] * -c.x + m[1] * -c.y + 0, m[5] likewise;  m[2] += c.x, m[5] += c.y.
 *   2. Pillow's two nearest-neighbour paths (Geometry.c).  JB_WARP_SHIFT, when a[1] == 0 and a[3] == 0: only a[0] == 1,
 *      a[4] == 1 and integral a[2], a[5] are accepted (the translations, a zero shear, a rotation by a multiple of 360):
 *      xin = x + (int)a[2], yin = y + (int)a[5]; every other such matrix -- a rotation by 180 is one -- is Pillow's scaling
 *      path with a running double sum: JB_ERR_UNSUPPORTED.  JB_WARP_FIXED for everything else: FIX(v) = FLOOR(v * 65536.0 + 0.5),
 *      FLOOR(v) = v < 0 ? (int)floor(v) : (int)v;  A0 = FIX(a[0]), A1 = FIX(a[1]), A3 = FIX(a[3]), A4 = FIX(a[4]),
 *      A2 = FIX(a[2] + a[0] * 0.5 + a[1] * 0.5), A5 = FIX(a[5] + a[3] * 0.5 + a[4] * 0.5);  in int32, shifts arithmetic:
 *      xin = (A2 + y * A1 + x * A0) >> 16, yin = (A5 + y * A4 + x * A3) >> 16.  The path is taken only when at the corners
 *      (0, 0), (w, 0), (0, h), (w, h) |x * a[0] + y * a[1] + a[2]| < 32768.0 and the same for the second row; otherwise Pillow
 *      goes to a float path: JB_ERR_UNSUPPORTED.
 *   3. out[y][x] = 0 <= xin < w && 0 <= yin < h ? u[yin][xin] : (0, 0, 0), u the view AS IT STANDS when the op is reached.
 * A chain may hold JB_COLOR_WARPS_MAX geometric operations, none of them BEHIND a neighbourhood operation (the filter would be
 * wanted at a gathered position); in front of one, and in front of, behind or between statistics operations they are allowed:
 * the statistics are those of the view as it stands, behind a warp of the warped view with its black pixels. */
enum { JB_COLOR_BRIGHTNESS = 1, JB_COLOR_CONTRAST, JB_COLOR_SATURATION, JB_COLOR_HUE, JB_COLOR_GRAYSCALE, JB_COLOR_SOLARIZE };
enum { JB_COLOR_POSTERIZE = 10, JB_COLOR_INVERT, JB_COLOR_AUTOCONTRAST, JB_COLOR_EQUALIZE };
enum { JB_COLOR_BLUR = 16, JB_COLOR_SHARPNESS };
enum { JB_COLOR_SHEAR_X = 32, JB_COLOR_SHEAR_Y, JB_COLOR_TRANSLATE_X, JB_COLOR_TRANSLATE_Y, JB_COLOR_ROTATE };
enum { JB_COLOR_WARPS_MAX = 2 }; /* geometric operations a chain may hold */
enum { JB_WARP_SHIFT = 0, JB_WARP_FIXED = 1 };
enum { JB_COLOR_OPS_MAX = 8 };
enum { JB_COLOR_STATS_MAX = 2 }; /* statistics operations (contrast, autocontrast, equalize) a chain may hold */
enum { JB_COLOR_BLUR_BOX_MAX = 7 }; /* the largest box radius r the blur kernel's halo is built for */
typedef struct jb_color_op {
  int32_t op;  /* JB_COLOR_* */
  float value; /* the factor, the hue shift, the threshold; 0 for JB_COLOR_GRAYSCALE */
} jb_color_op;
typedef struct jb_color_chain {
  int32_t n_ops, reserved; /* 0..JB_COLOR_OPS_MAX; 0 */
  jb_color_op ops[JB_COLOR_OPS_MAX];
} jb_color_chain; /* 72 bytes */
/* Can the n chains be had?  JB_ERR_NULL for a null array (n > 0); JB_ERR_GEOMETRY for n < 0 and for the first chain with
 * n_ops outside 0..8, reserved != 0, an unknown op, a factor that is not finite or below 0, a hue outside 0..255 or not
 * integral, a threshold outside 0..256 or not integral, or a JB_COLOR_GRAYSCALE value that is not 0; JB_ERR_UNSUPPORTED for
 * the first chain with more than one JB_COLOR_CONTRAST.  Chains are looked at in order, and the first one that fails
 * decides: *bad_index (may be NULL) is its index, -1 when no chain is to blame.  Pure host code.
 * JB_COLOR_BLUR adds, under the same rules (a chain that is wrong both ways is JB_ERR_GEOMETRY): JB_ERR_GEOMETRY for a
 * radius that is not finite or below 0; JB_ERR_UNSUPPORTED for a box radius above JB_COLOR_BLUR_BOX_MAX, for a second
 * JB_COLOR_BLUR in a chain, and for a JB_COLOR_CONTRAST behind a JB_COLOR_BLUR.
 * The RandAugment operations add, under the same rules: JB_ERR_GEOMETRY for posterize bits outside 0..8 or not integral, a
 * value other than 0 of JB_COLOR_INVERT / _AUTOCONTRAST / _EQUALIZE, a sharpness factor that is not finite or below 0;
 * JB_ERR_UNSUPPORTED for more than JB_COLOR_STATS_MAX statistics operations in a chain, for a second neighbourhood operation
 * (blur or sharpness), and for a statistics operation behind a neighbourhood operation.
 * The geometric operations add, under the same rules: JB_ERR_GEOMETRY for a value that is not finite and for a translation that
 * is not integral or whose absolute value is above 65535; JB_ERR_UNSUPPORTED for more than JB_COLOR_WARPS_MAX geometric
 * operations in a chain and for a geometric operation behind a neighbourhood operation.  jb_color_check does not know the
 * view's size: the two refusals of jb_warp_params that depend on it (a matrix of Pillow's scaling path, one of its float
 * path) come from the entry points, which know w x h (the target size), behind jb_color_check's status, JB_ERR_UNSUPPORTED
 * with the chain's flat index in jb_last_error; in every refusal nothing is launched or written. */
int jb_color_check(const jb_color_chain *chains, int n, int *bad_index);
/* A geometric operation on a view of w x h -> Pillow's path (*mode: JB_WARP_SHIFT or JB_WARP_FIXED) and its six integers:
 * for JB_WARP_SHIFT coef[2] and coef[5] are (int)a[2] and (int)a[5] and the others 0, for JB_WARP_FIXED coef[0..5] are A0..A5
 * (above).  The one text of the coefficients: the host statement and every launch use it, the kernels get the integers and never
 * see a double.  JB_ERR_NULL for a null pointer; JB_ERR_GEOMETRY for an op that is not geometric, for w or h outside 1..65535
 * and for a value that jb_color_check refuses; JB_ERR_UNSUPPORTED for a matrix of Pillow's scaling path (a rotation by 180
 * degrees) or of its float path; in a refusal nothing is written.  Pure host code. */
int jb_warp_params(int op, float value, int32_t w, int32_t h, int32_t *mode, int32_t coef[6]);
/* The table of one channel from its 256 counts: op = JB_COLOR_AUTOCONTRAST or JB_COLOR_EQUALIZE as defined above (a channel
 * that stays unchanged gets the identity); the one text of the two tables: the host statement and the device's table kernel
 * compile it.  JB_ERR_NULL for a null pointer, JB_ERR_GEOMETRY for another op; in a refusal nothing is written.  The counts
 * must add up to less than 2^32 (a view has at most 65535 x 65535 pixels).  Pure host code. */
int jb_color_lut(int op, const uint32_t counts[256], uint8_t lut[256]);
/* Pillow's GaussianBlur radius -> the box radius and the two 8.24 fixed-point weights of one pass (above); the one text that
 * turns a radius into weights: the kernels get the three integers.  JB_ERR_NULL for a null pointer; JB_ERR_GEOMETRY for a
 * radius that is not finite or below 0; JB_ERR_UNSUPPORTED for r > JB_COLOR_BLUR_BOX_MAX; in a refusal nothing is written.
 * Radius 0 gives r = 0, ww = 16777216, fw = 0: the identity.  Pure host code. */
int jb_blur_params(float radius, int32_t *r, uint32_t *ww, uint32_t *fw);
/* The chain on a HOST image of w x h interleaved uint8 pixels (rows in_row_stride / out_row_stride bytes apart, each at
 * least 3 * w; in == out is allowed): the CPU statement of the kernels' arithmetic, through the same csrc/jb_color_core.h.
 * JB_ERR_NULL; JB_ERR_GEOMETRY for w or h outside 1..65535 or a stride below 3 * w; then jb_color_check's status. */
int jb_color_host(const uint8_t *in, int64_t in_row_stride, int32_t w, int32_t h, const jb_color_chain *chain, uint8_t *out,
                  int64_t out_row_stride);
/* Chain i on DEVICE image i of n_images interleaved uint8 images of w x h (rows in_row_stride apart, images
 * in_image_stride; decoded by this library or not), written in format `spec` (NULL: interleaved uint8) at d_out: rows
 * out_row_stride apart (of a plane when planar), planes spec->plane_stride (0: tight), images out_image_stride, as a batch's
 * d_rgb is described.  The outputs must not overlap the inputs.  chains: a HOST array of n_images, read before the call
 * returns.  Launches on `stream` (NULL: the context's): jb_color_mean_kernel where a chain of the launch has a contrast
 * -- integer sums, so the result does not depend on the order of the additions -- then jb_color_apply_kernel, and where a
 * chain has a JB_COLOR_BLUR jb_color_blur_kernel for those views (a 64 x 32 tile with a halo, six passes in LDS), 32 images a
 * launch.  Where a chain has a JB_COLOR_AUTOCONTRAST or _EQUALIZE: jb_color_hist_kernel (integer counts) and
 * jb_color_table_kernel in front of them, one round per statistics operation of the longest chain; where one has a
 * JB_COLOR_SHARPNESS: jb_color_sharp_kernel for those views.  Where a chain of a launch has a geometric operation:
 * jb_color_warp_table_kernel in front (the operations' integers into the stream's scratch), and the launch's kernels are
 * their instantiations whose every pixel load is a gather through the geometric operations in front of the operation
 * concerned; a launch without one runs the kernels without that text.
 * JB_ERR_NULL; JB_ERR_GEOMETRY for n_images < 1, w or h outside 1..65535, strides below one row / one image, a bad spec, or
 * float output that is not aligned to its element size; then jb_color_check's status with the chain's index in
 * jb_last_error; then JB_ERR_UNSUPPORTED for a geometric operation that jb_warp_params refuses on w x h, with the chain's
 * index.  In every refusal nothing is launched or written. */
int jb_color_device(jb_ctx *ctx, const uint8_t *d_in, int64_t in_row_stride, int64_t in_image_stride, int32_t w, int32_t h,
                    int32_t n_images, const jb_color_chain *chains, void *d_out, int64_t out_row_stride, int64_t out_image_stride,
                    const jb_output_spec *spec, void *stream);
/* The sibling entry point plus `colors`: n_images * K chains parallel to `views`, read before the call returns.
 * DEFINITION: output (i, v) is format(chain[i * K + v](u)), u being what the sibling writes for the same call in
 * JB_FMT_RGB_U8_HWC, mirror included, bit for bit -- under either arithmetic, any orientation, any draft and any filter.
 * colors == NULL is exactly the sibling.  The sibling's refusals come first and are unchanged; then jb_color_check's status
 * with the chain's flat index in jb_last_error, then JB_ERR_UNSUPPORTED for a geometric operation that jb_warp_params refuses
 * on its view's target size (with view groups: its group's), with the same index; in every refusal nothing is launched or written.
 * The resample and filter kernels then write interleaved uint8 into a staging region of the stream's scratch -- counted
 * towards JPEGBLK_RESIZE_TMP_BYTES when images are packed into sub-batches -- and the two colour kernels read it. */
int jb_blocks_to_rgb_device_views_color(jb_ctx *ctx, const jb_device_batch *batch, const jb_view *views, int views_per_image,
                                        const jb_resize *rs, const jb_color_chain *colors, const jb_output_spec *spec, void *stream);
int jb_blocks_to_rgb_device_view_groups_color(jb_ctx *ctx, const jb_device_batch *batch, const jb_view *views, const jb_view_group *groups,
                                              const jb_view_output *outputs, int n_groups, const jb_color_chain *colors,
                                              const jb_output_spec *spec, void *stream);

/* ---- fit: aspect-preserving targets -- letterbox (pad) and centred crop (cover) ----
 * Every route above that gives a batch one output size STRETCHES its source to the target.  A jb_fit next to the
 * jb_resize says what else to do with a source whose aspect ratio is not the target's.  The SOURCE is the launch's
 * rectangle, or the whole frame when roi == NULL -- under an orientation the oriented frame's, as for every other option:
 * sw x sh at (sx, sy).  The target W x H and the filter are the jb_resize's.  A jb_fit_geometry says what happens:
 * `src` is the rectangle of the frame that is resampled, `inner` the rectangle of the target it lands in.
 * NULL or JB_FIT_STRETCH: src = source, inner = (0, 0, W, H) -- exactly the code paths and bits of the sections above.
 * JB_FIT_PAD (letterbox): Pillow's ImageOps.pad, operation for operation on IEEE doubles without contraction.  With
 * ir = (double)sw / (double)sh and dr = (double)W / (double)H: ir == dr gives the inner size W x H; ir > dr gives dw = W,
 * dh = rint((double)sh / (double)sw * (double)W); else dh = H, dw = rint((double)sw / (double)sh * (double)H); rint rounds
 * halves to even (Python's round).  An extent below 1 is raised to 1 (Pillow raises an error there), one above the
 * target's is cut to it.  Only one axis pads; with d = W - dw (or H - dh) the inner offset on it is rint(d * 0.5) for
 * JB_FIT_CENTER, 0 for JB_FIT_START, d for JB_FIT_END.  src is the source.  The inner rectangle holds what the ordinary
 * route gives for the source at the target dw x dh with the same filter (other than JB_FILTER_AREA:
 * Image.resize((dw, dh), method, box=source)); every other element of the target holds `fill`, converted as the store
 * stage converts a uint8: the byte itself in formats 0 and 1, (float)fill[c] * scale[c] + bias[c] -- two rounded
 * operations, and one conversion to binary16 for f16 -- in formats 2 and 3.
 * JB_FIT_COVER (the evaluation transform's centred crop): integers only, in int64.  sw * H == sh * W: src = source.
 * sw * H > sh * W: the crop is cw x sh, cw = clamp((2 * sh * W + H) / (2 * H), 1, sw), at x offset (sw - cw) / 2 for
 * JB_FIT_CENTER, 0 for JB_FIT_START, sw - cw for JB_FIT_END inside the source; else the same with the axes exchanged.
 * inner = (0, 0, W, H); `fill` is not looked at.  The result is what the ordinary route gives for roi = src.
 * Refusals, behind every one of the sections above and in this order, with nothing launched or written: an unknown
 * mode or anchor, reserved8 or reserved not 0 JB_ERR_GEOMETRY; a mode other than JB_FIT_STRETCH without a target size
 * JB_ERR_STATE; such a mode together with per-image rectangles or views JB_ERR_UNSUPPORTED.  The tap cap and the filter's
 * source window are those of the pair that is resampled -- src to the inner size -- not of the source against W x H.
 * Out of scope: a fit per image under per-image rectangles or views, fractional source boxes (ImageOps.fit's own
 * crop), the inner rectangle of every file of a batch run (ask jb_fit_check with the file's size). */
enum { JB_FIT_STRETCH = 0, JB_FIT_PAD = 1, JB_FIT_COVER = 2 };
enum { JB_FIT_CENTER = 0, JB_FIT_START = 1, JB_FIT_END = 2 };
typedef struct jb_fit {
  int32_t mode, anchor; /* JB_FIT_* */
  uint8_t fill[3];      /* JB_FIT_PAD: R, G, B of the border */
  uint8_t reserved8;    /* 0 */
  int32_t reserved;     /* 0 */
} jb_fit;
typedef struct jb_fit_geometry {
  jb_roi src;   /* what is resampled, in pixels of the (oriented) frame */
  jb_roi inner; /* where it lands, in pixels of the target */
} jb_fit_geometry;
/* jb_filter_check with a fit (NULL: stretch): JB_ERR_NULL for a null descriptor or jb_resize, the descriptor's own
 * errors, the rectangle's, the target's and the filter's, then the fit's (above; no target size is rs->out_w =
 * rs->out_h = 0).  desc is the frame whose coordinates `roi` is in (under an orientation: the oriented frame).  On JB_OK
 * *out (may be NULL) is the geometry.  Pure host code. */
int jb_fit_check(const jb_image_desc *desc, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit, jb_fit_geometry *out);
/* jb_blocks_to_rgb_device_filtered with a fit: d_rgb and its strides describe outputs of out_w x out_h, as there. */
int jb_blocks_to_rgb_device_fit(jb_ctx *ctx, const jb_device_batch *batch, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit,
                                const jb_output_spec *spec, void *stream);
/* jb_decode_memory_filtered / jb_decode_file_filtered with a fit; *width and *height are the target's. */
int jb_decode_memory_fit(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit,
                         const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);
int jb_decode_file_fit(jb_ctx *ctx, const char *path, const jb_roi *roi, const jb_resize *rs, const jb_fit *fit,
                       const jb_output_spec *spec, void **out, int32_t *width, int32_t *height);

/* ---- decoder arithmetic: the reference program's, or libjpeg's bit for bit ----
 * What a full-size decode computes between the coefficients and the uint8 pixels.  JB_ARITH_REFERENCE (the default) is
 * the reference program's: a float AAN IDCT, chroma replicated to the luma grid, float YCbCr -> RGB.  JB_ARITH_LIBJPEG
 * is libjpeg(-turbo)'s default decode -- jidctint.c ("islow"), jdsample.c's "fancy" upsampling, jdcolor.c -- so that the
 * full-size output is, bit for bit, Pillow's Image.open(f).convert("RGB") (and torchvision's and OpenCV's decode), and
 * every output option composes on top of it unchanged: formats 1-3, a rectangle, a target size, per-image rectangles and
 * the filters then give the bits of open -> convert("RGB") -> resize(box=) from the file to the normalised tensor.
 * All arithmetic is integer; >> is an arithmetic shift; clamp is to 0..255.
 *   1. Dequantise and IDCT (CONST_BITS 13, PASS1_BITS 2).  v[k] = coef[k] * q[k], natural order.  A columns pass, then a
 *      rows pass, run one 1-D network on in0..in7:
 *        even:  z1 = (in2 + in6) * 4433;  tmp2 = z1 - in6 * 15137;  tmp3 = z1 + in2 * 6270
 *               tmp0 = (in0 + in4) << 13;  tmp1 = (in0 - in4) << 13
 *               tmp10 = tmp0 + tmp3;  tmp13 = tmp0 - tmp3;  tmp11 = tmp1 + tmp2;  tmp12 = tmp1 - tmp2
 *        odd:   t0 = in7, t1 = in5, t2 = in3, t3 = in1;  z1 = t0 + t3;  z2 = t1 + t2;  z3 = t0 + t2;  z4 = t1 + t3
 *               z5 = (z3 + z4) * 9633;  t0 *= 2446;  t1 *= 16819;  t2 *= 25172;  t3 *= 12299
 *               z1 *= -7373;  z2 *= -20995;  z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5
 *               t0 += z1 + z3;  t1 += z2 + z4;  t2 += z2 + z3;  t3 += z1 + z4
 *        out0/7 = tmp10 +- t3;  out1/6 = tmp11 +- t2;  out2/5 = tmp12 +- t1;  out3/4 = tmp13 +- t0,
 *        each (x + (1 << (n - 1))) >> n with n = 11 after the columns pass and n = 18 after the rows pass.
 *      Sample = clamp(out + 128).
 *   2. Chroma upsampling.  The chroma planes are dw = ceil(W / hs) by dh = ceil(H / vs) samples (a coded block's padding
 *      beyond that is never read), and EVERY neighbour index is clamped to [0, dw - 1] / [0, dh - 1]: that one rule is
 *      libjpeg's first / last column and top / bottom row cases.
 *        4:2:2:  out[2x] = (3 c[x] + c[x-1] + 1) >> 2;  out[2x+1] = (3 c[x] + c[x+1] + 2) >> 2
 *        4:4:0:  row 2y: (3 c[y] + c[y-1] + 1) >> 2;  row 2y+1: (3 c[y] + c[y+1] + 2) >> 2
 *        4:2:0:  row 2y+v: s[x] = 3 c[y][x] + c[y + (v ? 1 : -1)][x];
 *                out[2x] = (3 s[x] + s[x-1] + 8) >> 4;  out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4
 *      As in libjpeg, with hs = 2 and dw <= 2 (width <= 4) chroma is plainly replicated in both directions (4:2:0: no
 *      vertical filter either); 4:4:0 has no such exception.
 *   3. Colour, with cb, cr = sample - 128:
 *        R = clamp(y + ((91881 cr + 32768) >> 16));  G = clamp(y + ((-22554 cb - 46802 cr + 32768) >> 16))
 *        B = clamp(y + ((116130 cb + 32768) >> 16))
 *      A grayscale file arrives as 4:4:4 with zero chroma blocks: R = G = B = Y, Pillow's L converted to RGB.
 *   4. A rectangle is a crop of the full decode: with a rectangle, per-image rectangles or a filter's window every pixel
 *      has the bits it has in the full-size decode -- the upsampler's neighbours are the true neighbouring samples, also
 *      in MCUs the rectangle does not touch; clamping happens at the frame's edges only.
 * Domain: the contract holds where every intermediate above fits int32 and the inputs of both passes fit int16 -- the
 * range libjpeg-turbo's SIMD code computes in, and the range every file encoded from 8-bit pixels stays in.  Outside it
 * the output is memory-safe and deterministic and its bits are pinned to nothing (libjpeg's C code, its SIMD code and a
 * plain clamp disagree there).
 * The setting belongs to the context -- of a batch decoder, to the decoder: every device, both sides of submit / collect
 * -- and governs every later call: the device seam in all its variants, jb_blocks_to_rgb / jb_submit / jb_submit_batch,
 * jb_decode_file* / jb_decode_memory*, batch runs and submissions.  It is no part of the output plan: no entry point
 * and no status of the sections above changes.  jb_ctx_set_arithmetic: JB_ERR_NULL for a null context, JB_ERR_GEOMETRY
 * for an unknown value, JB_ERR_STATE while a submission of the context is in flight.  JB_ARITH_LIBJPEG with a scale other
 * than 1 is JB_ERR_UNSUPPORTED -- at the call for a context, at jb_batch_decoder_set_arithmetic / _set_scale for a
 * decoder -- and nothing is written: libjpeg's own scaled decode uses reduced IDCTs, not an area mean, so there is
 * nothing to be exact against.  JPEGBLK_SMALL_GRID, JPEGBLK_ROW_TILING, JPEGBLK_BYTE_STORE and the linear tiling do
 * not apply under JB_ARITH_LIBJPEG; its launches keep uint8 Y, Cb, Cr planes in a scratch of the context, per stream,
 * held to JPEGBLK_RESIZE_TMP_BYTES per launch (one image at the least). */
enum { JB_ARITH_REFERENCE = 0, JB_ARITH_LIBJPEG = 1 };
int jb_ctx_set_arithmetic(jb_ctx *ctx, int arith);
/* the context's arithmetic; a null context: JB_ARITH_REFERENCE */
int jb_ctx_arithmetic(const jb_ctx *ctx);

/* ---- orientation: the Exif Orientation tag applied on the device, in front of every output option ----
 * Let `full` be the full-size uint8 decode [H, W, 3] of the context's arithmetic and oriented = T_o(full), T_o being
 * what Pillow's ImageOps.exif_transpose does for the tag value o (numpy on a = full):
 *   1  a                                  W x H        5  a.transpose(1,0,2)                   H x W
 *   2  a[:, ::-1]                         W x H        6  a.transpose(1,0,2)[:, ::-1]          H x W
 *   3  a[::-1, ::-1]                      W x H        7  a[::-1, ::-1].transpose(1,0,2)       H x W
 *   4  a[::-1]                            W x H        8  a.transpose(1,0,2)[::-1]             H x W
 * Every output option of the sections above then acts on `oriented` exactly as it is defined there for a full-size
 * decode of the oriented size: orientation comes FIRST.  Rectangles (roi, per-image rectangles), the filters' frame
 * extent in_size, the clamping of lo / hi and jb_filter_window are in oriented coordinates; rectangles are checked
 * against the oriented size; buffers, strides, *width and *height are the oriented output's.  The float formats use
 * the planar stage's expression, (float)u8 * scale[c] + bias[c], unfused.  Orientation 1 is bit for bit and launch for
 * launch the behaviour without this section: no scratch, no extra kernel.  Any other value costs one more kernel
 * (jb_orient.hip) and a pass through a scratch of the context (per stream, counted against JPEGBLK_RESIZE_TMP_BYTES).
 * A scale other than 1 together with an orientation other than 1 is JB_ERR_UNSUPPORTED wherever JB_ARITH_LIBJPEG with
 * a scale is, and nothing is uploaded or written: area reduction puts its partial boxes at the right and bottom
 * edges, and those do not commute with a mirror.
 * The setting belongs to the context, as the arithmetic does, and governs every later call.  JB_ORIENT_STORED (1, the
 * default) leaves the pixels as the file stores them; 2..8 are the Exif codes, applied whatever the file says;
 * JB_ORIENT_EXIF takes the value from the file in jb_decode_file* / jb_decode_memory* and the batch decoder
 * (jb_exif_orientation) -- the device seam and jb_blocks_to_rgb / jb_submit / jb_submit_batch have no file, and return
 * JB_ERR_STATE under it with nothing written.  jb_ctx_set_orientation: JB_ERR_NULL for a null context,
 * JB_ERR_GEOMETRY for a value outside 0..8, JB_ERR_STATE while a submission of the context is in flight.
 * Out of scope: XMP tiff:Orientation (which Pillow falls back to when Exif has no tag), Exif spread over several
 * APP1 segments, an orientation per image inside one launch. */
enum { JB_ORIENT_EXIF = 0, JB_ORIENT_STORED = 1 /* 2..8: the Exif codes */ };
int jb_ctx_set_orientation(jb_ctx *ctx, int orientation);
/* the context's orientation; a null context: JB_ORIENT_STORED */
int jb_ctx_orientation(const jb_ctx *ctx);
/* The Exif Orientation of a JPEG byte stream.  Walks the marker segments before the first SOS; in the first APP1 whose
 * payload starts "Exif\0\0" reads the TIFF header (II or MM, 42, the offset of IFD0) and scans IFD0 for tag 0x0112 of
 * type SHORT, count 1.  A value in 1..8 is returned in *orientation; everything else gives 1 with JB_OK: no such
 * segment, no tag, another type or count, a value outside 1..8, an offset or length that leaves the segment.
 * JB_ERR_NULL for a null argument, JB_ERR_FORMAT only when the bytes do not start with SOI.  Never reads outside
 * [jpeg, jpeg + bytes).  XMP is not looked at.  Pure host code. */
int jb_exif_orientation(const uint8_t *jpeg, size_t bytes, int *orientation);
/* The size of T_o(full) for a w x h frame: h x w for 5..8.  JB_ERR_NULL; JB_ERR_GEOMETRY for a size outside 1..65535
 * or an orientation outside 1..8.  Pure host code. */
int jb_oriented_size(int32_t w, int32_t h, int orientation, int32_t *ow, int32_t *oh);
/* The rectangle of the stored w x h frame that the rectangle `oriented` of T_o(full) shows: T_o of that stored
 * rectangle IS the oriented one.  JB_ERR_NULL; JB_ERR_GEOMETRY as jb_oriented_size, or when `oriented` does not lie
 * in the oriented frame.  Pure host code. */
int jb_orient_map_roi(int32_t w, int32_t h, int orientation, const jb_roi *oriented, jb_roi *stored);
/* What a call under `orientation` (1..8) at `scale` with the rectangle `roi` (NULL: none) of the oriented frame would
 * answer before it touches a device: JB_ERR_NULL for a null descriptor, the descriptor's own errors, JB_ERR_GEOMETRY
 * for a scale that is none or an orientation outside 0..8, JB_ERR_UNSUPPORTED for a scale other than 1 with an
 * orientation 2..8 (JB_ORIENT_EXIF passes here: a file decides, and an entry point without one answers JB_ERR_STATE), JB_ERR_GEOMETRY for a rectangle that does not lie in the ORIENTED frame.  Pure host code. */
int jb_orient_check(const jb_image_desc *desc, int orientation, int scale, const jb_roi *roi);

/* ---- draft decode: libjpeg's 1/2, 1/4 and 1/8 reduced decode (scale_denom; Pillow's Image.draft) ----
 * Under JB_ARITH_LIBJPEG a context with draft K in {2, 4, 8} decodes what libjpeg gives with scale_num / scale_denom =
 * 1 / K -- Pillow's im.draft(), which Image.thumbnail() uses too -- bit for bit.  This is NOT scale= (an area mean of
 * the full-size decode): every component gets a reduced IDCT of its own, and in subsampled files chroma is enlarged by
 * the IDCT where libjpeg does so, not by the upsampler.  For a frame W x H with luma factors hs, vs (chroma 1 x 1):
 *   The DRAFT FRAME is ow = ceil(W / K) by oh = ceil(H / K).
 *   Block sizes (jdmaster.c).  A luma block gives S = 8 / K samples per axis.  A chroma block gives Sc: Sc starts at S
 *     and doubles while Sc < 8 and (hs * S) % (2 * Sc) == 0 and (vs * S) % (2 * Sc) == 0.  4:2:0 therefore gets Sc = 2 S
 *     and no upsampling at all; 4:2:2, 4:4:0 and 4:4:4 get Sc = S and keep their upsampler.  What the upsampler still
 *     does is eh = hs * S / Sc, ev = vs * S / Sc (1 or 2).  Grayscale arrives as 4:4:4.
 *   Reduced IDCTs (jidctred.c; CONST_BITS 13, PASS1_BITS 2).  v = coef * q; D(x, n) = (x + (1 << (n - 1))) >> n, an
 *     arithmetic shift; sample = clamp(out + 128).  Size 8 is the islow IDCT of "decoder arithmetic".
 *     Size 4: one 1-D network on in0, in1, in2, in3, in5, in6, in7 (index 4 is never read):
 *         t0 = in0 << 14;  t2 = in2 * 15137 - in6 * 6270;  t10 = t0 + t2;  t12 = t0 - t2
 *         a = -in7 * 1730 + in5 * 11893 - in3 * 17799 + in1 * 8697
 *         b = -in7 * 4176 - in5 * 4926 + in3 * 7373 + in1 * 20995
 *         out0..3 = D(t10 + b, n), D(t12 + a, n), D(t12 - a, n), D(t10 - b, n)
 *       Columns pass over columns 0-3 and 5-7 with n = 12, giving 4 rows; rows pass over those rows with n = 19.
 *     Size 2: the network reads in0, in1, in3, in5, in7:
 *         t10 = in0 << 15;  t = -in7 * 5906 + in5 * 6967 - in3 * 10426 + in1 * 29692
 *         out0, out1 = D(t10 + t, n), D(t10 - t, n)
 *       Columns pass over columns 0, 1, 3, 5, 7 with n = 13; rows pass with n = 20.
 *     Size 1: out = D(v[0], 3).
 *   Planes.  Component c is a plane of its S- (luma) or Sc-sized (chroma) blocks.
 *   Upsampling.  Rule 2 of "decoder arithmetic" with (eh, ev) in the place of (hs, vs) and the draft frame in the place
 *     of W x H: dw = ceil(ow / eh), dh = ceil(oh / ev); the dw <= 2 exception stays.  At K = 8 libjpeg switches fancy
 *     upsampling off (jdsample.c: min_DCT_scaled_size > 1 fails) and chroma is plainly replicated: c[y / ev][x / eh].
 *   Colour.  Rule 3, unchanged.
 *   Domain.  As in "decoder arithmetic": every intermediate in int32, both passes' inputs in int16.
 * Draft comes FIRST: the draft image is "the full-size decode" for everything behind it.  Formats 0-3, a rectangle, a
 * target size with every filter and fit, per-image rectangles and views act on it exactly as their sections define for
 * a frame of ow x oh: rectangles, the filters' in_size, the tap cap, jb_fit_check and jb_filter_window take draft
 * coordinates (hand the pure-host checkers a descriptor with the draft frame's size), and buffers, *width / *height
 * and the batch decoder's widths / heights report the draft frame or the target.  Draft 1 (the default) is bit for bit
 * and launch for launch the behaviour without this section.
 * The setting belongs to the context (of a batch decoder: to the decoder), as the arithmetic and the orientation do,
 * and is no part of the output plan.  jb_ctx_set_draft: JB_ERR_NULL for a null context, JB_ERR_GEOMETRY for a value
 * outside {1, 2, 4, 8}, JB_ERR_STATE while a submission of the context is in flight.  A draft other than 1 under
 * JB_ARITH_REFERENCE, with a scale other than 1, or with an orientation other than JB_ORIENT_STORED (JB_ORIENT_EXIF
 * included) is JB_ERR_UNSUPPORTED -- at the call for a context, at the setters for a decoder (see
 * jb_batch_decoder_set_draft) -- and nothing is launched, uploaded or written.
 * Out of scope: scales M / 8 other than 1/2, 1/4, 1/8; JDCT_IFAST; choosing K from a requested size (Pillow's rule is
 * one line for the caller, and jb_draft_geometry_of gives the sizes). */
int jb_ctx_set_draft(jb_ctx *ctx, int denom);
/* the context's draft; a null context: 1 */
int jb_ctx_draft(const jb_ctx *ctx);
typedef struct jb_draft_geometry {
  int32_t width, height; /* ceil(W / K), ceil(H / K): the DRAFT FRAME */
  int32_t luma_block;    /* S = 8 / K: samples per axis of a luma block */
  int32_t chroma_block;  /* Sc, above */
  int32_t up_h, up_v;    /* eh = hs * S / Sc, ev = vs * S / Sc: what the upsampler still does (1 or 2) */
  int32_t fancy;         /* 1: the triangle filter; 0: plain replication (K = 8) */
  int32_t reserved;
} jb_draft_geometry;
/* The draft geometry of a frame at draft `denom` (1: the frame itself, S = Sc = 8, eh = hs, ev = vs).  JB_ERR_NULL; the
 * descriptor's own errors; JB_ERR_GEOMETRY for a denom outside {1, 2, 4, 8}.  Pure host code. */
int jb_draft_geometry_of(const jb_image_desc *desc, int denom, jb_draft_geometry *out);

/* ---- host front end ("next" rows of the scope table; reference jpeg.cpp:67-446, 826-907,
 *      include/file.hpp, include/huffman.hpp) --------------------------------------------- */
/* Parse a JFIF byte stream and Huffman-decode it into packed int16 blocks in the order
 * described above.  Two-call protocol: with coef == NULL only the headers are parsed and
 * *desc / qtabs are filled (size the buffer with jb_geometry_of); with coef != NULL (capacity
 * coef_cap_bytes) the entropy-coded data is decoded too.
 * What the reference accepts -- baseline, three components, one interleaved scan -- takes the
 * fast path and is integer-exact against the reference's decodeHuffman().  Beyond the reference
 * (it rejects them, jpeg.cpp:69-87, 255-264): progressive frames (SOF2), frames coded in several
 * scans, and grayscale frames, which are delivered as 4:4:4 with all-zero Cb/Cr blocks so that
 * the pixel path yields R = G = B.  Still rejected: luma factors outside {1,2}, chroma not 1x1
 * (JB_ERR_SAMPLING); 12-bit, lossless, hierarchical, arithmetic-coded, 2- or 4-component frames
 * (JB_ERR_UNSUPPORTED). */
int jb_entropy_decode(const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc,
                      uint16_t *qtabs /* 4*64 */, int16_t *coef, size_t coef_cap_bytes);
/* The same with the restart intervals of ONE image (DRI; e.g. the reference's images/img4.jpg)
 * decoded by n_threads host threads: intervals are independent because the DC predictors reset
 * at every restart (reference jpeg.cpp:419-425).  Images without restart markers, or with
 * markers that do not match the frame, take the serial path.  Output is identical. */
int jb_entropy_decode_mt(const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc,
                         uint16_t *qtabs /* 4*64 */, int16_t *coef, size_t coef_cap_bytes,
                         int n_threads);
/* The entropy stage ON THE DEVICE (beyond the reference, whose decodeHuffman() -- jpeg.cpp:405-446 --
 * is serial host code): the host only parses the headers and removes the byte stuffing.  Every restart
 * interval of the scan (the DC predictors reset at each restart, jpeg.cpp:419-425, so intervals are
 * independent; a scan without DRI is one interval) is cut into chunks of 128 bytes, one GPU lane per chunk:
 * the lanes of a workgroup fall into step with the true symbol sequence in a few passes over LDS
 * (self-synchronising decoding), a prefix sum gives every chunk its block index, a writing pass decodes
 * every chunk from its neighbour's final state, stores the coefficients and verifies the chain of chunk
 * states, and a last pass turns the DC differences into DC values (csrc/jb_huff.hip).  The coefficients land
 * in the layout described above.  d_coef is a DEVICE pointer (16-byte aligned, capacity coef_cap_bytes); the
 * result is integer-exact with jb_entropy_decode.  Synchronous.  Takes baseline frames of three components
 * (any of the four sampling layouts) or one component, with up to three Huffman tables of each kind.
 * JB_ERR_UNSUPPORTED: a valid stream this decoder does not take (restart markers that do not match the
 * frame, progressive or multi-scan files, Huffman tables with more long codes than its lookup tables
 * hold) -- use jb_entropy_decode.  JB_ERR_FORMAT: corrupt data, or chunks that did not fall into step
 * (dense adversarial data; one retry with more launches is made first) -- jb_entropy_decode is the authority.
 * The BATCH decoders (jb_decode_batch, jb_batch_decoder_*) take this path by default for every image it
 * accepts (16 chunks = 2 KB of scan or more) and fall back to the host decoder per image for whatever it
 * does not take or flags; JPEGBLK_GPU_HUFFMAN=0 keeps the entropy stage on the host threads (north_star's
 * split), =2 drops the size threshold.  The single-image jb_decode_file / jb_decode_memory take it for files
 * with 128 KB of entropy-coded data or more, where one image's latency is lower on the device (1920x1080
 * 4:4:4: 0.51 ms against 3.9 ms on one host core; 679x451: 0.75-0.95 against 0.7), with
 * JPEGBLK_GPU_HUFFMAN=1 or 2 for every file the device decoder takes, with =0 never. */
int jb_entropy_decode_device(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, jb_image_desc *desc,
                             uint16_t *qtabs /* 4*64, may be NULL */, int16_t *d_coef, size_t coef_cap_bytes);
/* How many images this context has decoded with the entropy stage on the device (through
 * jb_decode_file / jb_decode_memory / a batch decoder): lets callers and tests see which path ran. */
long long jb_ctx_device_entropy_images(const jb_ctx *ctx);
/* decode(path) -> RGB: the reference's whole `Image(path); readJPEG();` surface
 * (jpeg.cpp:797-807, 826-907) minus the X11 sink.  *rgb is malloc'd (tight rows, width*3);
 * release it with jb_free(). */
int jb_decode_file(jb_ctx *ctx, const char *path, uint8_t **rgb, int32_t *width, int32_t *height);
int jb_decode_memory(jb_ctx *ctx, const uint8_t *jpeg, size_t jpeg_bytes, uint8_t **rgb,
                     int32_t *width, int32_t *height);
void jb_free(void *p);
/* Frame descriptor (sampling factors, table ids) of the last image jb_decode_file / jb_decode_memory
 * decoded on this context -- with jb_geometry_of it yields the reference's public fields
 * mcuWidthReal / mcuHeightReal (jpeg.cpp:794-795, computed at :118-125). */
int jb_ctx_last_desc(const jb_ctx *ctx, jb_image_desc *out);

/* Batch of files: the multi-image form of decode(path) (BASELINE.json configs 4-5).  `n_threads`
 * host threads share one context on `device_id` (pinned staging ring) and walk the files
 * i = t, t + n_threads, ...  With JPEGBLK_GPU_HUFFMAN=0 -- north_star's split, "host Huffman on all
 * cores overlapped with device IDCT" -- a thread parses and Huffman-decodes image i into pinned
 * memory, submits it, and collects image i-1 while the device works, so the entropy stage of one
 * image overlaps the copies and the kernel of another, within a thread and across threads.  By
 * default the threads only parse, remove the byte stuffing and pack, and the entropy stage runs on
 * the device too (jb_entropy_decode_device above).  Per file: rgb[i] (malloc'd, tight rows; NULL on
 * failure, release with jb_free), widths[i], heights[i], statuses[i] (a jb_status).  `times`
 * (optional, 4 doubles) receives seconds: wall, summed entropy-decode, summed submit+wait,
 * summed file read.  Returns JB_OK when every file decoded, else the first failing status. */
int jb_decode_batch(int device_id, const char *const *paths, int n_paths, int n_threads,
                    uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times);
/* The same with the shared context and the per-thread pinned buffers kept across runs (creating
 * them -- page pinning above all -- costs milliseconds per thread).  n_threads is capped at the
 * CPUs the process may use (affinity mask and cgroup CPU quota): more entropy threads than that
 * only slow the batch down.  max_*_bytes pre-size every thread's
 * staging (0,0: sized lazily by the first run); a later run with larger images re-sizes. */
typedef struct jb_batch_decoder jb_batch_decoder;
int jb_batch_decoder_create(int device_id, int n_threads, size_t max_coef_bytes, size_t max_rgb_bytes,
                            jb_batch_decoder **out);
int jb_batch_decoder_run(jb_batch_decoder *dec, const char *const *paths, int n_paths, uint8_t **rgb,
                         int32_t *widths, int32_t *heights, int *statuses, double *times);
void jb_batch_decoder_destroy(jb_batch_decoder *dec);
/* Batches in a stream: submit returns at once and the batch runs on the decoder's own host threads; collect
 * waits for it and returns what jb_batch_decoder_run would have (status, and `times` if given).  Up to TWO
 * batches are in flight -- a third submit is refused with JB_ERR_STATE until the older one has been collected --
 * so that the start-up of batch k+1 (reading headers, the first groups' entropy stage and uploads) runs under
 * the tail of batch k (its last kernels and downloads): the seam the reference leaves synchronous per image
 * (jpeg.cpp:785-788) overlapped per batch as well.  Batches alternate between two sides, each with its own
 * host threads, staging and ring on the same device(s); the second side is built by the first submit (tens of
 * milliseconds, as creating a decoder).  Outputs: without an arena as for run (malloc'ed, jb_free); with a
 * pinned arena each side has one of the size given to jb_batch_decoder_set_arena, and with device regions side 0
 * writes into the first half of every region and side 1 into the second -- rgb[i] of batch k stay valid until
 * batch k+2 is submitted.  rgb / widths / heights / statuses must stay valid until the batch is collected (the
 * path strings are copied by submit).  jb_batch_decoder_run / _set_arena / _set_device_output[s] are refused
 * with JB_ERR_STATE while a batch is in flight; jb_batch_decoder_destroy waits for batches still running.
 * One thread at a time calls submit / collect on a decoder. */
int jb_batch_decoder_submit(jb_batch_decoder *dec, const char *const *paths, int n_paths, uint8_t **rgb,
                            int32_t *widths, int32_t *heights, int *statuses, int *ticket);
int jb_batch_decoder_collect(jb_batch_decoder *dec, int ticket, double *times);
/* One decoder over SEVERAL devices of the node (BASELINE.json configs 4-5 as ONE call; images are
 * independent -- reference jpeg.cpp:574-589 touches each block on its own, jpeg.cpp:916-929 decodes
 * one image per process -- so file i goes to device_ids[i % n_devices], no data crosses devices).
 * Per listed device: one shared-context staging ring and an equal share of the n_threads host
 * threads, each bound to the CPUs of that device's NUMA node with its pinned staging allocated
 * there.  A device may be listed more than once (two rings on one GPU).  The handle is used with
 * jb_batch_decoder_run / _set_arena / _destroy like a single-device one; an arena is one pinned
 * allocation shared by all devices. */
int jb_batch_decoder_create_multi(const int *device_ids, int n_devices, int n_threads, size_t max_coef_bytes,
                                  size_t max_rgb_bytes, jb_batch_decoder **out);
/* Images this decoder's current context(s) decoded with the entropy stage on the device (files with
 * restart intervals, see jb_entropy_decode_device); the count restarts when a run re-sizes the ring. */
long long jb_batch_decoder_device_entropy_images(const jb_batch_decoder *dec);
/* Optional pinned output arena owned by the decoder (bytes = 0 releases it).  With an arena,
 * jb_batch_decoder_run places every decoded image in it -- rgb[i] points INTO the arena: do not
 * jb_free it; it stays valid until the next run, set_arena or destroy -- and the device writes the
 * pixels straight to their final place: no per-image allocation, no host copy.  An image that
 * does not fit fails with JB_ERR_CAPACITY.  Without an arena the pixels go through per-thread
 * pinned staging and are copied into malloc'ed buffers (release with jb_free). */
int jb_batch_decoder_set_arena(jb_batch_decoder *dec, size_t bytes);
/* Device-resident output: the decoded images stay in HBM.  `d_base` is DEVICE memory of the
 * decoder's device that the caller owns (hipMalloc, a torch tensor's storage; 256-byte aligned),
 * `bytes` its size; jb_batch_decoder_run then places every image in it like in an arena -- rgb[i]
 * is a DEVICE pointer into the region (tight rows, 3*width bytes each; images decoded in one group
 * lie back to back, so an image's address has no particular alignment), valid until the next run --
 * and the fused kernel writes the pixels straight there:
 * nothing is downloaded, which removes what bounds the host-output forms (the device-to-host link).
 * For consumers that work on the pixels on the GPU.  The run returns when every image is complete
 * in device memory.  A region that is not device memory of the decoder's device (a host pointer,
 * another GPU's memory, a size that reaches beyond the allocation) is refused with JB_ERR_GEOMETRY.
 * (NULL, 0) returns to host output.  A multi-device decoder takes one region per
 * device: jb_batch_decoder_set_device_outputs. */
int jb_batch_decoder_set_device_output(jb_batch_decoder *dec, void *d_base, size_t bytes);
/* The same for a multi-device decoder: one region per listed device, in the order given to
 * jb_batch_decoder_create_multi (d_bases[k] is memory of device_ids[k]); file i lands in the region of
 * device_ids[i % n_devices].  n = 0: host output again. */
int jb_batch_decoder_set_device_outputs(jb_batch_decoder *dec, void *const *d_bases, const size_t *bytes, int n);
/* Output scale of the batch decoder's later runs and submissions (1 = full size, the default; 2, 4, 8: see "scaled
 * output" above).  widths / heights then report the output sizes, and every output form -- malloc'ed, pinned arena,
 * device regions -- holds ceil(W/denom) x ceil(H/denom) pixels per image with tight rows (an arena or region only
 * needs room for the reduced images).  Applies to every device of a multi-device decoder and to both sides of
 * submit / collect.  Refused with JB_ERR_STATE while a batch is in flight. */
int jb_batch_decoder_set_scale(jb_batch_decoder *dec, int denom);
/* Output format of the batch decoder's later runs and submissions (see "tensor-ready output" above; spec->plane_stride
 * must be 0: planes are tight).  Every output form -- malloc'ed, pinned arena, device regions -- then holds
 * jb_output_bytes(width, height, format) per image, rgb[i] pointing at elements of the format's type; with device
 * regions every rgb[i] is aligned to the element size.  Applies to every device of a multi-device decoder and to
 * both sides of submit / collect.  Refused with JB_ERR_STATE while a batch is in flight; a format other than
 * JB_FMT_RGB_U8_HWC while the scale is not 1 (and jb_batch_decoder_set_scale(!= 1) while such a format is set) with
 * JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_output_format(jb_batch_decoder *dec, const jb_output_spec *spec);
/* One rectangle for every image of the batch decoder's later runs and submissions (see "region of interest" above; NULL:
 * whole images again).  widths / heights then report the rectangle's size and every output form holds
 * jb_output_bytes(roi->width, roi->height, format) per image, so files of different sizes give outputs of one size.  A
 * file the rectangle does not fit in gets the per-image status JB_ERR_GEOMETRY and the batch goes on.  Applies to every
 * device of a multi-device decoder and to both sides of submit / collect.  Refused with JB_ERR_STATE while a batch is in
 * flight; with JB_ERR_GEOMETRY when no frame could hold the rectangle; while the scale is not 1 (and
 * jb_batch_decoder_set_scale(!= 1) while a rectangle is set) with JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_roi(jb_batch_decoder *dec, const jb_roi *roi);
/* One output size for every image of the batch decoder's later runs and submissions (see "fixed output size" above;
 * (0, 0): the images' own sizes again).  widths / heights then report out_w / out_h and every output form holds
 * jb_output_bytes(out_w, out_h, format) per image, so files of any size and layout give outputs of one size -- with a
 * rectangle set as well, the rectangle of every file resized (a file it does not fit in gets JB_ERR_GEOMETRY and the
 * batch goes on).  Applies to every device of a multi-device decoder and to both sides of submit / collect.  Refused
 * with JB_ERR_STATE while a batch is in flight; with JB_ERR_GEOMETRY for a size outside 1..65535; while the scale is not
 * 1 (and jb_batch_decoder_set_scale(!= 1) while a target size is set) with JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_resize(jb_batch_decoder *dec, int32_t out_w, int32_t out_h);
/* jb_batch_decoder_run / _submit with a rectangle per file (see "per-image rectangles" above): rois[i] belongs to
 * paths[i], in pixels of that file's frame; files of any size and layout may be mixed.  _submit_crops copies the array,
 * as it copies the path strings.  The target size must have been set (jb_batch_decoder_set_resize): without one the
 * call is refused with JB_ERR_STATE, and so is a decoder-wide rectangle (jb_batch_decoder_set_roi) set at the same time
 * -- two rectangles for one image is a mistake, not a composition.  A file its rectangle does not fit in gets the
 * per-image status JB_ERR_GEOMETRY and the batch goes on.  Every output form works as with set_resize (malloc'ed,
 * pinned arena, device regions), both sides of submit / collect, and multi-device decoders (file i and rectangle i go
 * to the same device).  widths / heights report out_w / out_h.  rois == NULL: JB_ERR_NULL. */
int jb_batch_decoder_run_crops(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_roi *rois, uint8_t **rgb,
                               int32_t *widths, int32_t *heights, int *statuses, double *times);
int jb_batch_decoder_submit_crops(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_roi *rois, uint8_t **rgb,
                                  int32_t *widths, int32_t *heights, int *statuses, int *ticket);
/* _run_crops / _submit_crops with K = views_per_image views per file (see "views" above): views[i * K + v] is view v of
 * paths[i], in pixels of that file's (oriented) frame.  The output arrays keep ONE entry per file: rgb[i] is one buffer
 * holding file i's K outputs back to back, each jb_output_bytes(out_w, out_h, format), tight; widths[i] / heights[i]
 * are a view's size, statuses[i] the file's.  The file stays the unit of everything the decoder does with an output --
 * arena, device region, jb_free, failure -- K times larger: every size check counts K outputs and answers
 * JB_ERR_CAPACITY where it answers today.  A file one of whose views does not fit gets JB_ERR_GEOMETRY and the batch
 * goes on.  The entropy stage runs once per file.  Refused with JB_ERR_UNSUPPORTED while the scale is not 1 or a
 * decoder-wide rectangle is set, with JB_ERR_STATE without a target size, with JB_ERR_GEOMETRY for views_per_image
 * outside 1..16; views == NULL: JB_ERR_NULL.  _submit_views copies the array. */
int jb_batch_decoder_run_views(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views, int views_per_image,
                               uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, double *times);
int jb_batch_decoder_submit_views(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views, int views_per_image,
                                  uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses, int *ticket);
/* _run_views / _submit_views with groups (see "view groups" above): views[i * K + s_g + v] is view v of group g of
 * paths[i].  rgb[i] is the file's BLOCK in the jb_view_groups_bytes layout -- a malloc'ed block, a piece of the arena or a
 * device region alike --, widths[i] / heights[i] report group 0's target, statuses[i] the file's.  The decoder's own target
 * size and filter are not read (none need be set).  The file stays the unit as for views, with the block as its size.
 * A file one of whose views does not fit gets JB_ERR_GEOMETRY and the batch goes on.  The entropy stage runs once per
 * file.  Refused with JB_ERR_UNSUPPORTED while the scale is not 1, a decoder-wide rectangle or a fit other than
 * JB_FIT_STRETCH is set; with JB_ERR_GEOMETRY for counts jb_view_groups_check refuses; views or groups == NULL:
 * JB_ERR_NULL.  _submit_view_groups copies both arrays. */
int jb_batch_decoder_run_view_groups(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views,
                                     const jb_view_group *groups, int n_groups, uint8_t **rgb, int32_t *widths, int32_t *heights,
                                     int *statuses, double *times);
int jb_batch_decoder_submit_view_groups(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views,
                                        const jb_view_group *groups, int n_groups, uint8_t **rgb, int32_t *widths, int32_t *heights,
                                        int *statuses, int *ticket);
/* "Colour chains": jb_batch_decoder_run_views / _submit_views / _run_view_groups / _submit_view_groups plus `colors`, n_paths * K
 * chains parallel to `views` -- colors[i * K + v] is applied to view v of paths[i] as jb_blocks_to_rgb_device_views_color
 * defines it; the layout of the outputs is the sibling's.  colors == NULL is exactly the sibling.  The sibling's call-wide
 * refusals come first; then a bad chain refuses the WHOLE call with jb_color_check's status (the chain's flat index in
 * jb_last_error) before a file is read; a file that fails for its own reasons gets its usual status.  The submit variants
 * copy the chains. */
int jb_batch_decoder_run_views_color(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views, int views_per_image,
                                     const jb_color_chain *colors, uint8_t **rgb, int32_t *widths, int32_t *heights, int *statuses,
                                     double *times);
int jb_batch_decoder_submit_views_color(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views,
                                        int views_per_image, const jb_color_chain *colors, uint8_t **rgb, int32_t *widths, int32_t *heights,
                                        int *statuses, int *ticket);
int jb_batch_decoder_run_view_groups_color(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views,
                                           const jb_view_group *groups, int n_groups, const jb_color_chain *colors, uint8_t **rgb,
                                           int32_t *widths, int32_t *heights, int *statuses, double *times);
int jb_batch_decoder_submit_view_groups_color(jb_batch_decoder *dec, const char *const *paths, int n_paths, const jb_view *views,
                                              const jb_view_group *groups, int n_groups, const jb_color_chain *colors, uint8_t **rgb,
                                              int32_t *widths, int32_t *heights, int *statuses, int *ticket);
/* The filter (JB_FILTER_*; see "resampling filters") of the batch decoder's later runs and submissions: it governs the
 * target size of jb_batch_decoder_set_resize and the per-image rectangles of _run_crops / _submit_crops alike, and is
 * kept while no target size is set (there is then nothing to resample).  A file whose reduction exceeds the tap cap gets
 * the per-image status JB_ERR_UNSUPPORTED and the batch goes on.  Applies to every device of a multi-device decoder and
 * to both sides of submit / collect.  Refused with JB_ERR_STATE while a batch is in flight, with JB_ERR_GEOMETRY for an
 * unknown filter. */
int jb_batch_decoder_set_filter(jb_batch_decoder *dec, int filter);
/* The fit (see "fit"; NULL: stretch again) of the batch decoder's later runs and submissions: what every file does with
 * the target size of jb_batch_decoder_set_resize.  Like the filter it is kept while no target size is set -- a run of
 * files with a mode other than JB_FIT_STRETCH and no target size gives every file the status JB_ERR_STATE.  widths /
 * heights report the target's size; a group is one geometry and so has one inner rectangle.  Applies to every device
 * of a multi-device decoder and to both sides of submit / collect.  Refused with JB_ERR_STATE while a batch is in
 * flight, with JB_ERR_GEOMETRY for an unknown mode or anchor or a reserved field that is not 0; while a mode other than
 * JB_FIT_STRETCH is set, _run_crops / _submit_crops and _run_views / _submit_views are refused with JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_fit(jb_batch_decoder *dec, const jb_fit *fit);
/* The arithmetic (JB_ARITH_*; see "decoder arithmetic") of the batch decoder's later runs and submissions.  Applies to
 * every device of a multi-device decoder and to both sides of submit / collect.  Refused with JB_ERR_STATE while a batch
 * is in flight, with JB_ERR_GEOMETRY for an unknown value, and JB_ARITH_LIBJPEG while the scale is not 1 (and
 * jb_batch_decoder_set_scale(!= 1) under JB_ARITH_LIBJPEG) with JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_arithmetic(jb_batch_decoder *dec, int arith);
/* The orientation (JB_ORIENT_*, 2..8; see "orientation") of the batch decoder's later runs and submissions.  Applies to
 * every device of a multi-device decoder and to both sides of submit / collect.  Under JB_ORIENT_EXIF every file's tag
 * is read when its headers are parsed; a group is one geometry and one orientation.  Reported widths and heights, the
 * decoder's rectangle and the rectangles of run_crops are oriented.  Refused with JB_ERR_STATE while a batch is in
 * flight, with JB_ERR_GEOMETRY for a value outside 0..8, and any value but JB_ORIENT_STORED while the scale is not 1
 * (and jb_batch_decoder_set_scale(!= 1) under such a value) with JB_ERR_UNSUPPORTED. */
int jb_batch_decoder_set_orientation(jb_batch_decoder *dec, int orientation);
/* The draft (1, 2, 4, 8; see "draft decode") of the batch decoder's later runs and submissions.  Applies to every
 * device of a multi-device decoder and to both sides of submit / collect.  Reported widths and heights, the decoder's
 * rectangle and the rectangles and views of run_crops / run_views are the draft frame's.  Refused with JB_ERR_STATE
 * while a batch is in flight, with JB_ERR_GEOMETRY for another value, and a value other than 1 with JB_ERR_UNSUPPORTED
 * under JB_ARITH_REFERENCE, while the scale is not 1 or while the orientation is not JB_ORIENT_STORED -- as
 * jb_batch_decoder_set_arithmetic(JB_ARITH_REFERENCE), _set_scale(!= 1) and _set_orientation(!= JB_ORIENT_STORED) are
 * while the draft is not 1. */
int jb_batch_decoder_set_draft(jb_batch_decoder *dec, int denom);
/* Output sink replacing the reference's X11 window / unused BMP writer (display.hpp,
 * jpeg.cpp:462-509): binary PPM (P6). */
int jb_write_ppm(const char *path, const uint8_t *rgb, int32_t width, int32_t height,
                 int64_t rgb_stride);
/* Replaces Image::saveToBMP / writeBMP (jpeg.cpp:462-509, 809-816): an uncompressed 24-bit
 * Windows BMP (BITMAPINFOHEADER, bottom-up rows padded to 4 bytes, bytes in B,G,R order).  The
 * reference writes the 12-byte OS/2 core header (16-bit sizes) and puts the planes out as
 * R,B,G (jpeg.cpp:497-499) with a padding of width%4 bytes (jpeg.cpp:472), which viewers show
 * with swapped colours or skewed rows; this writer emits what viewers expect. */
int jb_write_bmp(const char *path, const uint8_t *rgb, int32_t width, int32_t height,
                 int64_t rgb_stride);

#ifdef __cplusplus
}
#endif
#endif /* JPEGBLK_H */
