// jb_geometry.cpp -- the host-only arithmetic of the ABI (include/jpegblk.h): frame geometry and
// quantisation-table resolution.  No HIP dependency, so the front end can be built and fuzzed on
// a CPU-only toolchain with sanitizers (tools/fuzz/).
#include <cstring>

#include "../../include/jpegblk.h"

extern "C" {

// read_sof's derivations, reference jpeg.cpp:77-80 (block counts) and 110-127 (sampling checks,
// padding of odd block counts when the luma factor is 2)
int jb_geometry_of(const jb_image_desc *d, jb_geometry *g) {
  if (!d || !g) return JB_ERR_NULL;
  if (d->width < 1 || d->height < 1 || d->width > 65535 || d->height > 65535) return JB_ERR_GEOMETRY;
  if ((d->hs != 1 && d->hs != 2) || (d->vs != 1 && d->vs != 2)) return JB_ERR_SAMPLING;
  for (int i = 0; i < 3; i++)
    if (d->qtab_id[i] < 0 || d->qtab_id[i] > 3) return JB_ERR_QTAB;
  memset(g, 0, sizeof *g);
  g->mcu_w = (d->width + 7) / 8;
  g->mcu_h = (d->height + 7) / 8;
  g->mcu_w_real = g->mcu_w + ((d->hs == 2 && (g->mcu_w & 1)) ? 1 : 0);
  g->mcu_h_real = g->mcu_h + ((d->vs == 2 && (g->mcu_h & 1)) ? 1 : 0);
  g->mcus_x = g->mcu_w_real / d->hs;
  g->mcus_y = g->mcu_h_real / d->vs;
  g->blocks_per_mcu = d->hs * d->vs + 2;
  g->n_coded_blocks = (int64_t)g->mcus_x * g->mcus_y * g->blocks_per_mcu;
  g->coef_bytes = g->n_coded_blocks * 128;
  g->rgb_bytes = (int64_t)d->width * d->height * 3;
  return JB_OK;
}

int jb_scaled_size(int32_t width, int32_t height, int denom, int32_t *out_w, int32_t *out_h) {
  if (!out_w || !out_h) return JB_ERR_NULL;
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return JB_ERR_GEOMETRY;
  if (width < 1 || height < 1 || width > 65535 || height > 65535) return JB_ERR_GEOMETRY;
  *out_w = (width + denom - 1) / denom;
  *out_h = (height + denom - 1) / denom;
  return JB_OK;
}

// bytes per element of an output format (0: not a format); internal, shared by jb_api.cpp / jb_frontend.cpp / jb_batch.cpp
int jb_format_esize_(int format) {
  return format == JB_FMT_RGB_U8_HWC || format == JB_FMT_RGB_U8_CHW ? 1 : format == JB_FMT_RGB_F32_CHW ? 4 : format == JB_FMT_RGB_F16_CHW ? 2 : 0;
}

int jb_output_bytes(int32_t width, int32_t height, int format, int64_t *bytes) {
  if (!bytes) return JB_ERR_NULL;
  const int es = jb_format_esize_(format);
  if (es == 0 || width < 1 || height < 1 || width > 65535 || height > 65535) return JB_ERR_GEOMETRY;
  *bytes = 3LL * width * height * es;  // at most 3 * 65535^2 * 4 < 2^36
  return JB_OK;
}

int jb_output_spec_check(const jb_output_spec *s, int32_t height, int64_t row_stride) {
  if (!s) return JB_ERR_NULL;
  if (jb_format_esize_(s->format) == 0 || s->reserved != 0) return JB_ERR_GEOMETRY;
  if (s->format == JB_FMT_RGB_U8_HWC) return JB_OK;  // (the other fields are not looked at)
  if (height < 1 || height > 65535 || row_stride < 1) return JB_ERR_GEOMETRY;
  if (s->plane_stride != 0 && s->plane_stride < row_stride * (int64_t)height) return JB_ERR_GEOMETRY;
  if (s->format != JB_FMT_RGB_U8_CHW)
    for (int c = 0; c < 3; c++) {
      // finite: the exponent field is not all ones (tested on the bits)
      uint32_t a, b;
      memcpy(&a, &s->scale[c], 4);
      memcpy(&b, &s->bias[c], 4);
      if ((a & 0x7f800000u) == 0x7f800000u || (b & 0x7f800000u) == 0x7f800000u) return JB_ERR_GEOMETRY;
    }
  return JB_OK;
}

int jb_resolve_qtabs(const jb_image_desc *d, const uint16_t *qtabs, int32_t *out192) {
  if (!d || !qtabs || !out192) return JB_ERR_NULL;
  for (int c = 0; c < 3; c++) {
    if (d->qtab_id[c] < 0 || d->qtab_id[c] > 3) return JB_ERR_QTAB;
    // the table each component names (reference jpeg.cpp:584), natural order
    for (int i = 0; i < 64; i++) out192[c * 64 + i] = qtabs[d->qtab_id[c] * 64 + i];
  }
  return JB_OK;
}

}  // extern "C"
