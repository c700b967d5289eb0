// warp_host_check.cpp -- "colour chains", the geometric operations: the host text (jb_warp_params, jb_color_host through
// csrc/jb_color_core.h's jbc_gather) as a stand-alone program under AddressSanitizer + UBSan.  Every view lies in a heap buffer of
// EXACTLY its size, input and output, so a gather or a store one byte outside the view is a report; the signed arithmetic of the
// coefficients and of the positions runs under UBSan over sizes from 1 x 1 to the largest and over values up to the largest float.
// It also checks what can be said without a reference: a translation is a shift by -t, a zero shear and a full turn are the
// identity, two quarter turns of a square are a half turn, and a refusal writes nothing.
//
//     make -C tools/fuzz warp_host_check && tools/fuzz/warp_host_check
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../jpeg_decoder_amd/csrc/jb_internal.h"

static std::string g_err;
int jb_fail_(jb_ctx *, int code, const char *msg) {
  g_err = msg ? msg : "";
  return code;
}
extern "C" const char *jb_last_error(const jb_ctx *) { return g_err.c_str(); }

static int g_failed = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      fprintf(stderr, "FAILED: " __VA_ARGS__); \
      fprintf(stderr, " (%s)\n", #cond);     \
      g_failed++;                            \
    }                                        \
  } while (0)

static jb_color_chain chain_of(std::vector<jb_color_op> ops) {
  jb_color_chain c;
  memset(&c, 0, sizeof c);
  c.n_ops = (int32_t)ops.size();
  for (size_t i = 0; i < ops.size() && i < JB_COLOR_OPS_MAX; i++) c.ops[i] = ops[i];
  return c;
}

// the chain on a w x h view in exactly-sized heap buffers; the status, and the result in *out
static int run(int w, int h, const jb_color_chain &c, const std::vector<uint8_t> &in, std::vector<uint8_t> *out) {
  uint8_t *a = (uint8_t *)malloc((size_t)3 * w * h), *b = (uint8_t *)malloc((size_t)3 * w * h);
  memcpy(a, in.data(), (size_t)3 * w * h);
  memset(b, 0x5A, (size_t)3 * w * h);
  const int rc = jb_color_host(a, 3LL * w, w, h, &c, b, 3LL * w);
  out->assign(b, b + (size_t)3 * w * h);
  free(a);
  free(b);
  return rc;
}

int main() {
  const int sizes[][2] = {{1, 1}, {2, 1}, {3, 2}, {7, 13}, {61, 47}, {65, 33}, {257, 5}, {2, 300}, {224, 224}};
  const float shears[] = {0.0f, -0.0f, 0.03f, -0.27f, 0.3f, 0.99f, -0.99f, 7.5f, -300.0f, 1e6f, -3.4e38f};
  const float moves[] = {0.0f, 1.0f, -1.0f, 13.0f, -32.0f, 1000.0f, 65535.0f, -65535.0f};
  const float turns[] = {0.0f, 1.0f, -1.0f, 30.0f, 44.999f, 90.0f, 91.0f, 135.0f, -179.0f, 180.0f, 270.0f, 360.0f, 1e6f, -3.4e38f};
  int n_params = 0, n_refused = 0, n_views = 0;
  // jb_warp_params over every size, the largest included, and every value
  const int more[][2] = {{65535, 65535}, {65535, 1}, {1, 65535}, {32767, 3}, {3, 32768}};
  for (int pass = 0; pass < 2; pass++)
    for (size_t s = 0; s < (pass ? sizeof more : sizeof sizes) / sizeof sizes[0]; s++) {
      const int w = pass ? more[s][0] : sizes[s][0], h = pass ? more[s][1] : sizes[s][1];
      for (int op = JB_COLOR_SHEAR_X; op <= JB_COLOR_ROTATE; op++) {
        const bool move = op == JB_COLOR_TRANSLATE_X || op == JB_COLOR_TRANSLATE_Y;
        const float *v = move ? moves : op == JB_COLOR_ROTATE ? turns : shears;
        const size_t n = move ? sizeof moves / 4 : op == JB_COLOR_ROTATE ? sizeof turns / 4 : sizeof shears / 4;
        for (size_t i = 0; i < n; i++) {
          int32_t mode = 77, coef[6] = {77, 77, 77, 77, 77, 77};
          const int rc = jb_warp_params(op, v[i], w, h, &mode, coef);
          n_params++;
          if (rc != JB_OK) {
            n_refused++;
            CHECK(rc == JB_ERR_UNSUPPORTED && mode == 77 && coef[0] == 77 && coef[5] == 77, "op %d value %g %dx%d: rc %d", op, v[i], w, h, rc);
            continue;
          }
          if (move) {
            const int t = (int)v[i];
            CHECK(mode == JB_WARP_SHIFT && coef[2] == (op == JB_COLOR_TRANSLATE_X ? -t : 0) && coef[5] == (op == JB_COLOR_TRANSLATE_Y ? -t : 0),
                  "translation %d by %d", op, t);
          }
          if (v[i] == 0.0f || (op == JB_COLOR_ROTATE && v[i] == 360.0f)) CHECK(mode == JB_WARP_SHIFT && coef[2] == 0 && coef[5] == 0, "identity of op %d", op);
        }
      }
    }
  // jb_color_host: every operation alone, in pairs, around statistics and in front of the two filters
  for (size_t s = 0; s < sizeof sizes / sizeof sizes[0]; s++) {
    const int w = sizes[s][0], h = sizes[s][1];
    std::vector<uint8_t> in((size_t)3 * w * h), out, out2;
    for (size_t i = 0; i < in.size(); i++) in[i] = (uint8_t)(1 + (i * 2654435761u >> 13) % 255);
    for (int op = JB_COLOR_SHEAR_X; op <= JB_COLOR_ROTATE; op++) {
      const bool move = op == JB_COLOR_TRANSLATE_X || op == JB_COLOR_TRANSLATE_Y;
      const float *v = move ? moves : op == JB_COLOR_ROTATE ? turns : shears;
      const size_t n = move ? sizeof moves / 4 : op == JB_COLOR_ROTATE ? sizeof turns / 4 : sizeof shears / 4;
      for (size_t i = 0; i < n; i++) {
        int32_t mode, coef[6];
        const int want = jb_warp_params(op, v[i], w, h, &mode, coef);
        const int rc = run(w, h, chain_of({{op, v[i]}}), in, &out);
        n_views++;
        CHECK(rc == want, "op %d value %g %dx%d: host %d, params %d", op, v[i], w, h, rc, want);
        if (rc != JB_OK) {
          bool untouched = true;
          for (uint8_t b : out) untouched = untouched && b == 0x5A;
          CHECK(untouched, "op %d value %g %dx%d: a refusal wrote", op, v[i], w, h);
        } else if (mode == JB_WARP_SHIFT) {
          bool ok = true;
          for (int y = 0; y < h && ok; y++)
            for (int x = 0; x < w && ok; x++) {
              const int xi = x + coef[2], yi = y + coef[5];
              const bool inside = xi >= 0 && xi < w && yi >= 0 && yi < h;
              for (int c = 0; c < 3; c++) ok = ok && out[(size_t)3 * (y * w + x) + c] == (inside ? in[(size_t)3 * (yi * w + xi) + c] : 0);
            }
          CHECK(ok, "op %d value %g %dx%d: not the shift", op, v[i], w, h);
        }
      }
    }
    const float r = 30.0f;
    const jb_color_chain mixed[] = {
        chain_of({{JB_COLOR_SHEAR_X, 0.27f}, {JB_COLOR_ROTATE, -r}}),
        chain_of({{JB_COLOR_ROTATE, r}, {JB_COLOR_INVERT, 0.0f}, {JB_COLOR_TRANSLATE_X, -1.0f}}),
        chain_of({{JB_COLOR_ROTATE, r}, {JB_COLOR_CONTRAST, 1.3f}}),
        chain_of({{JB_COLOR_EQUALIZE, 0.0f}, {JB_COLOR_SHEAR_Y, 0.5f}, {JB_COLOR_AUTOCONTRAST, 0.0f}, {JB_COLOR_TRANSLATE_Y, 2.0f}}),
        chain_of({{JB_COLOR_ROTATE, -r}, {JB_COLOR_BLUR, 1.2f}, {JB_COLOR_SOLARIZE, 128.0f}}),
        chain_of({{JB_COLOR_SHEAR_X, 0.3f}, {JB_COLOR_BLUR, 6.0f}}),
        chain_of({{JB_COLOR_AUTOCONTRAST, 0.0f}, {JB_COLOR_TRANSLATE_X, 2.0f}, {JB_COLOR_SHEAR_Y, -0.27f}, {JB_COLOR_SHARPNESS, 1.6f}, {JB_COLOR_INVERT, 0.0f}}),
    };
    for (const jb_color_chain &c : mixed) {
      CHECK(run(w, h, c, in, &out) == JB_OK, "a mixed chain on %dx%d: %s", w, h, g_err.c_str());
      n_views++;
    }
    if (w == h) {  // two quarter turns of a square are its half turn: every pixel, reversed
      CHECK(run(w, h, chain_of({{JB_COLOR_ROTATE, 90.0f}, {JB_COLOR_ROTATE, 90.0f}}), in, &out) == JB_OK, "two quarter turns");
      bool ok = true;
      for (int i = 0; i < w * h; i++)
        for (int c = 0; c < 3; c++) ok = ok && out[(size_t)3 * i + c] == in[(size_t)3 * (w * h - 1 - i) + c];
      CHECK(ok, "two quarter turns of %dx%d are not the half turn", w, h);
    }
  }
  fprintf(stderr, "%d parameter sets (%d refused), %d views, %d failed\n", n_params, n_refused, n_views, g_failed);
  return g_failed ? 1 : 0;
}
