#!/usr/bin/env python3
"""Known-answer vectors of "resampling filters" (include/jpegblk.h) from Pillow itself: writes
tests/golden/pillow_resize_kat.npz -- per case k the frame full_k [H, W, 3] uint8, meta_k = (x, y, w, h, out_w, out_h,
filter) and out_k = Image.fromarray(full).resize((out_w, out_h), BILINEAR / BICUBIC, box=(x, y, x + w, y + h)), and the
Pillow version that computed them -- so that a machine without Pillow still tests against Pillow's own bits
(tests/test_filter_cpu.py).  The frames are seeded noise, or only 0 and 255 (bicubic's overshoot then reaches both clamps).
Run it where Pillow is installed; the file is a few KB."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "pillow_resize_kat.npz")

# (W, H, kind, (x, y, w, h) or None, (out_w, out_h)); every case with both filters
CASES = [(23, 17, "noise", None, (7, 5)),                # reduction, whole frame
         (23, 17, "binary", None, (5, 3)),               # stronger reduction, both clamps
         (23, 17, "noise", (5, 4, 9, 9), (33, 20)),      # enlargement of an interior rectangle
         (23, 17, "binary", (0, 0, 11, 8), (4, 13)),     # top-left corner: reduce x, enlarge y
         (23, 17, "noise", (12, 9, 11, 8), (17, 3)),     # bottom-right corner: enlarge x, reduce y
         (23, 17, "noise", (3, 2, 10, 6), (10, 6)),      # identity
         (23, 17, "binary", (11, 8, 1, 1), (4, 3)),      # a 1 x 1 rectangle
         (23, 17, "noise", (2, 1, 19, 14), (1, 1)),      # a 1 x 1 target
         (40, 9, "binary", (1, 0, 38, 9), (3, 9)),       # a long reduction along x, none along y
         (9, 40, "noise", (0, 3, 9, 36), (9, 5))]        # the same along y


def frame(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def main():
    import PIL
    from PIL import Image
    data = {"pillow_version": np.array(PIL.__version__)}
    k = 0
    for i, (w, h, kind, rect, target) in enumerate(CASES):
        full = frame(w, h, kind, 1000 + i)
        x, y, rw, rh = rect if rect is not None else (0, 0, w, h)
        for filt, resample in ((1, Image.BILINEAR), (2, Image.BICUBIC)):
            out = np.asarray(Image.fromarray(full).resize(target, resample, box=(x, y, x + rw, y + rh)))
            data[f"full_{k}"] = full
            data[f"meta_{k}"] = np.array([x, y, rw, rh, target[0], target[1], filt], np.int32)
            data[f"out_{k}"] = out
            k += 1
    data["n"] = np.array(k)
    np.savez_compressed(OUT, **data)
    print(f"{k} cases from Pillow {PIL.__version__} -> {os.path.normpath(OUT)} ({os.path.getsize(OUT)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
