#!/usr/bin/env python3
"""The cases of lj_kernel_check: every file of tests/golden/libjpeg_decode_kat.npz and libjpeg_draft_kat.npz at draft 1, 2,
4, 8, as the coefficients of the host front end, the resolved tables, a few rectangles of the draft frame and the image
Pillow gives (the KATs' own bytes).  Needs the built library (jb.entropy_decode is host code) and no GPU.
usage: lj_kernel_cases.py cases.bin"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rects_of(ow, oh):
    """the whole frame first, then rectangles on and off MCU edges, the frame's last pixel, and a single pixel"""
    out = [(0, 0, ow, oh)]
    for x, y, w, h in ((8, 4, 8, 4), (ow // 3, oh // 3, ow // 2, oh // 2), (ow - 1, oh - 1, 1, 1), (1, 0, ow - 1, 1), (ow // 2, 0, 1, oh)):
        if w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= ow and y + h <= oh and (x, y, w, h) not in out:
            out.append((x, y, w, h))
    return out


def main():
    import jpeg_decoder_amd as jb
    import draft_ref
    import libjpeg_ref
    full = {name: rgb for name, _, rgb in libjpeg_ref.load_kat()}
    n = 0
    with open(sys.argv[1], "wb") as f:
        for name, jpeg, drafts in draft_ref.load_kat():
            desc, q, coef = jb.entropy_decode(jpeg)
            g = jb.geometry_of(desc)
            q3 = jb.resolve_qtabs(desc, q)
            for K in (1, 2, 4, 8):
                if K == 1 and name not in full:
                    continue
                image = full[name] if K == 1 else drafts[K]
                oh, ow = image.shape[:2]
                rects = rects_of(ow, oh)
                f.write(np.array([desc.width, desc.height, desc.hs, desc.vs, K, g.mcus_x, g.mcus_y, len(rects)], np.int32).tobytes())
                f.write(np.array(rects, np.int32).tobytes())
                f.write(np.ascontiguousarray(q3, np.int32).tobytes())
                f.write(np.ascontiguousarray(coef, np.int16).tobytes())
                f.write(np.ascontiguousarray(image, np.uint8).tobytes())
                n += 1
    print(f"{n} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
