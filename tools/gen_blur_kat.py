#!/usr/bin/env python3
"""Writes tests/golden/blur_kat.npz: known answers for JB_COLOR_BLUR ("colour chains", include/jpegblk.h) from PILLOW
ITSELF -- img.filter(ImageFilter.GaussianBlur(radius)), what torchvision's PIL backend and DINO's GaussianBlur class call --
alone and inside DINO's chains, on the 61 x 47 image of tests/golden/color_kat.npz.  Before anything is written,
tests/blur_ref.py must give the same bits for every chain: the file then pins both.

    python tools/gen_blur_kat.py            (needs Pillow; the tests that read the file do not)

Keys: image [47, 61, 3] uint8; chains [n, 8, 2] float32 (op, value; op 0 ends a chain -- the radii are float32, as Pillow's
C entry point takes them); out [n, 47, 61, 3] uint8; pillow_version."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blur_ref as BR  # noqa: E402
import color_ref as R  # noqa: E402
from gen_color_kat import pillow_op  # noqa: E402

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
ROOT2 = np.float32(np.sqrt(2.0))          # where the box radius r flips from 0 to 1

CHAINS = [
    [(BLUR, 0.1)], [(BLUR, 0.5)], [(BLUR, 1.0)],
    [(BLUR, np.nextafter(ROOT2, np.float32(0)))], [(BLUR, ROOT2)], [(BLUR, np.nextafter(ROOT2, np.float32(2)))],
    [(BLUR, 2.0)], [(BLUR, 3.7)], [(BLUR, 8.0)], [(BLUR, 0.0)],
    # dino_augment's three shapes: the first global view (blur always), the second (solarize), a local one
    [(B, 1.2), (C, 0.8), (S, 1.1), (H, 12), (BLUR, 1.3)],
    [(C, 1.3), (S, 0.9), (H, 240), (B, 0.7), (G, 0), (BLUR, 0.7), (Z, 128)],
    [(G, 0), (BLUR, 1.9)],
    [(BLUR, 1.6), (Z, 128)],
    [(S, 1.2), (B, 1.4), (BLUR, 2.0), (H, 100), (Z, 77), (B, 0.5)],        # ops on both sides, r = 1
    [(C, 0.6), (BLUR, 5.0), (S, 1.5)],                                      # a contrast in front, r = 4
]


def main():
    import PIL
    from PIL import Image, ImageFilter
    u = np.load(os.path.join(ROOT, "tests", "golden", "color_kat.npz"))["image"]
    chains = np.zeros((len(CHAINS), R.OPS_MAX, 2), np.float32)
    outs = []
    for i, chain in enumerate(CHAINS):
        im = Image.fromarray(u)
        for j, (op, value) in enumerate(chain):
            chains[i, j] = op, value
            value = float(chains[i, j, 1])
            im = im.filter(ImageFilter.GaussianBlur(value)) if op == BLUR else pillow_op(im, op, value)
        got = np.asarray(im)
        want = BR.apply_chain(u, [(int(op), float(v)) for op, v in chains[i] if int(op) != 0])
        assert np.array_equal(got, want), f"blur_ref differs from Pillow on chain {i}: {chain}"
        outs.append(got)
    # the box radius does flip across sqrt(2) (the filters on its two sides are close: the flip moves weight from fw to ww)
    assert [BR.params(chains[i, 0, 1])[0] for i in (3, 4, 5)] in ([0, 0, 1], [0, 1, 1])
    path = os.path.join(ROOT, "tests", "golden", "blur_kat.npz")
    np.savez_compressed(path, image=u, chains=chains, out=np.stack(outs), pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
