#!/usr/bin/env python3
"""Writes tests/golden/color_kat.npz: known answers for the colour chains ("colour chains", include/jpegblk.h) from
PILLOW ITSELF -- ImageEnhance.Brightness / Contrast / Color, the convert("HSV") hue shift as torchvision's PIL backend does
it, convert("L") and ImageOps.solarize -- on a 61 x 47 image with a saturated gradient, a gray ramp and black and white
patches.  Before anything is written, tests/color_ref.py must give the same bits for every chain: the file then pins both.

    python tools/gen_color_kat.py            (needs Pillow; the tests that read the file do not)

Keys: image [47, 61, 3] uint8; chains [n, 8, 2] float32 (op, value; op 0 ends a chain); out [n, 47, 61, 3] uint8;
pillow_version."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_ref as R  # noqa: E402

B, C, S, H, G, Z = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE

CHAINS = [
    [(B, 0.0)], [(B, 1.7)], [(C, 0.6)], [(C, 1.7)], [(S, 0.0)], [(S, 1.7)],           # each op alone at two values
    [(H, 0)], [(H, 1)], [(H, 128)], [(H, 255)],
    [(G, 0)], [(Z, 0)], [(Z, 128)], [(Z, 256)],
    [(B, 1.0), (C, 1.0), (S, 1.0)],                                                    # factor 1: the identity, through the blend
    [(C, 1.4), (B, 0.7), (S, 1.3), (H, 25)],                                           # contrast first,
    [(B, 1.2), (H, 230), (C, 0.8), (S, 0.9)],                                          # in the middle,
    [(S, 1.1), (H, 12), (B, 0.9), (C, 1.25)],                                          # last
    [(B, 1.3), (S, 0.5), (H, 77), (Z, 100), (C, 1.6), (G, 0), (B, 0.8), (Z, 200)],     # 8 operations
    [(G, 0), (S, 1.7)],                                                                # grayscale, then saturation
]


def image():
    h, w = 47, 61
    u = np.zeros((h, w, 3), np.uint8)
    x = np.arange(w)
    for y in range(24):                                   # a saturated gradient: hue along x, value / saturation along y
        hsv = np.stack([(x * 255 // (w - 1)), np.full(w, 255 - 5 * y), np.full(w, 255 - 9 * (y % 12))], -1).astype(np.uint8)
        u[y] = R.hsv_to_rgb(hsv[None])[0]
    for y in range(24, 36):                               # a gray ramp
        u[y] = (x * 255 // (w - 1))[:, None]
    u[36:, :20] = 0                                       # black, white, and a few odd colours
    u[36:, 20:40] = 255
    u[36:, 40:] = np.array([[1, 254, 127], [200, 199, 201], [255, 0, 255]], np.uint8)[np.arange(w - 40) % 3]
    return u


def pillow_op(im, op, value):
    from PIL import Image, ImageEnhance, ImageOps
    if op == B:
        return ImageEnhance.Brightness(im).enhance(value)
    if op == C:
        return ImageEnhance.Contrast(im).enhance(value)
    if op == S:
        return ImageEnhance.Color(im).enhance(value)
    if op == G:
        lum = im.convert("L")
        return Image.merge("RGB", (lum, lum, lum))
    if op == Z:
        return ImageOps.solarize(im, int(value))
    h, s, v = im.convert("HSV").split()                   # torchvision's adjust_hue on a PIL image
    nh = (np.asarray(h).astype(np.int64) + int(value)) & 255
    return Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB")


def main():
    import PIL
    from PIL import Image
    u = image()
    chains = np.zeros((len(CHAINS), R.OPS_MAX, 2), np.float32)
    outs = []
    for i, chain in enumerate(CHAINS):
        im = Image.fromarray(u)
        for j, (op, value) in enumerate(chain):
            chains[i, j] = op, value
            im = pillow_op(im, op, value)
        got = np.asarray(im)
        want = R.apply_chain(u, chain)
        assert np.array_equal(got, want), f"color_ref differs from Pillow on chain {i}: {chain}"
        outs.append(got)
    path = os.path.join(ROOT, "tests", "golden", "color_kat.npz")
    np.savez_compressed(path, image=u, chains=chains, out=np.stack(outs), pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
