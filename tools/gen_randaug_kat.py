#!/usr/bin/env python3
"""Writes tests/golden/randaug_kat.npz: known answers for JB_COLOR_POSTERIZE / _INVERT / _AUTOCONTRAST / _EQUALIZE / _SHARPNESS
("colour chains", include/jpegblk.h) from PILLOW ITSELF -- ImageOps.posterize / invert / autocontrast / equalize and
ImageEnhance.Sharpness, what torchvision's PIL backend calls for RandAugment, AutoAugment and TrivialAugmentWide -- alone and
between the older operations, on the 61 x 47 image of tests/golden/color_kat.npz.  Before anything is written,
tests/randaug_ref.py must give the same bits for every chain: the file then pins both.

    python tools/gen_randaug_kat.py            (needs Pillow; the tests that read the file do not)

Keys: image [47, 61, 3] uint8; chains [n, 8, 2] float32 (op, value; op 0 ends a chain); out [n, 47, 61, 3] uint8;
pillow_version."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import blur_ref as BR  # noqa: E402
import color_ref as R  # noqa: E402
import randaug_ref as RA  # noqa: E402
from gen_color_kat import pillow_op  # noqa: E402

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS

CHAINS = [
    # each new operation alone, at the ends of its range
    [(P, 0)], [(P, 8)], [(P, 4)], [(I, 0)], [(A, 0)], [(E, 0)],
    [(SH, 0.0)], [(SH, 0.1)], [(SH, 1.0)], [(SH, 1.9)],
    # each new operation between old ones
    [(B, 1.3), (P, 3), (S, 0.6)], [(H, 40), (I, 0), (B, 0.8)], [(B, 0.5), (A, 0), (Z, 128)], [(S, 1.4), (E, 0), (H, 200)],
    [(G, 0), (SH, 1.45), (Z, 100)], [(B, 0.4), (P, 2), (A, 0), (I, 0)],
    # pairs of statistics operations, both orders
    [(E, 0), (C, 1.4)], [(C, 0.6), (E, 0)], [(A, 0), (C, 1.3)], [(C, 0.5), (A, 0)], [(A, 0), (E, 0)], [(E, 0), (B, 0.7), (A, 0)],
    [(E, 0), (E, 0)], [(B, 0.6), (A, 0), (S, 1.5), (A, 0)],
    # a sharpness and a blur behind statistics operations, operations in front and behind
    [(B, 0.7), (E, 0), (S, 1.2), (C, 1.2), (SH, 1.9), (Z, 77), (P, 5)], [(A, 0), (SH, 0.1), (I, 0)], [(E, 0), (BLUR, 1.3), (P, 6)],
    [(H, 12), (SH, 0.55), (S, 0.3)],
]


def pillow_any(im, op, value):
    from PIL import ImageEnhance, ImageFilter, ImageOps
    if op == P:
        return ImageOps.posterize(im, int(value))
    if op == I:
        return ImageOps.invert(im)
    if op == A:
        return ImageOps.autocontrast(im)
    if op == E:
        return ImageOps.equalize(im)
    if op == SH:
        return ImageEnhance.Sharpness(im).enhance(value)
    if op == BLUR:
        return im.filter(ImageFilter.GaussianBlur(value))
    return pillow_op(im, op, value)


def main():
    import PIL
    from PIL import Image
    u = np.load(os.path.join(ROOT, "tests", "golden", "color_kat.npz"))["image"]
    chains = np.zeros((len(CHAINS), R.OPS_MAX, 2), np.float32)
    outs = []
    for i, chain in enumerate(CHAINS):
        im = Image.fromarray(u)
        for j, (op, value) in enumerate(chain):
            chains[i, j] = op, value
            im = pillow_any(im, op, float(chains[i, j, 1]))
        got = np.asarray(im)
        want = RA.apply_chain(u, [(int(op), float(v)) for op, v in chains[i] if int(op) != 0])
        assert np.array_equal(got, want), f"randaug_ref differs from Pillow on chain {i}: {chain}"
        outs.append(got)
    path = os.path.join(ROOT, "tests", "golden", "randaug_kat.npz")
    np.savez_compressed(path, image=u, chains=chains, out=np.stack(outs), pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
