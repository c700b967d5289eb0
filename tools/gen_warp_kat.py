#!/usr/bin/env python3
"""Writes tests/golden/warp_kat.npz: known answers for JB_COLOR_SHEAR_X / _SHEAR_Y / _TRANSLATE_X / _TRANSLATE_Y / _ROTATE
("colour chains", include/jpegblk.h) from PILLOW ITSELF -- Image.transform(size, AFFINE, matrix, NEAREST) with the matrix of
torchvision's _get_inverse_affine_matrix (restated in tests/warp_ref.py: torchvision is not needed) for the shears and the
translations, Image.rotate(deg) for the rotations -- alone, between colour operations, in pairs, in front of and behind the
statistics operations and in front of a blur and a sharpness, on the 61 x 47 image of tests/golden/color_kat.npz.  Before
anything is written, tests/warp_ref.py must give the same bits for every chain: the file then pins both.

    python tools/gen_warp_kat.py            (needs Pillow; the tests that read the file do not)

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
import warp_ref as WR  # noqa: E402
from gen_randaug_kat import pillow_any  # noqa: E402

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS
SX, SY, TX, TY, ROT = WR.SHEAR_X, WR.SHEAR_Y, WR.TRANSLATE_X, WR.TRANSLATE_Y, WR.ROTATE

SHEARS = [0, 0.03, -0.03, 0.27, -0.27, 0.3, 0.99, -0.99]
TRANSLATIONS = [0, 1, -1, 13, -13, -32, 1000]                      # (1000 moves everything out of the view)
ROTATIONS = [1, -1, 30, -30, 44.999, 90, 91, 135, -179, 360]

CHAINS = (
    # each operation alone
    [[(op, v)] for op in (SX, SY) for v in SHEARS] + [[(op, t)] for op in (TX, TY) for t in TRANSLATIONS] + [[(ROT, d)] for d in ROTATIONS] + [
        # each operation between colour operations
        [(B, 1.3), (SX, 0.27), (S, 0.6)], [(H, 40), (SY, -0.3), (I, 0)], [(P, 3), (TX, 13), (Z, 128)], [(G, 0), (TY, -13), (B, 0.7)],
        [(S, 1.4), (ROT, 30), (P, 5)],
        # two geometric operations, both orders
        [(SX, 0.27), (ROT, -30)], [(ROT, -30), (SX, 0.27)], [(TX, 13), (I, 0), (SY, 0.3)], [(SY, 0.3), (I, 0), (TX, 13)], [(ROT, 91), (TY, -1)],
        # in front of and behind each statistics operation (behind: the statistics are the warped view's, black included)
        [(ROT, 30), (C, 1.4)], [(C, 1.4), (ROT, 30)], [(SX, -0.27), (A, 0)], [(A, 0), (SX, -0.27)], [(TY, 13), (E, 0)], [(E, 0), (TY, 13)],
        [(SY, 0.27), (E, 0), (ROT, 44.999), (C, 0.6), (I, 0)],
        # in front of a blur and of a sharpness
        [(ROT, -30), (BLUR, 1.3), (P, 6)], [(B, 1.1), (SX, 0.3), (TX, -13), (SH, 1.7), (Z, 100)],
    ])


def pillow_warp(im, op, value):
    from PIL import Image
    if op == ROT:
        return im.rotate(value)                                     # (NEAREST, no expand, black fill: the defaults)
    return im.transform(im.size, Image.AFFINE, WR.matrix(op, value, im.size[0], im.size[1]), Image.NEAREST)


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
            v = float(chains[i, j, 1])
            im = pillow_warp(im, op, v) if op in WR.WARPS else pillow_any(im, op, v)
        got = np.asarray(im)
        want = WR.apply_chain(u, [(int(op), float(v)) for op, v in chains[i] if int(op) != 0])
        assert np.array_equal(got, want), f"warp_ref differs from Pillow on chain {i}: {chain}"
        outs.append(got)
    path = os.path.join(ROOT, "tests", "golden", "warp_kat.npz")
    np.savez_compressed(path, image=u, chains=chains, out=np.stack(outs), pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__, len(CHAINS), "chains")


if __name__ == "__main__":
    main()
