"""The numpy restatement of the RandAugment colour operations ("colour chains", include/jpegblk.h): what Pillow's
ImageOps.posterize / invert / autocontrast (cutoff 0) / equalize and ImageEnhance.Sharpness compute on uint8 pixels.  Written
from Pillow's definitions, independently of csrc/jb_color_core.h: the tables come from np.bincount, np.cumsum and Python's own
integers and floats, the SMOOTH filter from whole-array float32 products and sums.

apply_chain(u, chain) is blur_ref.apply_chain plus ops 10..13 and 17."""
import numpy as np

import blur_ref as BR
import color_ref as R

POSTERIZE, INVERT, AUTOCONTRAST, EQUALIZE, SHARPNESS = 10, 11, 12, 13, 17
STATS_MAX = 2
F32 = np.float32


def autocontrast_lut(h):
    """ImageOps.autocontrast's table of one channel from its 256 counts (a list of Python ints): Python floats are fp64"""
    nz = [i for i in range(256) if h[i]]
    lo, hi = (nz[0], nz[-1]) if nz else (0, 0)
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(max(int(ix * scale + offset), 0), 255) for ix in range(256)]


def equalize_lut(h):
    """ImageOps.equalize's table of one channel from its 256 counts (a list of Python ints)"""
    histo = [c for c in h if c]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += h[i]
    return lut


def equalize_overshoots(h):
    """does the unclipped quotient pass 255 for these counts?  (where Pillow's min matters)"""
    histo = [c for c in h if c]
    if len(histo) <= 1 or (sum(histo) - histo[-1]) // 255 == 0:
        return False
    step = (sum(histo) - histo[-1]) // 255
    n, worst = step // 2, 0
    for i in range(256):
        worst = max(worst, n // step)
        n += h[i]
    return worst > 255


def counts(u):
    """the three 256-bin histograms of an [h, w, 3] uint8 array, as lists of Python ints"""
    return [[int(c) for c in np.bincount(u[..., ch].ravel(), minlength=256)] for ch in range(3)]


def by_table(u, make):
    out = np.empty_like(u)
    for ch, h in enumerate(counts(u)):
        out[..., ch] = np.asarray(make(h), np.uint8)[u[..., ch]]
    return out


def smooth(u):
    """ImageFilter.SMOOTH of an [h, w, 3] uint8 array: Filter.c's 3 x 3 in float32, the row below first; the outermost rows
    and columns are copies"""
    out = u.copy()
    h, w = u.shape[:2]
    if h < 3 or w < 3:
        return out
    p = u.astype(F32)
    k1, k5 = F32(1.0) / F32(13.0), F32(5.0) / F32(13.0)
    acc = np.full((h - 2, w - 2, 3), F32(0.5), F32)
    for rows, (ka, kb, kc) in ((slice(2, h), (k1, k1, k1)), (slice(1, h - 1), (k1, k5, k1)), (slice(0, h - 2), (k1, k1, k1))):
        left, mid, right = p[rows, 0:w - 2], p[rows, 1:w - 1], p[rows, 2:w]
        line = (left * ka + mid * kb) + right * kc                # float32 arrays: every product and every sum is rounded
        acc = acc + line
    assert acc.dtype == F32
    s = np.where(acc <= 0, 0, np.where(acc >= 255, 255, np.trunc(acc))).astype(np.uint8)
    out[1:-1, 1:-1] = s
    return out


def sharpen(u, a):
    """ImageEnhance.Sharpness(im).enhance(a): Image.blend(SMOOTH(im), im, a)"""
    return R.blend(smooth(u), u, a)


def apply_op(u, op, value):
    if op == POSTERIZE:
        return u & np.uint8(~((1 << (8 - int(value))) - 1) & 255)
    if op == INVERT:
        return (255 - u).astype(np.uint8)
    if op == AUTOCONTRAST:
        return by_table(u, autocontrast_lut)
    if op == EQUALIZE:
        return by_table(u, equalize_lut)
    if op == SHARPNESS:
        return sharpen(u, value)
    if op == BR.BLUR:
        return BR.gaussian_blur(u, value)
    return R.apply_op(u, op, value)


def apply_chain(u, chain):
    u = np.ascontiguousarray(u, dtype=np.uint8)
    for op, value in (chain or []):
        u = apply_op(u, op, value)
    return u
