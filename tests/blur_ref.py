"""The numpy restatement of JB_COLOR_BLUR ("colour chains", include/jpegblk.h): what Pillow's ImageFilter.GaussianBlur(radius)
computes on uint8 pixels -- BoxBlur.c's three "extended box blur" passes along the rows, then three along the columns, each
rounded to uint8, the edge sample repeated for the input of EVERY pass.  Written from Pillow's definition, independently of
csrc/jb_color_core.h: whole-array window sums from a prefix sum over an edge-padded line, no running sum.

apply_chain(u, chain) is color_ref.apply_chain plus op 16."""
import numpy as np

import color_ref as R

BLUR = 16
BOX_MAX = 7
F32 = np.float32


def box_radius(radius):
    """Pillow's _gaussian_blur_radius(radius, 3) -> the fractional box radius, a float32"""
    radius = F32(radius)
    sigma2 = F32(F32(radius * radius) / F32(3))
    big_l = F32(np.sqrt(12.0 * np.float64(sigma2) + 1.0))
    small_l = F32(np.floor((np.float64(big_l) - 1.0) / 2.0))
    a = F32(F32(F32(2) * small_l + F32(1)) * F32(F32(small_l * F32(small_l + F32(1))) - F32(F32(3) * sigma2)))
    a = F32(a / F32(F32(6) * F32(sigma2 - F32(F32(small_l + F32(1)) * F32(small_l + F32(1))))))
    return F32(small_l + a)


def params(radius):
    """-> (r, ww, fw): the integer box radius and the two 8.24 weights of one pass"""
    fr = box_radius(radius)
    r = int(fr)
    ww = int(F32(F32(16777216) / F32(F32(fr * F32(2)) + F32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(a, r, ww, fw):
    """one pass along the LAST axis of an integer array of samples in 0..255"""
    n = a.shape[-1]
    pad = np.take(a, np.clip(np.arange(-r - 1, n + r + 1), 0, n - 1), axis=-1).astype(np.int64)
    cs = np.concatenate([np.zeros(pad.shape[:-1] + (1,), np.int64), np.cumsum(pad, -1)], -1)
    # pad index of sample x is x + r + 1: the box is pad[x + 1 .. x + 2 r + 1], the sides pad[x] and pad[x + 2 r + 2]
    x = np.arange(n)
    box = cs[..., x + 2 * r + 2] - cs[..., x + 1]
    sides = pad[..., x] + pad[..., x + 2 * r + 2]
    acc = ww * box + fw * sides + (1 << 23)
    assert int(acc.max()) < 1 << 32
    return acc >> 24


def gaussian_blur(u, radius):
    """ImageFilter.GaussianBlur(radius) of an [h, w, 3] (or [h, w]) uint8 array"""
    u = np.ascontiguousarray(u, dtype=np.uint8)
    if box_radius(radius) == 0:
        return u.copy()
    r, ww, fw = params(radius)
    a = np.moveaxis(u.astype(np.int64), 1, -1)      # rows last: [h, 3, w]
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    a = np.moveaxis(a, 0, -1)                       # columns last: [3, w, h]
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    if u.ndim == 2:
        return np.ascontiguousarray(a.T).astype(np.uint8)
    return np.ascontiguousarray(a.transpose(2, 1, 0)).astype(np.uint8)


def apply_chain(u, chain):
    u = np.ascontiguousarray(u, dtype=np.uint8)
    for op, value in (chain or []):
        u = gaussian_blur(u, value) if op == BLUR else R.apply_op(u, op, value)
    return u
