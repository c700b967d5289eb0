"""The numpy restatement of the colour chains ("colour chains", include/jpegblk.h): what torchvision's PIL backend computes
for ColorJitter / RandomGrayscale / Solarize on uint8 pixels, operation for operation -- ImageEnhance.Brightness / Contrast /
Color (Image.blend against a degenerate image), the convert("HSV") hue shift, convert("L") and ImageOps.solarize.  Written
from Pillow's definitions, independently of csrc/jb_color_core.h; every float32 step is an np.float32 step.

A chain is a list of (op, value); apply_chain(u, chain) takes and returns an [h, w, 3] uint8 array."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAYSCALE, SOLARIZE = 1, 2, 3, 4, 5, 6
OPS_MAX = 8

F32 = np.float32


def luma(u):
    """convert("L"): (19595 R + 38470 G + 7471 B + 32768) >> 16 -> [h, w] int64"""
    p = u.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def blend(d, v, a):
    """Image.blend(degenerate, image, a) per sample: d, v integer arrays in 0..255 -> uint8"""
    a = F32(a)
    d = np.asarray(d, np.int64)
    v = np.asarray(v, np.int64)
    t = d.astype(F32) + a * (v - d).astype(F32)          # two float32 roundings: the product, then the sum
    if F32(0) <= a <= F32(1):
        return np.trunc(t).astype(np.uint8)
    out = np.trunc(np.clip(t, F32(0), F32(255))).astype(np.uint8)
    out[t <= 0] = 0
    out[t >= 255] = 255
    return out


def contrast_mean(u):
    """ImageEnhance.Contrast's int(mean(L) + 0.5), in integers: (2 S + N) div (2 N)"""
    s, n = int(luma(u).sum()), u.shape[0] * u.shape[1]
    return (2 * s + n) // (2 * n)


def rgb_to_hsv(u):
    p = u.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    mx, mn = p.max(-1), p.min(-1)
    gray = mx == mn
    cr = np.where(gray, 1, mx - mn).astype(F32)
    mxf = np.where(gray, 1, mx).astype(F32)
    s = cr / mxf                                           # float32 divisions, correctly rounded
    rc, gc, bc = (mx - r).astype(F32) / cr, (mx - g).astype(F32) / cr, (mx - b).astype(F32) / cr
    rd, gd, bd = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == mx, bd - gd, np.where(g == mx, 2.0 + rd - bd, 4.0 + gd - rd))
    h = h.astype(F32).astype(np.float64)                   # h is a float variable
    h2 = np.fmod(h / 6.0 + 1.0, 1.0).astype(F32).astype(np.float64)
    hh = np.clip((h2 * 255.0).astype(np.int64), 0, 255)
    ss = np.clip((s * F32(255.0)).astype(np.int64), 0, 255)
    hh[gray] = 0
    ss[gray] = 0
    return np.stack([hh, ss, mx], -1).astype(np.uint8)


def _rnd(x):
    """round half away from zero (x >= 0 here), clipped to 0..255"""
    return np.clip(np.floor(x.astype(np.float64) + 0.5).astype(np.int64), 0, 255)


def hsv_to_rgb(q):
    h, s, v = q[..., 0].astype(F32), q[..., 1].astype(F32), q[..., 2].astype(F32)
    hh = h * F32(6) / F32(255)
    i = np.floor(hh)
    f = hh - i
    fs = s / F32(255)
    one = F32(1)
    p = _rnd(v * (one - fs))
    qq = _rnd(v * (one - fs * f))
    t = _rnd(v * (one - fs * (one - f)))
    vi = q[..., 2].astype(np.int64)
    k = i.astype(np.int64) % 6
    r = np.choose(k, [vi, qq, p, p, t, vi])
    g = np.choose(k, [t, vi, vi, qq, p, p])
    b = np.choose(k, [p, p, t, vi, vi, qq])
    out = np.stack([r, g, b], -1)
    out[q[..., 1] == 0] = vi[q[..., 1] == 0][:, None]
    return out.astype(np.uint8)


def apply_op(u, op, value):
    if op == BRIGHTNESS:
        return blend(0, u, value)
    if op == CONTRAST:
        return blend(contrast_mean(u), u, value)
    if op == SATURATION:
        return blend(luma(u)[..., None], u, value)
    if op == GRAYSCALE:
        return np.repeat(luma(u)[..., None], 3, -1).astype(np.uint8)
    if op == SOLARIZE:
        return np.where(u.astype(np.int64) < int(value), u, 255 - u).astype(np.uint8)
    if op == HUE:
        q = rgb_to_hsv(u)
        q[..., 0] = (q[..., 0].astype(np.int64) + int(value)) & 255
        return hsv_to_rgb(q)
    raise ValueError(f"unknown op {op}")


def apply_chain(u, chain):
    u = np.ascontiguousarray(u, dtype=np.uint8)
    for op, value in (chain or []):
        u = apply_op(u, op, value)
    return u


def cube_slices(bs=(0, 1, 17, 127, 128, 254, 255)):
    """all R, G for the given B: a [256 * len(bs), 256, 3] image"""
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.concatenate([np.stack([r, g, np.full_like(r, b)], -1) for b in bs], 0)


def cube():
    """the whole 2^24 cube as one 4096 x 4096 image"""
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
