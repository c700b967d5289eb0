"""The numpy restatement of the geometric operations of the colour chains ("colour chains", include/jpegblk.h): torchvision's
ShearX / ShearY / TranslateX / TranslateY / Rotate at NEAREST with a black fill, as Pillow computes them.  Written from
torchvision's _get_inverse_affine_matrix, Pillow's Image.rotate and Geometry.c's two nearest-neighbour paths, independently of
csrc/jb_color_core.h: the matrix is Python's own math on Python floats (fp64, one rounding per operation), the gather is whole-
array int64 arithmetic wrapped to int32.

matrix(op, value, w, h) -> the six doubles; params(op, value, w, h) -> (mode, [c0 .. c5]) or raises Unsupported / Geometry;
warp(u, op, value) -> the warped array; apply_chain(u, chain) is randaug_ref.apply_chain plus ops 32..36."""
import math

import numpy as np

import randaug_ref as RA

SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE = 32, 33, 34, 35, 36
WARPS = (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE)
WARPS_MAX = 2
SHIFT, FIXED = 0, 1


class Geometry(ValueError):
    """what the library refuses with JB_ERR_GEOMETRY (-2)"""


class Unsupported(ValueError):
    """what the library refuses with JB_ERR_UNSUPPORTED (-9)"""


def inverse_affine(center, translate, shear):
    """torchvision's _get_inverse_affine_matrix(center, 0, translate, 1, shear) with the shear ALREADY in radians"""
    rot, scale = 0.0, 1.0
    sx, sy = shear
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(deg, w, h):
    """Image.rotate(deg, NEAREST) without expand, center or translate: its matrix"""
    angle = deg % 360.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, m):
        (a, b, c, d, e, f) = m
        return a * x + b * y + c, d * x + e * y + f

    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = transform(-cx, -cy, m)
    m[2] += cx
    m[5] += cy
    return m


def matrix(op, value, w, h):
    v = float(np.float32(value))
    if op not in WARPS or not (1 <= w <= 65535 and 1 <= h <= 65535) or not math.isfinite(v):
        raise Geometry((op, value, w, h))
    if op in (SHEAR_X, SHEAR_Y):
        s = math.radians(math.degrees(math.atan(v)))
        return inverse_affine((0.0, 0.0), (0.0, 0.0), (s, 0.0) if op == SHEAR_X else (0.0, s))
    if op in (TRANSLATE_X, TRANSLATE_Y):
        if v != math.floor(v) or abs(v) > 65535:
            raise Geometry((op, value))
        return inverse_affine((w * 0.5, h * 0.5), (v, 0.0) if op == TRANSLATE_X else (0.0, v), (0.0, 0.0))
    return rotate_matrix(v, w, h)


def _floor_c(v):
    return int(math.floor(v)) if v < 0 else int(v)


def params(op, value, w, h):
    """Pillow's choice between its two nearest-neighbour paths, and the integers of the one taken"""
    a = matrix(op, value, w, h)
    if a[1] == 0 and a[3] == 0:
        if a[0] != 1 or a[4] != 1 or a[2] != math.floor(a[2]) or a[5] != math.floor(a[5]):
            raise Unsupported("Pillow's scaling path: %r" % (a,))
        return SHIFT, [0, 0, int(a[2]), 0, 0, int(a[5])]
    for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
        if not (abs(x * a[0] + y * a[1] + a[2]) < 32768.0 and abs(x * a[3] + y * a[4] + a[5]) < 32768.0):
            raise Unsupported("Pillow's float path: %r" % (a,))

    def fix(v):
        return _floor_c(v * 65536.0 + 0.5)

    return FIXED, [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def positions(mode, c, w, h):
    """(xin, yin, inside) for every output pixel: three [h, w] arrays"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    if mode == SHIFT:
        xin, yin = x + c[2], y + c[5]
    else:
        xin = _wrap32(c[2] + y * c[1] + x * c[0]) >> 16
        yin = _wrap32(c[5] + y * c[4] + x * c[3]) >> 16
    return xin, yin, (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)


def warp(u, op, value):
    h, w = u.shape[:2]
    mode, c = params(op, value, w, h)
    xin, yin, inside = positions(mode, c, w, h)
    out = np.zeros_like(u)
    out[inside] = u[yin[inside], xin[inside]]
    return out


def apply_chain(u, chain):
    u = np.ascontiguousarray(u, dtype=np.uint8)
    for op, value in (chain or []):
        u = warp(u, op, value) if op in WARPS else RA.apply_op(u, op, value)
    return u
