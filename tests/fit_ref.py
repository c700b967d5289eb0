"""NumPy / plain-Python statement of "fit" (include/jpegblk.h) for the tests, written from the header's text and not from
the C code: the geometry of JB_FIT_PAD (Pillow's ImageOps.pad: Python floats are IEEE doubles, round() rounds halves to
even) and of JB_FIT_COVER (integers), and the pixels -- the ordinary resize of `src` to the inner size (pillow_resize_ref
for bilinear / bicubic, resize_ref's area resize for the area filter) pasted on a canvas of the fill colour, then
format_ref's conversion.  tests/test_fit_cpu.py holds it against live Pillow."""
import numpy as np

import format_ref as fr
import pillow_resize_ref as pr
from resize_ref import area_resize

STRETCH, PAD, COVER = 0, 1, 2
CENTER, START, END = 0, 1, 2


def _clamp(v, hi):
    return max(1, min(int(v), hi))


def geometry(source, target, mode, anchor=CENTER):
    """source (sx, sy, sw, sh), target (W, H) -> (src, inner), each (x, y, w, h)"""
    sx, sy, sw, sh = source
    W, H = target
    src, inner = (sx, sy, sw, sh), (0, 0, W, H)
    if mode == PAD:
        ir, dr = sw / sh, W / H
        if ir != dr:
            if ir > dr:
                dh = _clamp(round(sh / sw * W), H)
                d = H - dh
                inner = (0, {CENTER: round(d * 0.5), START: 0, END: d}[anchor], W, dh)
            else:
                dw = _clamp(round(sw / sh * H), W)
                d = W - dw
                inner = ({CENTER: round(d * 0.5), START: 0, END: d}[anchor], 0, dw, H)
    elif mode == COVER:
        if sw * H > sh * W:
            cw = _clamp((2 * sh * W + H) // (2 * H), sw)
            src = (sx + {CENTER: (sw - cw) // 2, START: 0, END: sw - cw}[anchor], sy, cw, sh)
        elif sw * H < sh * W:
            ch = _clamp((2 * sw * H + W) // (2 * W), sh)
            src = (sx, sy + {CENTER: (sh - ch) // 2, START: 0, END: sh - ch}[anchor], sw, ch)
    return src, inner


def _resize(full, rect, size, filt):
    if filt == pr.FILTER_AREA:
        x, y, w, h = rect
        return area_resize(full[y:y + h, x:x + w], size[0], size[1])
    return pr.resize(full, rect, size, filt)


def fit_u8(full, source, target, mode, anchor=CENTER, fill=(0, 0, 0), filt=pr.FILTER_AREA):
    """full [H, W, 3] uint8 (the oriented frame), source (x, y, w, h) or None (the whole frame) -> [target_h, target_w, 3] uint8"""
    full = np.asarray(full)
    if source is None:
        source = (0, 0, full.shape[1], full.shape[0])
    src, (ix, iy, iw, ih) = geometry(source, target, mode, anchor)
    out = np.empty((target[1], target[0], 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    out[iy:iy + ih, ix:ix + iw] = _resize(full, src, (iw, ih), filt)
    return out


def fit(full, source, target, mode, anchor=CENTER, fill=(0, 0, 0), filt=pr.FILTER_AREA, fmt=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    return fr.to_format(fit_u8(full, source, target, mode, anchor, fill, filt), fmt, scale, bias)
