"""NumPy restatement of "resampling filters" (include/jpegblk.h): Pillow's 8-bit bilinear / bicubic resampling of a
rectangle of a frame, operation by operation -- the weights in Python floats (IEEE doubles, one rounding per operation,
a SEQUENTIAL ww sum in tap order), 22-bit fixed point, int64 sums, a uint8 rounding between the horizontal and the
vertical pass.  tests/test_filter_cpu.py holds it against Pillow's own bits."""
import numpy as np

import format_ref as fr

FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC = 0, 1, 2


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


_F = {FILTER_BILINEAR: (_bilinear, 1.0), FILTER_BICUBIC: (_bicubic, 2.0)}


def axis_weights(filt, in_size, in0, in1, n):
    """-> [(lo, [k_0, k_1, ...]) for every output]: the first source sample and the fixed-point weights of its taps."""
    f, S = _F[filt]
    scale = (in1 - in0) / n
    fs = 1.0 if scale < 1.0 else scale
    sup = S * fs
    inv = 1.0 / fs
    out = []
    for j in range(n):
        center = in0 + (j + 0.5) * scale
        lo = max(int(center - sup + 0.5), 0)          # int() truncates toward zero
        hi = min(int(center + sup + 0.5), in_size)
        w = [f((t + lo - center + 0.5) * inv) for t in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((lo, [int(v * 4194304.0 + 0.5) if v >= 0 else int(v * 4194304.0 - 0.5) for v in w]))
    return out


def axis_window(filt, in_size, in0, in1, n):
    """-> (lo, hi): the union of the outputs' [lo, hi)"""
    ws = axis_weights(filt, in_size, in0, in1, n)
    return min(lo for lo, _ in ws), max(lo + len(k) for lo, k in ws)


def window(filt, W, H, rect, target):
    """-> (x, y, w, h): the pixels of the W x H frame the filter reads for `rect` -> `target` = (ow, oh)"""
    x, y, w, h = rect
    x0, x1 = axis_window(filt, W, x, x + w, target[0])
    y0, y1 = axis_window(filt, H, y, y + h, target[1])
    return x0, y0, x1 - x0, y1 - y0


def _pass(src, weights, clamp="clip"):
    """src [n_in, ...] -> [len(weights), ...]: clip8((2^21 + sum_t k[t] * src[lo + t]) >> 22) along axis 0, in int64.
    clamp (for tests that must tell a missing clamp from a present one; "clip" is the definition): "none" leaves the
    clamp out and returns the int64 values, "wrap" keeps their low 8 bits as a plain uint8 store would."""
    out = np.empty((len(weights),) + src.shape[1:], np.uint8 if clamp != "none" else np.int64)
    s64 = src.astype(np.int64)
    for j, (lo, k) in enumerate(weights):
        acc = np.full(src.shape[1:], 1 << 21, np.int64)
        for t, kt in enumerate(k):
            acc += kt * s64[lo + t]
        assert np.all(np.abs(acc) < 2 ** 31)         # the definition's sum is a signed 32-bit one
        out[j] = np.clip(acc >> 22, 0, 255) if clamp == "clip" else (acc >> 22) & 0xff if clamp == "wrap" else acc >> 22
    return out


def resize(full, rect, target, filt, mid_clamp="clip", out_clamp="clip"):
    """full [H, W, 3] uint8, rect (x, y, w, h) or None (the whole frame), target (ow, oh) -> [oh, ow, 3] uint8.
    mid_clamp / out_clamp: _pass's clamp of the horizontal / the vertical pass -- anything but the default "clip" is
    the WRONG answer of a kernel that lost that clamp (mid_clamp "none": the unclamped int64 goes into the second
    pass; out_clamp "wrap": the low byte is stored), for tests to tell from the right one."""
    full = np.asarray(full)
    assert full.dtype == np.uint8 and full.ndim == 3
    H, W = full.shape[:2]
    x, y, w, h = rect if rect is not None else (0, 0, W, H)
    ow, oh = target
    kx = axis_weights(filt, W, x, x + w, ow)
    ky = axis_weights(filt, H, y, y + h, oh)
    t = _pass(np.ascontiguousarray(full.transpose(1, 0, 2)), kx, mid_clamp).transpose(1, 0, 2)   # every frame row: [H, ow, 3]
    return _pass(np.ascontiguousarray(t), ky, out_clamp)


def resize_rect_clamped(full, rect, target, filt):
    """What a kernel that clamps at the RECTANGLE instead of the frame would compute (crop first, then resize): the wrong
    answer the margin tests must tell from the right one."""
    x, y, w, h = rect
    return resize(full[y:y + h, x:x + w], None, target, filt)


def resize_to_format(full, rect, target, filt, fmt, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    return fr.to_format(resize(full, rect, target, filt), fmt, scale, bias)
