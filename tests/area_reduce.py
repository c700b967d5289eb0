"""The area reduction of include/jpegblk.h ("scaled output"), restated in numpy for the tests:
out[y][x][c] = floor((S + n/2) / n) over the n pixels of the K x K box that lie inside the image."""
import numpy as np


def area_reduce(rgb, k):
    """uint8 [H, W, C] -> uint8 [ceil(H/k), ceil(W/k), C]."""
    rgb = np.asarray(rgb)
    if k == 1:
        return rgb.copy()
    h, w = rgb.shape[:2]
    oh, ow = -(-h // k), -(-w // k)
    pad = np.zeros((oh * k, ow * k) + rgb.shape[2:], np.int64)
    pad[:h, :w] = rgb
    s = pad.reshape(oh, k, ow, k, *rgb.shape[2:]).sum(axis=(1, 3))
    ny = np.minimum(k, h - np.arange(oh) * k)
    nx = np.minimum(k, w - np.arange(ow) * k)
    n = (ny[:, None] * nx[None, :]).reshape(oh, ow, *([1] * (rgb.ndim - 2)))
    return ((s + n // 2) // n).astype(np.uint8)
