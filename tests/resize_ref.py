"""The exact area resize of include/jpegblk.h ("fixed output size"), restated in numpy int64 for the tests.  On a common
grid of iw * ow units per axis source column i covers [i * ow, (i + 1) * ow) and output column j covers
[j * iw, (j + 1) * iw); wx[j][i] is the integer length of their overlap; rows the same.  Per channel S = wy @ img @ wx.T
and out = floor((S + floor(D / 2)) / D) with D = iw * ih."""
import numpy as np


def weights(n_in, n_out):
    """int64 [n_out, n_in]: the overlap of output cell j with source cell i on the grid of n_in * n_out units."""
    i = np.arange(n_in, dtype=np.int64)[None, :]
    j = np.arange(n_out, dtype=np.int64)[:, None]
    return np.maximum(np.minimum((i + 1) * n_out, (j + 1) * n_in) - np.maximum(i * n_out, j * n_in), 0)


def area_sums(img_u8, ow, oh):
    """uint8 [ih, iw, C] -> the exact sums S, int64 [oh, ow, C]."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3
    ih, iw = img.shape[:2]
    wx, wy = weights(iw, ow), weights(ih, oh)
    return np.stack([wy @ img[:, :, c].astype(np.int64) @ wx.T for c in range(img.shape[2])], axis=2)


def area_resize(img_u8, ow, oh):
    """uint8 [ih, iw, C] -> uint8 [oh, ow, C]."""
    ih, iw = np.asarray(img_u8).shape[:2]
    d = iw * ih
    return ((area_sums(img_u8, ow, oh) + d // 2) // d).astype(np.uint8)
