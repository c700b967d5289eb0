"""NumPy statement of the output formats of include/jpegblk.h ("tensor-ready output"), operation by operation:
uint8 -> float32 (exact), ONE float32 multiply, ONE float32 add, and for f16 one IEEE conversion (round to nearest
even).  Every array operation below rounds once, in float32 / float16 arithmetic, so the tests compare bits."""
import numpy as np

FMT_RGB_U8_HWC, FMT_RGB_U8_CHW, FMT_RGB_F32_CHW, FMT_RGB_F16_CHW = 0, 1, 2, 3

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMAGENET = ([1.0 / (255.0 * s) for s in IMAGENET_STD], [-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)])
# every float32 product u * (1/255) that is inexact, and 126 of them differ between round-toward-zero and round-to-nearest
UNIT = ([1.0 / 255.0] * 3, [0.0] * 3)
# exact in float32; 8 of the 256 products lie exactly halfway between two float16 values
F16_TIES = ([1.0 + 2.0 ** -11] * 3, [0.0] * 3)
PARAM_SETS = {"imagenet": IMAGENET, "unit": UNIT, "f16_ties": F16_TIES}


def to_format(full_hwc_u8, fmt, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """full [H, W, 3] uint8 -> the image in `fmt`: [H, W, 3] uint8 (format 0) or [3, H, W] uint8 / float32 / float16."""
    full = np.asarray(full_hwc_u8)
    assert full.dtype == np.uint8 and full.ndim == 3 and full.shape[2] == 3
    if fmt == FMT_RGB_U8_HWC:
        return full.copy()
    planes = np.ascontiguousarray(full.transpose(2, 0, 1))
    if fmt == FMT_RGB_U8_CHW:
        return planes
    assert fmt in (FMT_RGB_F32_CHW, FMT_RGB_F16_CHW), fmt
    s = np.asarray(scale, np.float32).reshape(3, 1, 1)
    b = np.asarray(bias, np.float32).reshape(3, 1, 1)
    prod = planes.astype(np.float32) * s     # one float32 multiply
    out = prod + b                           # one float32 add
    assert out.dtype == np.float32
    return out if fmt == FMT_RGB_F32_CHW else out.astype(np.float16)


def bits(a):
    """The raw bits of an array (so that -0.0 vs 0.0 or a NaN cannot slip through a comparison)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
