"""Rectangles for the per-image crops of a batch (Context.blocks_to_rgb_device(..., crops=), BatchDecoder.run(..., crops=)),
and the K views per image of views=.

Pure Python over a numpy.random.Generator: the rectangles of a batch can be drawn from the sizes that
entropy_decode(jpeg_bytes, headers_only=True) reports, before anything is decoded.  Under an orientation (ORIENT_EXIF or
2..8) rectangles are in oriented coordinates: draw them from oriented_size(width, height, exif_orientation(jpeg_bytes)).
"""
import math


def random_resized_crop(width, height, rng, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """The usual random-resized-crop rectangle of a width x height image -> (x, y, w, h), always inside the image (it
    passes jb_roi_check).  Ten draws of an area (a uniform share `scale` of the image's) and an aspect ratio w / h
    (log-uniform in `ratio`); the first whose rounded rectangle fits the image is placed uniformly.  When none fits:
    the centre crop of the whole image, its aspect ratio clamped to the ratio bounds.  rng: a numpy.random.Generator;
    the same generator state gives the same rectangle."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("an image is at least 1 x 1")
    area = width * height
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * float(rng.uniform(scale[0], scale[1]))
        aspect = math.exp(float(rng.uniform(log_lo, log_hi)))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            y = int(rng.integers(0, height - h + 1))
            x = int(rng.integers(0, width - w + 1))
            return x, y, w, h
    # the fallback: the whole image, cut to the nearest allowed aspect ratio, centred
    in_ratio = width / height
    if in_ratio < ratio[0]:
        w, h = width, int(round(width / ratio[0]))
    elif in_ratio > ratio[1]:
        w, h = int(round(height * ratio[1])), height
    else:
        w, h = width, height
    w, h = min(max(w, 1), width), min(max(h, 1), height)
    return (width - w) // 2, (height - h) // 2, w, h


def random_views(width, height, rng, k, p_mirror=0.5, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """k views of a width x height image for views= -> [(x, y, w, h, mirror)] * k: RandomResizedCrop followed by
    RandomHorizontalFlip, k times.  Per view the draws of random_resized_crop in its order, then one
    rng.random() < p_mirror; the same generator state gives the same views."""
    views = []
    for _ in range(int(k)):
        x, y, w, h = random_resized_crop(width, height, rng, scale, ratio)
        views.append((x, y, w, h, bool(float(rng.random()) < p_mirror)))
    return views


def random_multicrop(width, height, rng, groups=((2, (0.4, 1.0)), (8, (0.05, 0.4))), p_mirror=0.5, ratio=(3 / 4, 4 / 3)):
    """One row of K views of a width x height image for views= with view_groups= -> [(x, y, w, h, mirror)] * K, group-major:
    the multi-crop of DINO / DINOv2 / iBOT / SwAV -- groups = ((k, (scale_lo, scale_hi)), ...), by default 2 "global" and 8
    "local" crops.  The draws are exactly random_views(width, height, rng, k, p_mirror, scale, ratio) per group, in group order,
    on the same generator."""
    views = []
    for k, scale in groups:
        views += random_views(width, height, rng, k, p_mirror, scale, ratio)
    return views
