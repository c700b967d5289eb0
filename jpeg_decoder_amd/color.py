"""Colour chains for the K views per image of views= / view_groups= with colors= ("colour chains", include/jpegblk.h).

Pure Python over a numpy.random.Generator, like crops.py: the chains of a batch can be drawn before anything is decoded,
and the same generator state gives the same chains.  A chain is a list of (op, value) with op one of the COLOR_* numbers;
[] is the identity.  The procedures are torchvision's (ColorJitter, RandomApply, RandomGrayscale, RandomSolarize) and DINO's
own GaussianBlur class; the generator is numpy's, so the draws are not torch's.
"""
COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE, COLOR_GRAYSCALE, COLOR_SOLARIZE = 1, 2, 3, 4, 5, 6
COLOR_BLUR = 16


def hue_shift(f):
    """A hue factor f in [-0.5, 0.5] -> the COLOR_HUE value d in 0..255: int(f * 255) (truncated toward zero) mod 256, what
    torchvision's uint8 cast of f * 255 gives."""
    return int(float(f) * 255) % 256


def color_jitter(rng, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
    """torchvision's ColorJitter(brightness, contrast, saturation, hue) -> a chain of up to four operations.  The draws, in
    this order: a permutation of the four operations (rng.permutation(4)), then for brightness, contrast and saturation a
    uniform factor in [max(0, 1 - x), 1 + x] each, then for hue a uniform f in [-hue, hue] (hue_shift maps it).  A parameter
    of 0 draws nothing and adds no operation."""
    for name, x in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if x < 0:
            raise ValueError(f"{name} must not be negative")
    if not 0 <= hue <= 0.5:
        raise ValueError("hue must lie in [0, 0.5]")
    order = [int(i) for i in rng.permutation(4)]
    ops = {}
    for i, (op, x) in enumerate(((COLOR_BRIGHTNESS, brightness), (COLOR_CONTRAST, contrast), (COLOR_SATURATION, saturation))):
        if x > 0:
            ops[i] = (op, float(rng.uniform(max(0.0, 1.0 - x), 1.0 + x)))
    if hue > 0:
        ops[3] = (COLOR_HUE, float(hue_shift(rng.uniform(-hue, hue))))
    return [ops[i] for i in order if i in ops]


def random_apply(rng, p, chain):
    """RandomApply([...], p): one rng.random() -> the chain, or [] when the draw is not below p."""
    return list(chain) if float(rng.random()) < p else []


def random_grayscale(rng, p=0.1):
    """RandomGrayscale(p) (three equal channels): one rng.random() -> [(COLOR_GRAYSCALE, 0)] or []."""
    return [(COLOR_GRAYSCALE, 0.0)] if float(rng.random()) < p else []


def random_solarize(rng, p=0.5, threshold=128):
    """RandomSolarize(threshold, p): one rng.random() -> [(COLOR_SOLARIZE, threshold)] or []."""
    return [(COLOR_SOLARIZE, float(int(threshold)))] if float(rng.random()) < p else []


def dino_color(rng, global_view_index=None):
    """The colour part of DINO's augmentation for one view, without the blur: ColorJitter(0.4, 0.4, 0.2, 0.1) with p = 0.8,
    RandomGrayscale(0.2), and for the second global view (global_view_index == 1) Solarize with p = 0.2.
    global_view_index: 0 or 1 for the two global views, None for a local one.  The jitter is drawn whether it is applied
    or not, so every view consumes the same draws but the solarize's."""
    jitter = color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
    chain = random_apply(rng, 0.8, jitter) + random_grayscale(rng, 0.2)
    if global_view_index == 1:
        chain += random_solarize(rng, 0.2)
    return chain


def random_blur(rng, p, radius_min=0.1, radius_max=2.0):
    """DINO's GaussianBlur(p, radius_min, radius_max) -- Pillow's ImageFilter.GaussianBlur with a uniform radius: one
    rng.random() and one rng.uniform(radius_min, radius_max), BOTH always drawn, so every view consumes the same draws
    -> [(COLOR_BLUR, radius)], or [] when the first draw is not below p."""
    if not 0 <= radius_min <= radius_max:
        raise ValueError("0 <= radius_min <= radius_max wanted")
    apply = float(rng.random()) < p
    radius = float(rng.uniform(radius_min, radius_max))
    return [(COLOR_BLUR, radius)] if apply else []


def dino_augment(rng, global_view_index=None):
    """DINO's augmentation behind the crop and the flip for one view, blur included, in the paper's order:
    ColorJitter(0.4, 0.4, 0.2, 0.1) with p = 0.8, RandomGrayscale(0.2), GaussianBlur with p = 1.0 for the first global view
    (global_view_index == 0), 0.1 for the second (1) and 0.5 for a local one (None), and for the second global view Solarize
    with p = 0.2.  The draws are dino_color's, with random_blur's two behind the grayscale's."""
    jitter = color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
    chain = random_apply(rng, 0.8, jitter) + random_grayscale(rng, 0.2)
    chain += random_blur(rng, {0: 1.0, 1: 0.1, None: 0.5}[global_view_index])
    if global_view_index == 1:
        chain += random_solarize(rng, 0.2)
    return chain
