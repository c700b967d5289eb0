"""Colour chains for the K views per image of views= / view_groups= with colors= ("colour chains", include/jpegblk.h).

Pure Python over a numpy.random.Generator, like crops.py: the chains of a batch can be drawn before anything is decoded,
and the same generator state gives the same chains.  A chain is a list of (op, value) with op one of the COLOR_* numbers;
[] is the identity.  The procedures are torchvision's (ColorJitter, RandomApply, RandomGrayscale, RandomSolarize) and DINO's
own GaussianBlur class; the generator is numpy's, so the draws are not torch's.  rand_augment_color and
trivial_augment_wide_color are torchvision's RandAugment and TrivialAugmentWide restricted to their colour operations;
rand_augment and trivial_augment_wide draw from the full table of fourteen, the five geometric entries included.

The geometric operations (COLOR_SHEAR_X .. COLOR_ROTATE) are torchvision's F.affine / F.rotate at its default interpolation
(NEAREST) and fill (None: black).  torchvision is not a dependency of this package and was not at hand when they were written:
the matrix formulas (include/jpegblk.h) are RESTATED from torchvision's _get_inverse_affine_matrix and checked against Pillow's
Image.transform(size, AFFINE, matrix, NEAREST) and Image.rotate -- not against torchvision itself.
"""
COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE, COLOR_GRAYSCALE, COLOR_SOLARIZE = 1, 2, 3, 4, 5, 6
COLOR_POSTERIZE, COLOR_INVERT, COLOR_AUTOCONTRAST, COLOR_EQUALIZE = 10, 11, 12, 13
COLOR_BLUR, COLOR_SHARPNESS = 16, 17
COLOR_SHEAR_X, COLOR_SHEAR_Y, COLOR_TRANSLATE_X, COLOR_TRANSLATE_Y, COLOR_ROTATE = 32, 33, 34, 35, 36
COLOR_OPS_MAX, COLOR_STATS_MAX, COLOR_WARPS_MAX = 8, 2, 2


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


# ---- RandAugment / TrivialAugmentWide: the colour operations ----------------------------------------------------------------
def posterize(bits):
    """ImageOps.posterize(im, bits), bits in 0..8 -> a one-operation chain."""
    if int(bits) != bits or not 0 <= bits <= 8:
        raise ValueError("bits must be an integer in 0..8")
    return [(COLOR_POSTERIZE, float(int(bits)))]


def invert():
    """ImageOps.invert(im) -> a one-operation chain."""
    return [(COLOR_INVERT, 0.0)]


def autocontrast():
    """ImageOps.autocontrast(im) (cutoff 0) -> a one-operation chain."""
    return [(COLOR_AUTOCONTRAST, 0.0)]


def equalize():
    """ImageOps.equalize(im) -> a one-operation chain."""
    return [(COLOR_EQUALIZE, 0.0)]


def sharpness(a):
    """ImageEnhance.Sharpness(im).enhance(a), a finite and >= 0 -> a one-operation chain."""
    if not 0 <= a < float("inf"):
        raise ValueError("the sharpness factor must be finite and not negative")
    return [(COLOR_SHARPNESS, float(a))]


def _linspace32(start, end, steps):
    """torch.linspace(start, end, steps) in float32, operation for operation: start + i * step in the lower half, end -
    (steps - 1 - i) * step in the upper"""
    import numpy as np
    f = np.float32
    if steps == 1:
        return [float(f(start))]
    step = f(f(end) - f(start)) / f(steps - 1)
    return [float(f(start) + f(i) * step) if i < steps // 2 else float(f(end) - f(steps - 1 - i) * step) for i in range(steps)]


def _posterize_bits(bins, span):
    """8 - round(arange(bins) / ((bins - 1) / span)) in float32, round half to even (torch's): span 4 or 6"""
    import numpy as np
    if bins == 1:
        return [8]
    return [8 - int(np.round(np.float32(i) / np.float32((bins - 1) / span))) for i in range(bins)]


# the nine colour entries of torchvision's operation tables, in the tables' order
_IDENTITY, _BRIGHTNESS, _COLOR, _CONTRAST, _SHARPNESS, _POSTERIZE, _SOLARIZE, _AUTOCONTRAST, _EQUALIZE = range(9)
_SIGNED = {_BRIGHTNESS: COLOR_BRIGHTNESS, _COLOR: COLOR_SATURATION, _CONTRAST: COLOR_CONTRAST, _SHARPNESS: COLOR_SHARPNESS}
_STATS = (COLOR_CONTRAST, COLOR_AUTOCONTRAST, COLOR_EQUALIZE)


def _takes(chain, op):
    """can `chain` take one more `op` under jb_color_check's rules?"""
    ops = [o for o, _ in chain]
    if len(ops) >= COLOR_OPS_MAX:
        return False
    if op in _STATS:
        if op == COLOR_CONTRAST and COLOR_CONTRAST in ops:
            return False
        return sum(o in _STATS for o in ops) < COLOR_STATS_MAX and COLOR_SHARPNESS not in ops and COLOR_BLUR not in ops
    if op in (COLOR_SHARPNESS, COLOR_BLUR):
        return COLOR_SHARPNESS not in ops and COLOR_BLUR not in ops
    return True


def _augment_entry(index, factor_mag, bits, threshold, negative):
    """one entry of the operation table with its magnitude -> a chain of one operation, or [] for Identity"""
    import math
    if index == _IDENTITY:
        return []
    if index in _SIGNED:
        return [(_SIGNED[index], 1.0 - factor_mag if negative else 1.0 + factor_mag)]
    if index == _POSTERIZE:
        return posterize(bits)
    if index == _SOLARIZE:
        return [(COLOR_SOLARIZE, float(math.ceil(threshold)))]      # v < 178.5 is v < 179
    return autocontrast() if index == _AUTOCONTRAST else equalize()


def rand_augment_color(rng, num_ops=2, magnitude=9, num_magnitude_bins=31):
    """torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins) restricted to the nine colour entries of its operation
    table -- Identity, Brightness, Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize -> a chain of up to
    num_ops operations (Identity adds none).  Per operation: the entry's index (rng.integers(9)), then for Brightness / Color /
    Contrast / Sharpness the sign (rng.integers(2), 1: negative) of the factor 1 +- linspace(0, 0.9, bins)[magnitude].
    Posterize keeps 8 - round(arange(bins) / ((bins - 1) / 4))[magnitude] bits, Solarize's threshold is
    ceil(linspace(255, 0, bins)[magnitude]) (what v < t means for Pillow's float threshold).
    ONE DEPARTURE from torchvision: an operation drawn that the chain so far cannot take -- a second Contrast, a second
    Sharpness, a Contrast / AutoContrast / Equalize behind a Sharpness, a third statistics operation -- is drawn again, index
    and sign.  At num_ops = 2 these are 5 of the 81 ordered pairs."""
    bins = int(num_magnitude_bins)
    if not 0 <= magnitude < bins:
        raise ValueError("magnitude must lie in 0..num_magnitude_bins - 1")
    if not 0 <= num_ops <= COLOR_OPS_MAX:
        raise ValueError("num_ops must lie in 0..8")
    m = int(magnitude)
    factor_mag, bits, threshold = _linspace32(0.0, 0.9, bins)[m], _posterize_bits(bins, 4)[m], _linspace32(255.0, 0.0, bins)[m]
    chain = []
    for _ in range(int(num_ops)):
        while True:
            index = int(rng.integers(9))
            negative = bool(int(rng.integers(2))) if index in _SIGNED else False
            entry = _augment_entry(index, factor_mag, bits, threshold, negative)
            if not entry or _takes(chain, entry[0][0]):
                break
        chain += entry
    return chain


def trivial_augment_wide_color(rng, num_magnitude_bins=31):
    """torchvision's TrivialAugmentWide(num_magnitude_bins) restricted to the nine colour entries of its operation table -> a
    chain of at most one operation.  The draws: the entry's index (rng.integers(9)); for an entry with magnitudes the bin
    (rng.integers(bins)); for Brightness / Color / Contrast / Sharpness the sign (rng.integers(2), 1: negative) of the factor
    1 +- linspace(0, 0.99, bins)[m].  Posterize keeps 8 - round(arange(bins) / ((bins - 1) / 6))[m] bits, Solarize's threshold
    is ceil(linspace(255, 0, bins)[m]).  A chain of one operation can always be had: nothing is drawn again."""
    bins = int(num_magnitude_bins)
    if bins < 1:
        raise ValueError("num_magnitude_bins must be at least 1")
    index = int(rng.integers(9))
    m = int(rng.integers(bins)) if index in _SIGNED or index in (_POSTERIZE, _SOLARIZE) else 0
    negative = bool(int(rng.integers(2))) if index in _SIGNED else False
    return _augment_entry(index, _linspace32(0.0, 0.99, bins)[m], _posterize_bits(bins, 6)[m], _linspace32(255.0, 0.0, bins)[m], negative)


# ---- the geometric operations, and RandAugment / TrivialAugmentWide over the full table -----------------------------------------
_WARPS = (COLOR_SHEAR_X, COLOR_SHEAR_Y, COLOR_TRANSLATE_X, COLOR_TRANSLATE_Y, COLOR_ROTATE)


def _finite(v, what):
    """v as the float32 the chain carries (the helpers' tests see the value the library will), finite there"""
    import ctypes
    v = ctypes.c_float(float(v)).value
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"{what} must be finite in float32")
    return v


def shear_x(v):
    """F.affine(img, angle=0, translate=[0, 0], scale=1, shear=[degrees(atan(v)), 0], NEAREST, centre [0, 0]) -- RandAugment's
    ShearX of magnitude v -> a one-operation chain."""
    return [(COLOR_SHEAR_X, _finite(v, "the shear"))]


def shear_y(v):
    """The same with shear=[0, degrees(atan(v))]: ShearY -> a one-operation chain."""
    return [(COLOR_SHEAR_Y, _finite(v, "the shear"))]


def _translation(t):
    if int(t) != t or abs(t) > 65535:
        raise ValueError("a translation must be an integer in -65535..65535")
    return float(int(t))


def translate_x(t):
    """F.affine(img, angle=0, translate=[t, 0], scale=1, shear=[0, 0], NEAREST): the view moves t pixels to the right, black
    comes in -> a one-operation chain."""
    return [(COLOR_TRANSLATE_X, _translation(t))]


def translate_y(t):
    """The same with translate=[0, t]: t pixels down -> a one-operation chain."""
    return [(COLOR_TRANSLATE_Y, _translation(t))]


def rotate(deg):
    """F.rotate(img, deg, NEAREST) = Image.rotate(deg): counter-clockwise about the centre, the size kept -> a one-operation
    chain; [] for a multiple of 360 (the identity).  ValueError for 180 modulo 360: Pillow takes another path for it (a
    transpose; as a matrix its scaling path), which the chains refuse."""
    deg = _finite(deg, "the angle")
    if deg % 360.0 == 0.0:
        return []
    if deg % 360.0 == 180.0:
        raise ValueError("a rotation by 180 degrees modulo 360 is not a chain operation")
    return [(COLOR_ROTATE, deg)]


# torchvision's operation table in its order
(_T_IDENTITY, _T_SHEAR_X, _T_SHEAR_Y, _T_TRANSLATE_X, _T_TRANSLATE_Y, _T_ROTATE, _T_BRIGHTNESS, _T_COLOR, _T_CONTRAST, _T_SHARPNESS,
 _T_POSTERIZE, _T_SOLARIZE, _T_AUTOCONTRAST, _T_EQUALIZE) = range(14)
_T_COLOR_ENTRY = {_T_IDENTITY: _IDENTITY, _T_BRIGHTNESS: _BRIGHTNESS, _T_COLOR: _COLOR, _T_CONTRAST: _CONTRAST, _T_SHARPNESS: _SHARPNESS,
                  _T_POSTERIZE: _POSTERIZE, _T_SOLARIZE: _SOLARIZE, _T_AUTOCONTRAST: _AUTOCONTRAST, _T_EQUALIZE: _EQUALIZE}
_T_SIGNED = (_T_SHEAR_X, _T_SHEAR_Y, _T_TRANSLATE_X, _T_TRANSLATE_Y, _T_ROTATE, _T_BRIGHTNESS, _T_COLOR, _T_CONTRAST, _T_SHARPNESS)
_T_FIXED = (_T_IDENTITY, _T_AUTOCONTRAST, _T_EQUALIZE)   # the entries without a magnitude


def _takes_any(chain, op):
    """_takes with the geometric operations' rules: COLOR_WARPS_MAX of them, none behind a neighbourhood operation"""
    ops = [o for o, _ in chain]
    if op in _WARPS:
        return len(ops) < COLOR_OPS_MAX and sum(o in _WARPS for o in ops) < COLOR_WARPS_MAX and COLOR_SHARPNESS not in ops and COLOR_BLUR not in ops
    return _takes(chain, op)


def _table_entry(index, shear, tx, ty, angle, factor_mag, bits, threshold, negative):
    """one entry of the full table with its magnitudes -> a chain of at most one operation"""
    sign = -1.0 if negative else 1.0
    if index == _T_SHEAR_X:
        return shear_x(sign * shear)
    if index == _T_SHEAR_Y:
        return shear_y(sign * shear)
    if index == _T_TRANSLATE_X:
        return translate_x(int(sign * tx))          # torchvision's int(): toward zero
    if index == _T_TRANSLATE_Y:
        return translate_y(int(sign * ty))
    if index == _T_ROTATE:
        return rotate(sign * angle)
    return _augment_entry(_T_COLOR_ENTRY[index], factor_mag, bits, threshold, negative)


def rand_augment(rng, width, height, num_ops=2, magnitude=9, num_magnitude_bins=31):
    """torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins) for a view of width x height, over its full table in its
    order -- Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate, Brightness, Color, Contrast, Sharpness, Posterize,
    Solarize, AutoContrast, Equalize -> a chain of up to num_ops operations (Identity and a rotation by 0 add none).  Per
    operation: the entry's index (rng.integers(14)), then for the nine signed entries -- the five geometric ones and Brightness /
    Color / Contrast / Sharpness -- the sign (rng.integers(2), 1: negative).  The magnitudes are float32 linspaces at
    [magnitude]: ShearX / ShearY linspace(0, 0.3), TranslateX linspace(0, 150 / 331 * width) and TranslateY the same with the
    height, both truncated with int(), Rotate linspace(0, 30); the colour entries as rand_augment_color states them.
    ONE DEPARTURE from torchvision, rand_augment_color's: an operation drawn that the chain so far cannot take is drawn again,
    index and sign -- a second Contrast, a second Sharpness, a Contrast / AutoContrast / Equalize behind a Sharpness, a third
    statistics operation, and now a geometric operation behind a Sharpness or a third geometric operation.  At num_ops = 2
    these are 10 of the 196 ordered pairs: rand_augment_color's 5 and Sharpness followed by each of the five geometric entries.
    The refusals that depend on the size cannot occur: width and height must lie in 1..16384 (ValueError), where a shear of at
    most 0.3 and a rotation of at most 30 degrees keep every corner inside Pillow's 16.16 fixed point."""
    bins = int(num_magnitude_bins)
    if not 0 <= magnitude < bins:
        raise ValueError("magnitude must lie in 0..num_magnitude_bins - 1")
    if not 0 <= num_ops <= COLOR_OPS_MAX:
        raise ValueError("num_ops must lie in 0..8")
    if not (1 <= width <= 16384 and 1 <= height <= 16384) or int(width) != width or int(height) != height:
        raise ValueError("width and height must be integers in 1..16384")
    m = int(magnitude)
    shear, angle = _linspace32(0.0, 0.3, bins)[m], _linspace32(0.0, 30.0, bins)[m]
    tx, ty = _linspace32(0.0, 150.0 / 331.0 * int(width), bins)[m], _linspace32(0.0, 150.0 / 331.0 * int(height), bins)[m]
    factor_mag, bits, threshold = _linspace32(0.0, 0.9, bins)[m], _posterize_bits(bins, 4)[m], _linspace32(255.0, 0.0, bins)[m]
    chain = []
    for _ in range(int(num_ops)):
        while True:
            index = int(rng.integers(14))
            negative = bool(int(rng.integers(2))) if index in _T_SIGNED else False
            entry = _table_entry(index, shear, tx, ty, angle, factor_mag, bits, threshold, negative)
            if not entry or _takes_any(chain, entry[0][0]):
                break
        chain += entry
    return chain


def trivial_augment_wide(rng, num_magnitude_bins=31):
    """torchvision's TrivialAugmentWide(num_magnitude_bins) over its full table (rand_augment's order) -> a chain of at most one
    operation.  The draws: the entry's index (rng.integers(14)); for an entry with magnitudes -- all but Identity, AutoContrast
    and Equalize -- the bin (rng.integers(bins)); for the nine signed entries the sign (rng.integers(2), 1: negative).  ShearX /
    ShearY linspace(0, 0.99)[m], TranslateX / TranslateY int(linspace(0, 32)[m]), Rotate linspace(0, 135)[m]; the colour entries
    as trivial_augment_wide_color states them.  No size is needed (every corner of a view up to 16384 a side stays inside
    Pillow's fixed point at these magnitudes) and a chain of one operation can always be had: nothing is drawn again."""
    bins = int(num_magnitude_bins)
    if bins < 1:
        raise ValueError("num_magnitude_bins must be at least 1")
    index = int(rng.integers(14))
    m = int(rng.integers(bins)) if index not in _T_FIXED else 0
    negative = bool(int(rng.integers(2))) if index in _T_SIGNED else False
    t = _linspace32(0.0, 32.0, bins)[m]
    return _table_entry(index, _linspace32(0.0, 0.99, bins)[m], t, t, _linspace32(0.0, 135.0, bins)[m], _linspace32(0.0, 0.99, bins)[m],
                        _posterize_bits(bins, 6)[m], _linspace32(255.0, 0.0, bins)[m], negative)
