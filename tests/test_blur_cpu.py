"""JB_COLOR_BLUR, host side ("colour chains", include/jpegblk.h): the numpy restatement tests/blur_ref.py against Pillow's
ImageFilter.GaussianBlur where Pillow imports; jb_blur_params against Pillow's measured weights and against blur_ref;
jb_color_host -- the kernel's arithmetic through the same csrc/jb_color_core.h -- against Pillow's recorded answers
(tests/golden/blur_kat.npz, tools/gen_blur_kat.py) and against blur_ref, with ops on both sides and in == out; every new
refusal of jb_color_check; the draws of random_blur and dino_augment.  Everything is bit-exact: no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
from conftest import GOLD

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
SIZES = [(1, 1), (2, 3), (5, 4), (3, 200), (61, 47), (96, 96)]            # (w, h)
ROOT2 = np.float32(np.sqrt(2.0))                                           # the box radius flips from 0 to 1 here
EDGE_RADII = [0.0, float(np.nextafter(ROOT2, np.float32(0))), float(ROOT2), float(np.nextafter(ROOT2, np.float32(2))), 3.7, 8.0]


def radii():
    """200 radii drawn uniformly from [0.1, 2.0], then the edge cases"""
    return [float(x) for x in np.random.default_rng(16).uniform(0.1, 2.0, 200)] + EDGE_RADII


def content(w, h, seed=0):
    """random content with a saturated 0 / 255 half (the right one; of a 1-wide image all of it)"""
    rng = np.random.default_rng(1000 * w + h + seed)
    u = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    u[:, w // 2:] = np.where(rng.random((h, w - w // 2, 3)) < 0.5, 0, 255)
    return u


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    if not os.path.exists(jb.lib_path()):
        jb.build_library()
    return jb


def kat():
    z = np.load(os.path.join(GOLD, "blur_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    return z["image"], chains, z["out"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_reference_matches_pillow(size):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    u = content(*size)
    im = Image.fromarray(u)
    for radius in radii():
        want = np.asarray(im.filter(ImageFilter.GaussianBlur(radius)))
        assert np.array_equal(BR.gaussian_blur(u, radius), want), radius


def test_blur_params(jb):
    table = {0.1: (0, 16721291, 27962), 0.5: (0, 15379114, 699051), 1.0: (0, 11184811, 2796202), 2.0: (1, 4473924, 1677722)}
    for radius, want in table.items():
        assert jb.blur_params(radius) == want == BR.params(radius), radius
    assert abs(float(BR.box_radius(1.0)) - 0.25000003) < 1e-8 and float(BR.box_radius(2.0)) == 1.375
    for radius in radii():
        assert jb.blur_params(radius) == BR.params(radius), radius
    assert jb.blur_params(0.0) == (0, 16777216, 0)
    assert [jb.blur_params(x)[0] for x in EDGE_RADII[1:4]] in ([0, 0, 1], [0, 1, 1])
    assert jb.blur_params(8.0)[0] == 7 == jb.COLOR_BLUR_BOX_MAX and jb.COLOR_BLUR == 16
    for radius, status in ((-0.5, -2), (float("nan"), -2), (float("inf"), -2), (-float("inf"), -2), (9.0, -9), (1e30, -9)):
        with pytest.raises(jb.JbError) as e:
            jb.blur_params(radius)
        assert e.value.status == status, radius
    assert BR.params(9.0)[0] == 8
    L = jb.lib()
    r, ww, fw = ctypes.c_int32(-5), ctypes.c_uint32(5), ctypes.c_uint32(5)
    assert L.jb_blur_params(1.0, None, ctypes.byref(ww), ctypes.byref(fw)) == -1
    assert L.jb_blur_params(1.0, ctypes.byref(r), None, ctypes.byref(fw)) == -1
    assert L.jb_blur_params(1.0, ctypes.byref(r), ctypes.byref(ww), None) == -1
    assert L.jb_blur_params(9.0, ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)) == -9
    assert (r.value, ww.value, fw.value) == (-5, 5, 5)                  # a refusal writes nothing


def test_host_matches_the_known_answers_and_the_reference(jb):
    image, chains, outs = kat()
    assert len(chains) >= 16 and image.shape == (47, 61, 3)
    assert sum(len(c) > 1 for c in chains) >= 4 and any(c[0][0] == C and c[1][0] == BLUR for c in chains)
    for chain, want in zip(chains, outs):
        assert np.array_equal(jb.color_host(image, chain), want), chain    # Pillow's recorded bits
        assert np.array_equal(BR.apply_chain(image, chain), want), chain


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_matches_the_reference(jb, size):
    u = content(*size, seed=7)
    for radius in radii()[:200:8] + EDGE_RADII:
        assert np.array_equal(jb.color_host(u, [(BLUR, radius)]), BR.gaussian_blur(u, radius)), radius
    # ops on both sides of the blur; the contrast's mean is that of the view in front of the blur
    for chain in ([(B, 1.3), (BLUR, 1.1), (Z, 128)], [(S, 0.4), (C, 1.4), (G, 0), (BLUR, 2.0), (H, 37), (B, 0.8)],
                  [(BLUR, 0.3), (S, 1.6)], [(H, 200), (BLUR, 6.0)]):
        assert np.array_equal(jb.color_host(u, chain), BR.apply_chain(u, chain)), chain


def test_host_in_place_and_with_strides(jb):
    w, h = 37, 29
    u = content(w, h, seed=3)
    chain = [(C, 1.2), (BLUR, 1.7), (Z, 100)]
    want = BR.apply_chain(u, chain)
    c = jb.ColorChain.make(chain)
    stride = 3 * w + 5
    buf = np.full((h, stride), 0xA5, np.uint8)
    buf[:, :3 * w] = u.reshape(h, 3 * w)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert jb.lib().jb_color_host(p, stride, w, h, ctypes.byref(c), p, stride) == 0          # in == out
    assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want) and (buf[:, 3 * w:] == 0xA5).all()


def test_blur_refusals(jb):
    """every new refusal, its status and its index, with an old-style bad chain (an unknown op) BEHIND it: the first bad
    chain decides; and jb_color_host, given the bad chain, writes nothing"""
    inf, nan = float("inf"), float("nan")
    good = [(B, 1.2), (C, 0.9), (G, 0), (BLUR, 2.0), (Z, 128)]
    jb.color_check([good, [(BLUR, 0.0)], [(BLUR, 8.0)], [(C, 1.0), (BLUR, 1.0)], None])
    cases = [([(BLUR, -0.1)], -2), ([(BLUR, nan)], -2), ([(BLUR, inf)], -2),
             ([(BLUR, 9.0)], -9),                                          # box radius 8
             ([(BLUR, 1.0), (B, 1.0), (BLUR, 1.0)], -9),                   # two blurs
             ([(BLUR, 1.0), (C, 1.0)], -9),                                # a contrast behind a blur
             ([(BLUR, 1.0), (C, 1.0), (H, 300)], -2),                      # ... together with a bad hue: GEOMETRY
             ([(BLUR, 9.0), (BLUR, -1.0)], -2), ([(BLUR, 9.0), (BLUR, 1.0), (C, 1.0), (C, 1.0)], -9)]
    assert BR.params(9.0)[0] == 8
    u = np.full((4, 5, 3), 9, np.uint8)
    for i, (bad, status) in enumerate(cases):
        chains = [good] * (i % 3) + [bad, [(7, 0)], [(H, 0.5)]]
        with pytest.raises(jb.JbError) as e:
            jb.color_check(chains)
        assert e.value.status == status and e.value.bad_index == i % 3, (i, str(e.value))
        out = np.full_like(u, 0x5A)
        c = jb.ColorChain.make(bad)
        rc = jb.lib().jb_color_host(u.ctypes.data_as(ctypes.c_void_p), 15, 5, 4, ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), 15)
        assert rc == status and (out == 0x5A).all(), bad
    # an old-style bad chain IN FRONT of a new one decides too
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[(C, 1.0), (C, 1.0)], [(BLUR, -1.0)]])
    assert e.value.status == -9 and e.value.bad_index == 0
    assert ctypes.sizeof(jb.ColorChain) == 72 and jb.COLOR_OPS_MAX == 8


def test_blur_draws(jb):
    from jpeg_decoder_amd import color
    assert color.COLOR_BLUR == 16
    # dino_color's draws are what they were: the same generator state gives the chains the functions it is made of give
    rng, rng2 = np.random.default_rng(11), np.random.default_rng(11)
    for g in (0, 1, None, None, 1):
        jitter = color.color_jitter(rng2, 0.4, 0.4, 0.2, 0.1)
        want = color.random_apply(rng2, 0.8, jitter) + color.random_grayscale(rng2, 0.2)
        if g == 1:
            want += color.random_solarize(rng2, 0.2)
        assert color.dino_color(rng, g) == want
    assert rng.random() == rng2.random()
    # random_blur: one random() and one uniform(), both always drawn
    for p in (0.0, 0.5, 1.0):
        rng, rng2 = np.random.default_rng(5), np.random.default_rng(5)
        got = color.random_blur(rng, p)
        a, radius = float(rng2.random()), float(rng2.uniform(0.1, 2.0))
        assert got == ([(BLUR, radius)] if a < p else []) and rng.random() == rng2.random()
    assert color.random_blur(np.random.default_rng(1), 1.0, 3.0, 3.0) == [(BLUR, 3.0)]
    with pytest.raises(ValueError):
        color.random_blur(np.random.default_rng(1), 1.0, 2.0, 1.0)
    # dino_augment: dino_color's draws with the blur's two behind the grayscale's; every view consumes the same draws but
    # the solarize's
    for g, p in ((0, 1.0), (1, 0.1), (None, 0.5)):
        rng, rng2 = np.random.default_rng(23), np.random.default_rng(23)
        for _ in range(40):
            jitter = color.color_jitter(rng2, 0.4, 0.4, 0.2, 0.1)
            want = color.random_apply(rng2, 0.8, jitter) + color.random_grayscale(rng2, 0.2) + color.random_blur(rng2, p)
            if g == 1:
                want += color.random_solarize(rng2, 0.2)
            got = color.dino_augment(rng, g)
            assert got == want
            jb.color_check([got])
            ops = [op for op, _ in got]
            assert ops.count(BLUR) == (1 if g == 0 else ops.count(BLUR)) <= 1
            if BLUR in ops:
                assert 0.1 <= got[ops.index(BLUR)][1] <= 2.0 and C not in ops[ops.index(BLUR):] and jb.blur_params(got[ops.index(BLUR)][1])[0] <= 1
                assert all(op == Z for op in ops[ops.index(BLUR) + 1:])
        assert rng.random() == rng2.random()
    kinds = {tuple(op for op, _ in color.dino_augment(rng, 1) if op in (G, BLUR, Z)) for _ in range(600)}
    assert kinds == {(), (G,), (BLUR,), (Z,), (G, BLUR), (G, Z), (BLUR, Z), (G, BLUR, Z)}
    for name in ("blur_params", "COLOR_BLUR", "COLOR_BLUR_BOX_MAX", "random_blur", "dino_augment"):
        assert name in jb.__all__ and hasattr(jb, name), name
