"""Colour chains, host side ("colour chains", include/jpegblk.h): jb_color_host -- the kernels' arithmetic through the same
csrc/jb_color_core.h -- against Pillow's recorded answers (tests/golden/color_kat.npz, tools/gen_color_kat.py), against the
numpy restatement tests/color_ref.py over the colour cube, and against Pillow itself where it imports; the contrast mean's
rounding; every refusal of jb_color_check; jpeg_decoder_amd.color's draws; the binding's colors= keyword.  Everything is
bit-exact: no tolerance anywhere."""
import ctypes
import os
import re

import numpy as np
import pytest

import color_ref as R
from conftest import GOLD, ROOT

B, C, S, H, G, Z = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE
# the ten blend factors: inside [0, 1], its ends, and outside (where the result is clipped)
FACTORS = (0.0, 0.25, 0.3, 0.5, 0.6, 0.999, 1.0, 1.4, 1.7, 2.5)


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    if not os.path.exists(jb.lib_path()):
        jb.build_library()
    return jb


def kat():
    z = np.load(os.path.join(GOLD, "color_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    return z["image"], chains, z["out"]


def test_host_matches_the_known_answers_and_the_reference(jb):
    image, chains, outs = kat()
    assert len(chains) >= 16 and image.shape == (47, 61, 3)
    for chain, want in zip(chains, outs):
        got = jb.color_host(image, chain)
        assert np.array_equal(got, want), chain                      # Pillow's recorded bits
        assert np.array_equal(R.apply_chain(image, chain), want), chain
    assert np.array_equal(jb.color_host(image, []), image) and np.array_equal(jb.color_host(image, None), image)


@pytest.mark.parametrize("chain", [[(H, 37)], [(S, 0.3)], [(G, 0)]], ids=["hue37", "saturation0.3", "grayscale"])
def test_host_matches_the_reference_over_the_cube_slices(jb, chain):
    # (the whole cube takes numpy several seconds per chain: B in {0, 1, 17, 127, 128, 254, 255} x all R, G here; the whole
    # cube runs against Pillow below)
    u = R.cube_slices()
    assert np.array_equal(jb.color_host(u, chain), R.apply_chain(u, chain))


def test_host_matches_pillow_over_the_whole_cube(jb):
    Image = pytest.importorskip("PIL.Image")
    u = R.cube()
    im = Image.fromarray(u)
    lum = np.asarray(im.convert("L"))
    assert np.array_equal(jb.color_host(u, [(G, 0)]), np.repeat(lum[..., None], 3, -1))
    h, s, v = im.convert("HSV").split()
    nh = ((np.asarray(h).astype(np.int64) + 37) & 255).astype(np.uint8)
    want = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    assert np.array_equal(jb.color_host(u, [(H, 37)]), want)
    from PIL import ImageEnhance
    assert np.array_equal(jb.color_host(u, [(S, 0.3)]), np.asarray(ImageEnhance.Color(im).enhance(0.3)))


def test_reference_blend_matches_pillow_on_every_pair():
    Image = pytest.importorskip("PIL.Image")
    d, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for a in FACTORS:
        want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(v), a))
        assert np.array_equal(R.blend(d, v, a), want), a


def test_host_blend_matches_the_reference_on_every_pair(jb):
    # BRIGHTNESS is blend(0, v, a) and CONTRAST blend(m, v, a): a 256-wide image whose luma mean is exactly m gives every
    # (m, v) pair -- the rows hold every v in the red channel, and a gray filler sets the mean
    v = np.arange(256, dtype=np.uint8)
    for a in FACTORS:
        u = np.zeros((1, 256, 3), np.uint8)
        u[0, :, :] = v[:, None]
        assert np.array_equal(jb.color_host(u, [(B, a)]), R.apply_chain(u, [(B, a)])), a
        for m in (0, 1, 127, 128, 254, 255):
            u = np.full((2, 256, 3), m, np.uint8)                     # row 1 is all m; row 0 red = v, mean luma stays near m
            u[0, :, 0] = v
            assert np.array_equal(jb.color_host(u, [(C, a)]), R.apply_chain(u, [(C, a)])), (a, m)


def test_contrast_mean_rounding(jb):
    def mean_of(u):
        # factor 0 turns every channel into m
        out = jb.color_host(u, [(C, 0.0)])
        assert len(np.unique(out)) == 1
        return int(out.flat[0])
    one = np.array([[[10, 200, 30]]], np.uint8)
    assert mean_of(one) == int(R.luma(one)[0, 0]) == R.contrast_mean(one)
    rng = np.random.default_rng(5)
    u = rng.integers(0, 256, (13, 7, 3), dtype=np.uint8)
    assert mean_of(u) == R.contrast_mean(u) == int(R.luma(u).mean() + 0.5)
    # means of exactly k + 1/2 round up: the gray pixels 0, 1 give 1; 254, 255 give 255; four pixels 7, 7, 8, 8 give 8
    for grays, want in (((0, 1), 1), ((254, 255), 255), ((7, 7, 8, 8), 8), ((7, 7, 7, 8), 7)):
        u = np.repeat(np.array(grays, np.uint8)[None, :, None], 3, -1)
        assert (R.luma(u)[0] == np.array(grays)).all()
        assert mean_of(u) == want == R.contrast_mean(u), grays
    # the mean is of the view AS IT STANDS when the contrast is reached
    u = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    chain = [(B, 0.5), (Z, 100), (C, 0.0)]
    assert mean_of(R.apply_chain(u, chain[:2])) == int(jb.color_host(u, chain).flat[0])


def _chain(jb, ops, n_ops=None, reserved=0):
    c = jb.ColorChain.make(ops)
    if n_ops is not None:
        c.n_ops = n_ops
    c.reserved = reserved
    return c


def test_color_check_refusals(jb):
    inf, nan = float("inf"), float("nan")
    good = [(B, 1.2), (C, 0.0), (S, 2.0), (H, 255), (G, 0), (Z, 256), (Z, 0), (H, 0)]
    jb.color_check([good, [], None])
    geometry = [_chain(jb, [], n_ops=-1), _chain(jb, [], n_ops=9), _chain(jb, [], reserved=1), [(0, 1.0)], [(7, 1.0)],
                [(B, -0.1)], [(C, inf)], [(S, nan)], [(B, nan)], [(H, -1)], [(H, 256)], [(H, 1.5)], [(H, nan)],
                [(Z, -1)], [(Z, 257)], [(Z, 127.5)], [(G, 1)], [(B, 1.0)] * 9]
    for i, bad in enumerate(geometry):
        chains = [good] * (i % 3) + [bad, [(7, 0)]]                   # (the FIRST bad chain is named)
        with pytest.raises(jb.JbError) as e:
            jb.color_check(chains)
        assert e.value.status == -2 and e.value.bad_index == i % 3, (i, str(e.value))
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[], [(C, 1.0), (B, 1.0), (C, 1.0)]])
    assert e.value.status == -9 and e.value.bad_index == 1
    # a chain that is wrong in both ways is JB_ERR_GEOMETRY; of two bad chains the first decides
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[(C, 1.0), (C, 1.0), (H, 300)]])
    assert e.value.status == -2 and e.value.bad_index == 0
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[(C, 1.0), (C, 1.0)], [(H, 300)]])
    assert e.value.status == -9 and e.value.bad_index == 0
    L = jb.lib()
    bad = ctypes.c_int(5)
    assert L.jb_color_check(None, 1, ctypes.byref(bad)) == -1 and bad.value == -1
    assert L.jb_color_check(None, 0, None) == 0
    assert L.jb_color_check(None, -1, ctypes.byref(bad)) == -2
    # jb_color_host reports the same statuses and writes nothing
    u = np.zeros((2, 2, 3), np.uint8)
    with pytest.raises(jb.JbError) as e:
        jb.color_host(u, [(H, 1.5)])
    assert e.value.status == -2
    assert ctypes.sizeof(jb.ColorChain) == 72 and ctypes.sizeof(jb.ColorOp) == 8 and jb.COLOR_OPS_MAX == 8


def test_color_draws(jb):
    from jpeg_decoder_amd import color
    def draw(seed):
        rng = np.random.default_rng(seed)
        return [color.dino_color(rng, g) for g in (0, 1, None, None)] + [color.color_jitter(rng, 0.4, 0.4, 0.2, 0.1)]
    assert draw(3) == draw(3) and draw(3) != draw(4)
    rng = np.random.default_rng(0)
    seen_orders = set()
    for _ in range(200):
        chain = color.color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
        assert sorted(op for op, _ in chain) == [B, C, S, H]
        seen_orders.add(tuple(op for op, _ in chain))
        for op, value in chain:
            if op == H:
                assert value == int(value) and (0 <= value <= 25 or 231 <= value <= 255), value
            else:
                x = {B: 0.4, C: 0.4, S: 0.2}[op]
                assert 1 - x <= value <= 1 + x
        jb.color_check([chain])
    assert len(seen_orders) > 12                                      # (of 24 permutations)
    # a parameter of 0 adds no operation; a large one is clamped at 0 from below
    assert color.color_jitter(rng, 0, 0, 0, 0) == []
    assert all(0 <= v <= 3 for _, v in color.color_jitter(rng, 2.0, 0, 0, 0))
    # the hue mapping: truncation toward zero, then mod 256
    assert [color.hue_shift(f) for f in (0.0, 0.1, 0.5, -0.001, -0.004, -0.1, -0.5)] == [0, 25, 127, 0, 255, 231, 129]
    # p = 0 and p = 1
    assert color.random_grayscale(rng, 0.0) == [] and color.random_grayscale(rng, 1.0) == [(G, 0.0)]
    assert color.random_solarize(rng, 1.0) == [(Z, 128.0)] and color.random_solarize(rng, 1.0, 77) == [(Z, 77.0)]
    assert color.random_apply(rng, 0.0, [(B, 1.0)]) == [] and color.random_apply(rng, 1.0, [(B, 1.0)]) == [(B, 1.0)]
    kinds = set()
    for _ in range(300):
        chain = color.dino_color(rng, 1)
        jb.color_check([chain])
        kinds.add((len(chain) >= 4, (G, 0.0) in chain, (Z, 128.0) in chain))
    assert len(kinds) == 8                                            # jitter, grayscale and solarize each come and go
    assert all((Z, 128.0) not in color.dino_color(rng, g) for g in (0, None) for _ in range(50))


def test_colors_keyword(jb):
    from jpeg_decoder_amd.api import _Request, _ROUTES
    with pytest.raises(ValueError):
        _Request(resize=(8, 8), colors=[[[]]])
    views = [[(0, 0, 8, 8), (1, 1, 4, 4, True)]] * 3
    chains = [[None, [(H, 3)]], [[], []], [[(B, 1.5), (C, 0.5)], None]]
    r = _Request(resize=(8, 8), views=views, colors=chains)
    route, tail = r.routed()
    assert route == "views_color" and _ROUTES[route] == (None, None, "jb_blocks_to_rgb_device_views_color")
    assert tail[3] is r.colors and len(r.colors) == 6
    assert [c.n_ops for c in r.colors] == [0, 1, 0, 0, 2, 0] and r.colors[4].ops[1].op == C and r.colors[4].ops[1].value == 0.5
    r = _Request(views=views, view_groups=[(1, (8, 8)), (1, (4, 4), jb.FILTER_BICUBIC)], colors=chains)
    route, tail = r.routed()
    assert route == "view_groups_color" and _ROUTES[route] == (None, None, "jb_blocks_to_rgb_device_view_groups_color")
    assert tail[4] is r.colors
    # without colors the routes are the ones they were
    assert _Request(resize=(8, 8), views=views).routed()[0] == "views"
    assert _Request(views=views, view_groups=[(2, (8, 8))]).routed()[0] == "view_groups"
    for bad in ([[None, None]] * 2, [[None]] * 3, [[None, None, None]] * 3):
        with pytest.raises(jb.JbError) as e:
            _Request(resize=(8, 8), views=views, colors=bad)
        assert e.value.status == -2
    for call in (lambda d: d.run([], colors=[]), lambda d: d.run_to_device([], colors=[]), lambda d: d.submit([], colors=[]),
                 lambda d: d.run_to_tensor([], None, colors=[])):
        with pytest.raises(ValueError):
            call(object.__new__(jb.BatchDecoder))


def test_new_symbols_are_declared_and_exported(jb):
    header = open(os.path.join(ROOT, "include", "jpegblk.h")).read()
    L = ctypes.CDLL(jb.lib_path())
    names = ["jb_color_check", "jb_color_host", "jb_color_device", "jb_blocks_to_rgb_device_views_color",
             "jb_blocks_to_rgb_device_view_groups_color", "jb_batch_decoder_run_views_color", "jb_batch_decoder_submit_views_color",
             "jb_batch_decoder_run_view_groups_color", "jb_batch_decoder_submit_view_groups_color"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    for name in ("ColorChain", "ColorOp", "color_check", "color_host", "color_jitter", "random_apply", "random_grayscale",
                 "random_solarize", "dino_color", "COLOR_BRIGHTNESS", "COLOR_CONTRAST", "COLOR_SATURATION", "COLOR_HUE",
                 "COLOR_GRAYSCALE", "COLOR_SOLARIZE"):
        assert name in jb.__all__ and hasattr(jb, name), name
    assert hasattr(jb.Context, "color_device")
    assert (jb.COLOR_BRIGHTNESS, jb.COLOR_CONTRAST, jb.COLOR_SATURATION, jb.COLOR_HUE, jb.COLOR_GRAYSCALE, jb.COLOR_SOLARIZE) == (1, 2, 3, 4, 5, 6)
