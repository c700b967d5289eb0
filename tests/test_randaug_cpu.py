"""The RandAugment colour operations, host side ("colour chains", include/jpegblk.h): JB_COLOR_POSTERIZE / _INVERT /
_AUTOCONTRAST / _EQUALIZE / _SHARPNESS.  jb_color_host -- the kernels' arithmetic through the same csrc/jb_color_core.h --
against Pillow's recorded answers (tests/golden/randaug_kat.npz, tools/gen_randaug_kat.py) and against the numpy restatement
tests/randaug_ref.py on random and low-entropy images; jb_color_lut over every (lo, hi) pair and on adversarial counts; every
new refusal of jb_color_check; the draws of rand_augment_color and trivial_augment_wide_color.  Everything is bit-exact."""
import ctypes
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
import randaug_ref as RA
from conftest import GOLD

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS
SIZES = [(1, 1), (2, 1), (3, 1), (2, 2), (3, 3), (7, 13), (39, 39), (61, 47)]        # (w, h)
FACTORS = [0.0, 0.1, 0.55, 1.0, 1.3, 1.45, 1.9]


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    if not os.path.exists(jb.lib_path()):
        jb.build_library()
    return jb


def content(w, h, seed=0):
    """random, narrow-range, few-valued or two-valued content, by seed"""
    rng = np.random.default_rng(1000 * w + h + seed)
    kind = seed % 4
    if kind == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 1:
        return rng.integers(40, 200, (h, w, 3), dtype=np.uint8)
    if kind == 2:
        return rng.choice(np.array([3, 90, 91, 200, 250], np.uint8), (h, w, 3))
    return np.where(rng.random((h, w, 3)) < 0.2, 17, 230).astype(np.uint8)


def kat():
    z = np.load(os.path.join(GOLD, "randaug_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    return z["image"], chains, z["out"]


def test_constants_and_exports(jb):
    assert (jb.COLOR_POSTERIZE, jb.COLOR_INVERT, jb.COLOR_AUTOCONTRAST, jb.COLOR_EQUALIZE, jb.COLOR_SHARPNESS) == (P, I, A, E, SH) == (10, 11, 12, 13, 17)
    assert jb.COLOR_STATS_MAX == 2 == RA.STATS_MAX and jb.COLOR_OPS_MAX == 8
    for name in ("COLOR_POSTERIZE", "COLOR_INVERT", "COLOR_AUTOCONTRAST", "COLOR_EQUALIZE", "COLOR_SHARPNESS", "COLOR_STATS_MAX", "color_lut",
                 "posterize", "invert", "autocontrast", "equalize", "sharpness", "rand_augment_color", "trivial_augment_wide_color"):
        assert name in jb.__all__ and hasattr(jb, name), name
    assert jb.posterize(3) + jb.invert() + jb.autocontrast() + jb.equalize() + jb.sharpness(1.5) == [(P, 3.0), (I, 0.0), (A, 0.0), (E, 0.0), (SH, 1.5)]
    for bad in (lambda: jb.posterize(9), lambda: jb.posterize(2.5), lambda: jb.sharpness(-1), lambda: jb.sharpness(float("nan")), lambda: jb.sharpness(float("inf"))):
        with pytest.raises(ValueError):
            bad()


def test_reference_matches_pillow():
    """tests/randaug_ref.py alone against Pillow, where Pillow imports: it shows that the reference the other tests use is
    Pillow's, independently of the library.  It runs no code of the library and passes without the feature: it is not one of
    the tests that cover it."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    for w, h in SIZES:
        for seed in range(4):
            u = content(w, h, seed)
            im = Image.fromarray(u)
            assert np.array_equal(RA.apply_op(u, A, 0), np.asarray(ImageOps.autocontrast(im)))
            assert np.array_equal(RA.apply_op(u, E, 0), np.asarray(ImageOps.equalize(im)))
            assert np.array_equal(RA.apply_op(u, I, 0), np.asarray(ImageOps.invert(im)))
            for bits in range(9):
                assert np.array_equal(RA.apply_op(u, P, bits), np.asarray(ImageOps.posterize(im, bits)))
            for a in FACTORS:
                assert np.array_equal(RA.sharpen(u, a), np.asarray(ImageEnhance.Sharpness(im).enhance(a))), (w, h, a)


def test_host_matches_the_known_answers_and_the_reference(jb):
    image, chains, outs = kat()
    assert len(chains) >= 24 and image.shape == (47, 61, 3)
    kinds = [tuple(op for op, _ in c if op in (C, A, E)) for c in chains]
    assert {(E, C), (C, E), (A, C), (C, A), (A, E), (E, A), (E, E), (A, A)} <= set(kinds)
    assert {v for c in chains for op, v in c if op == SH} >= {0.0, np.float32(0.1), 1.0, np.float32(1.9)}
    assert {v for c in chains for op, v in c if op == P} >= {0.0, 8.0}
    for chain, want in zip(chains, outs):
        assert np.array_equal(jb.color_host(image, chain), want), chain     # Pillow's recorded bits
        assert np.array_equal(RA.apply_chain(image, chain), want), chain


HOST_CHAINS = [[(A, 0)], [(E, 0)], [(I, 0)], [(P, 1)], [(P, 7)], [(E, 0), (C, 1.3)], [(C, 0.7), (A, 0)], [(A, 0), (B, 0.8), (E, 0)],
               [(S, 1.3), (E, 0), (H, 77), (A, 0), (SH, 1.6), (Z, 128)], [(P, 3), (A, 0), (BLUR, 1.2), (I, 0)], [(B, 1.2), (SH, 0.3), (P, 5)]]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_matches_the_reference(jb, size):
    for seed in range(4):
        u = content(*size, seed=seed)
        for a in FACTORS:
            assert np.array_equal(jb.color_host(u, [(SH, a)]), RA.sharpen(u, a)), a
        for chain in HOST_CHAINS:
            assert np.array_equal(jb.color_host(u, chain), RA.apply_chain(u, chain)), (seed, chain)


def test_host_224_and_in_place_with_strides(jb):
    u = content(224, 224)
    for a in FACTORS:
        assert np.array_equal(jb.color_host(u, [(SH, a)]), RA.sharpen(u, a)), a
    w, h = 37, 29
    u = content(w, h, seed=1)
    chain = [(E, 0), (C, 1.2), (SH, 1.7), (P, 4)]
    want = RA.apply_chain(u, chain)
    c = jb.ColorChain.make(chain)
    stride = 3 * w + 5
    buf = np.full((h, stride), 0xA5, np.uint8)
    buf[:, :3 * w] = u.reshape(h, 3 * w)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert jb.lib().jb_color_host(p, stride, w, h, ctypes.byref(c), p, stride) == 0          # in == out
    assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want) and (buf[:, 3 * w:] == 0xA5).all()


def test_autocontrast_table_over_every_pair(jb):
    """all 32,640 (lo, hi) with lo < hi against the fp64 definition (Python's floats), and the unchanged cases"""
    n = 0
    for lo in range(256):
        for hi in range(lo + 1, 256):
            h = np.zeros(256, np.uint32)
            h[lo], h[hi] = 1 + (lo % 3), 1 + (hi % 5)
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = [min(max(int(ix * scale + offset), 0), 255) for ix in range(256)]
            got = jb.color_lut(A, h)
            assert got.tolist() == want, (lo, hi)
            n += 1
    assert n == 32640
    one = np.zeros(256, np.uint32)
    one[77] = 5
    assert jb.color_lut(A, one).tolist() == list(range(256)) == RA.autocontrast_lut(one.tolist())
    h = np.zeros(256, np.uint32)
    h[[10, 50, 200]] = 3, 1, 2                                                        # bins between lo and hi do not matter
    assert jb.color_lut(A, h).tolist() == RA.autocontrast_lut(h.tolist())


def _eq(jb, h):
    h = np.asarray(h, np.uint32)
    got = jb.color_lut(E, h).tolist()
    assert got == RA.equalize_lut([int(c) for c in h]), h[h != 0]
    return got


def test_equalize_table_on_adversarial_counts(jb):
    ident = list(range(256))
    h = np.zeros(256, np.int64)
    h[200] = 1000
    assert _eq(jb, h) == ident                                                        # one bin
    h[:] = 0
    h[[3, 250]] = 700, 300
    assert _eq(jb, h) != ident                                                        # two bins: step = 700 // 255 = 2
    h[:] = 0
    h[[3, 250]] = 254, 100000
    assert _eq(jb, h) == ident                                                        # step == 0: N - h[last] = 254 < 255
    h[[3, 250]] = 255, 100000
    assert _eq(jb, h) != ident                                                        # ... and step == 1
    # the unclipped quotient passes 255: 300 pixels spread over 150 bins, step 1, n reaches 299
    h[:] = 0
    h[:150] = 2
    h[255] = 3
    assert RA.equalize_overshoots(h.tolist()) and max(_eq(jb, h)) == 255
    # counts near 2^32: N = 65535 * 65535, in two bins, in 256 bins, and with the last bin holding almost everything
    big = 65535 * 65535
    h[:] = 0
    h[[0, 255]] = big - 7, 7
    _eq(jb, h)
    h[[0, 255]] = 7, big - 7
    assert _eq(jb, h) == ident
    h[:] = big // 256
    h[0] += big - int(h.sum())
    assert int(h.sum()) == big
    lut = _eq(jb, h)
    assert lut[0] == 0 and lut[255] == 255
    h[:] = 0
    h[[1, 2, 3]] = big - (1 << 31) - 5, 5, 1 << 31                                    # step / 2 + before passes 2^32 in bin 3 .. 255
    assert int(h.sum()) == big and ((big - (1 << 31)) // 255) // 2 + big >= 1 << 32
    _eq(jb, h)
    rng = np.random.default_rng(5)
    for _ in range(200):
        h = rng.integers(0, 1 << int(rng.integers(1, 24)), 256) * (rng.random(256) < rng.random())
        _eq(jb, h)


def test_color_lut_refusals(jb):
    L = jb.lib()
    h = np.ones(256, np.uint32)
    lut = np.full(256, 0x5A, np.uint8)
    hp, lp = h.ctypes.data_as(ctypes.c_void_p), lut.ctypes.data_as(ctypes.c_void_p)
    assert L.jb_color_lut(E, None, lp) == -1 and L.jb_color_lut(E, hp, None) == -1
    for op in (0, C, P, I, SH, 14, 99):
        assert L.jb_color_lut(op, hp, lp) == -2
    assert (lut == 0x5A).all()                                                        # a refusal writes nothing
    # counts that uint32 cannot hold, or that are no counts, are refused and not wrapped
    for bad in (np.ones(255, np.uint32), np.full(256, -1), np.full(256, 1 << 24), np.full(256, 0.5), [float("nan")] * 256, [1 << 32] + [0] * 255):
        with pytest.raises(jb.JbError) as e:
            jb.color_lut(E, bad)
        assert e.value.status == -2
    assert jb.color_lut(E, [3.0] * 256).tolist() == jb.color_lut(E, [3] * 256).tolist()


def test_new_refusals(jb):
    """every new refusal, its status and its index, with an old-style bad chain (an unknown op) BEHIND it: the first bad chain
    decides; and jb_color_host, given the bad chain, writes nothing"""
    inf, nan = float("inf"), float("nan")
    good = [(B, 1.2), (E, 0), (P, 4), (C, 0.9), (I, 0), (SH, 1.5), (Z, 128), (P, 0)]
    jb.color_check([good, [(P, 0)], [(P, 8)], [(SH, 0.0)], [(A, 0), (A, 0)], [(E, 0), (A, 0), (BLUR, 1.0)], [(C, 1), (E, 0), (SH, 1e30)], None])
    cases = [([(P, -1)], -2), ([(P, 9)], -2), ([(P, 2.5)], -2), ([(P, nan)], -2),
             ([(I, 1)], -2), ([(A, 0.5)], -2), ([(E, -1)], -2), ([(E, nan)], -2),
             ([(SH, -0.1)], -2), ([(SH, nan)], -2), ([(SH, inf)], -2),
             ([(A, 0), (E, 0), (A, 0)], -9), ([(C, 1.0), (E, 0), (B, 1.0), (A, 0)], -9),          # three statistics operations
             ([(C, 1.0), (A, 0), (C, 1.0)], -9),                                                   # (two contrasts: today's refusal)
             ([(SH, 1.0), (SH, 1.0)], -9), ([(SH, 1.0), (BLUR, 1.0)], -9), ([(BLUR, 1.0), (B, 1.0), (SH, 1.0)], -9),
             ([(SH, 1.0), (C, 1.0)], -9), ([(SH, 1.0), (A, 0)], -9), ([(SH, 1.0), (B, 1.0), (E, 0)], -9), ([(BLUR, 1.0), (E, 0)], -9),
             ([(BLUR, 1.0), (A, 0)], -9),
             ([(SH, 1.0), (E, 0), (H, 300)], -2),                                                  # wrong both ways: GEOMETRY
             ([(A, 0), (E, 0), (A, 0), (P, 9)], -2), ([(SH, 1.0), (SH, 1.0), (7, 0)], -2), ([(SH, 1.0), (SH, 1.0), (9, 0)], -2)]
    u = np.full((4, 5, 3), 9, np.uint8)
    for i, (bad, status) in enumerate(cases):
        chains = [good] * (i % 3) + [bad, [(7, 0)], [(H, 0.5)]]
        with pytest.raises(jb.JbError) as e:
            jb.color_check(chains)
        assert e.value.status == status and e.value.bad_index == i % 3, (i, bad, str(e.value))
        out = np.full_like(u, 0x5A)
        c = jb.ColorChain.make(bad)
        rc = jb.lib().jb_color_host(u.ctypes.data_as(ctypes.c_void_p), 15, 5, 4, ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), 15)
        assert rc == status and (out == 0x5A).all(), bad
    # today's messages stay for today's refusals; an old-style bad chain IN FRONT of a new one decides
    for bad, text in (([(C, 1.0), (A, 0), (C, 1.0)], "more than one JB_COLOR_CONTRAST"), ([(BLUR, 1.0), (BLUR, 1.0)], "more than one JB_COLOR_BLUR"),
                      ([(BLUR, 1.0), (C, 1.0)], "a JB_COLOR_CONTRAST behind a JB_COLOR_BLUR")):
        with pytest.raises(jb.JbError) as e:
            jb.color_check([bad])
        assert e.value.status == -9 and text in str(e.value)
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[(C, 1.0), (C, 1.0)], [(SH, -1.0)]])
    assert e.value.status == -9 and e.value.bad_index == 0
    for op in (0, 7, 9, 14, 15, 18, 99):                                             # unassigned numbers stay unknown
        with pytest.raises(jb.JbError) as e:
            jb.color_check([[(op, 0)]])
        assert e.value.status == -2


def test_generators(jb):
    from jpeg_decoder_amd import color
    ra, taw = color.rand_augment_color, color.trivial_augment_wide_color
    # the same seed gives the same chains
    assert [ra(np.random.default_rng(3)) for _ in range(2)][0] == ra(np.random.default_rng(3))
    a, b = np.random.default_rng(8), np.random.default_rng(8)
    assert [ra(a, 3, 17) + taw(a) for _ in range(50)] == [ra(b, 3, 17) + taw(b) for _ in range(50)]
    # every chain can be had, over 10,000 draws; every entry and every pair that can be had is seen
    rng = np.random.default_rng(2024)
    chains = [ra(rng, int(rng.integers(0, 5)), int(rng.integers(0, 31))) for _ in range(5000)] + [taw(rng) for _ in range(5000)]
    jb.color_check(chains)
    assert {op for c in chains for op, _ in c} == {B, S, C, SH, P, Z, A, E}
    assert any(c == [] for c in chains[5000:]) and max(len(c) for c in chains[5000:]) == 1 and max(len(c) for c in chains[:5000]) == 4
    pairs = {tuple(op for op, _ in c) for c in (ra(rng) for _ in range(4000))}
    assert len([p for p in pairs if len(p) == 2]) == 8 * 8 - 5
    assert not pairs & {(C, C), (SH, SH), (SH, C), (SH, A), (SH, E)}
    # the magnitude tables at m = 0, 9 and 30: RandAugment's (num_ops = 1: the entry decides the draws)
    def table(gen, m):
        """entry -> the set of values seen at magnitude bin m"""
        seen = {}
        rng = np.random.default_rng(m)
        for _ in range(600):
            for op, v in gen(rng, m):
                seen.setdefault(op, set()).add(v)
        return seen
    near = lambda got, want: len(got) == len(want) and all(any(abs(g - w) < 2e-7 for g in got) for w in want)
    for m, mag, bits, thr in ((0, 0.0, 8, 255), (9, 0.27, 7, 179), (30, 0.9, 4, 0)):
        t = table(lambda rng, m: ra(rng, 1, m), m)
        for op in (B, S, C, SH):
            assert near(t[op], {1 - mag, 1 + mag}), (m, op, t[op])
        assert t[P] == {float(bits)} and t[Z] == {float(thr)} and t[A] == t[E] == {0.0}
    # TrivialAugmentWide's: linspace(0, 0.99, 31), posterize down to 2 bits; the bin is a draw
    rng = np.random.default_rng(77)
    seen = {}
    for _ in range(20000):
        for op, v in taw(rng):
            seen.setdefault(op, set()).add(v)
    for op in (B, S, C, SH):
        want = {1 + s * 0.99 * m / 30 for m in range(31) for s in (-1, 1)}
        assert near(seen[op], want), op
    assert seen[P] == {8.0 - round(m / 5) for m in range(31)} == {float(b) for b in range(2, 9)}
    assert seen[Z] == {float(int(np.ceil(255 - 8.5 * m))) for m in range(31)} and len(seen[Z]) == 31
    import math
    assert all(math.ceil(255 - 8.5 * m) == (255 - 8.5 * m if m % 2 == 0 else 255 - 8.5 * m + 0.5) for m in range(31))
    # the draws: index, then (TrivialAugmentWide) the bin, then the sign
    rng, rng2 = np.random.default_rng(13), np.random.default_rng(13)
    for _ in range(200):
        got = taw(rng)
        index = int(rng2.integers(9))
        if index in (1, 2, 3, 4, 5, 6):
            rng2.integers(31)
        if index in (1, 2, 3, 4):
            rng2.integers(2)
        assert (got == []) == (index == 0)
    assert rng.random() == rng2.random()
    with pytest.raises(ValueError):
        ra(rng, 2, 31)
    with pytest.raises(ValueError):
        ra(rng, 9, 3)
