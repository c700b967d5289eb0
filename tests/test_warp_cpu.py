"""The geometric operations of the colour chains, host side ("colour chains", include/jpegblk.h): JB_COLOR_SHEAR_X / _SHEAR_Y /
_TRANSLATE_X / _TRANSLATE_Y / _ROTATE.  jb_color_host -- the kernels' gather through the same csrc/jb_color_core.h -- against
Pillow's recorded answers (tests/golden/warp_kat.npz, tools/gen_warp_kat.py) and against the numpy restatement
tests/warp_ref.py; jb_warp_params against the restatement and against closed forms; every new refusal of jb_color_check, of
jb_warp_params and of the size; the draws of rand_augment and trivial_augment_wide.  Everything is exact equality."""
import ctypes
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
import randaug_ref as RA
import warp_ref as WR
from conftest import GOLD

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS
SX, SY, TX, TY, ROT = WR.SHEAR_X, WR.SHEAR_Y, WR.TRANSLATE_X, WR.TRANSLATE_Y, WR.ROTATE
SIZES = [(1, 1), (2, 1), (3, 2), (7, 13), (61, 47), (257, 5), (2, 300)]              # (w, h)
SHEARS = [0.0, 0.03, -0.03, 0.27, -0.27, 0.3, 0.99, -0.99]
TRANSLATIONS = [0, 1, -1, 13, -13, -32, 1000]
ROTATIONS = [1, -1, 30, -30, 44.999, 90, 91, 135, -179, 360]


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    if not os.path.exists(jb.lib_path()):
        jb.build_library()
    return jb


def content(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    return rng.integers(1, 256, (h, w, 3), dtype=np.uint8)               # (no black: a filled pixel is told from a copied one)


def kat():
    z = np.load(os.path.join(GOLD, "warp_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    return z["image"], chains, z["out"]


def params(jb, op, v, w, h):
    """(mode, coef) or the status of the refusal"""
    try:
        return jb.warp_params(op, v, w, h)
    except jb.JbError as e:
        return e.status


def ref_params(op, v, w, h):
    try:
        return WR.params(op, v, w, h)
    except WR.Unsupported:
        return -9
    except WR.Geometry:
        return -2


def test_constants_and_exports(jb):
    assert (jb.COLOR_SHEAR_X, jb.COLOR_SHEAR_Y, jb.COLOR_TRANSLATE_X, jb.COLOR_TRANSLATE_Y, jb.COLOR_ROTATE) == (SX, SY, TX, TY, ROT) == (32, 33, 34, 35, 36)
    assert jb.COLOR_WARPS_MAX == 2 == WR.WARPS_MAX and (jb.WARP_SHIFT, jb.WARP_FIXED) == (WR.SHIFT, WR.FIXED) == (0, 1)
    assert ctypes.sizeof(jb.ColorChain) == 72
    for name in ("COLOR_SHEAR_X", "COLOR_SHEAR_Y", "COLOR_TRANSLATE_X", "COLOR_TRANSLATE_Y", "COLOR_ROTATE", "COLOR_WARPS_MAX", "warp_params",
                 "shear_x", "shear_y", "translate_x", "translate_y", "rotate", "rand_augment", "trivial_augment_wide"):
        assert name in jb.__all__ and hasattr(jb, name), name
    assert jb.shear_x(0.25) + jb.shear_y(-0.5) + jb.translate_x(3) + jb.translate_y(-4) + jb.rotate(30) == [(SX, 0.25), (SY, -0.5), (TX, 3.0), (TY, -4.0), (ROT, 30.0)]
    assert jb.rotate(0) == jb.rotate(360) == jb.rotate(-720.0) == []
    for bad in (lambda: jb.rotate(180), lambda: jb.rotate(-180), lambda: jb.rotate(540.0), lambda: jb.rotate(float("nan")), lambda: jb.shear_x(float("inf")),
                lambda: jb.shear_y(float("nan")), lambda: jb.translate_x(1.5), lambda: jb.translate_y(65536), lambda: jb.translate_x(float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_reference_matches_pillow():
    """tests/warp_ref.py alone against Pillow, where Pillow imports: Image.transform(AFFINE, NEAREST) with the restated matrix
    and Image.rotate itself.  It runs no code of the library and passes without the feature: it is not one of the tests that
    cover it."""
    Image = pytest.importorskip("PIL.Image")
    for w, h in SIZES + [(64, 64)]:
        u = content(w, h)
        im = Image.fromarray(u)
        for op, values in ((SX, SHEARS), (SY, SHEARS), (TX, TRANSLATIONS), (TY, TRANSLATIONS)):
            for v in values:
                want = np.asarray(im.transform(im.size, Image.AFFINE, WR.matrix(op, v, w, h), Image.NEAREST))
                assert np.array_equal(WR.warp(u, op, v), want), (w, h, op, v)
        for d in ROTATIONS + [270, -90, 12.5]:
            assert np.array_equal(WR.warp(u, ROT, d), np.asarray(im.rotate(d))), (w, h, d)


def test_host_matches_the_known_answers_and_the_reference(jb):
    image, chains, outs = kat()
    assert len(chains) >= 55 and image.shape == (47, 61, 3)
    alone = {c[0] for c in chains if len(c) == 1}
    assert alone >= {(op, float(np.float32(v))) for op in (SX, SY) for v in SHEARS} | {(op, float(t)) for op in (TX, TY) for t in TRANSLATIONS}
    assert alone >= {(ROT, float(np.float32(d))) for d in ROTATIONS}
    kinds = {tuple(op for op, _ in c if op in WR.WARPS + (C, A, E, BLUR, SH)) for c in chains}
    assert {(ROT, C), (C, ROT), (SX, A), (A, SX), (TY, E), (E, TY), (SX, ROT), (ROT, SX), (ROT, BLUR), (SX, TX, SH)} <= kinds
    for chain, want in zip(chains, outs):
        assert np.array_equal(jb.color_host(image, chain), want), chain     # Pillow's recorded bits
        assert np.array_equal(WR.apply_chain(image, chain), want), chain
    moved_out = [o for c, o in zip(chains, outs) if c in ([(TX, 1000.0)], [(TY, 1000.0)])]
    assert len(moved_out) == 2 and not any(o.any() for o in moved_out)


HOST_CHAINS = [[(SX, 0.27)], [(SY, -0.99)], [(TX, 1)], [(TY, -13)], [(TX, 1000)], [(ROT, 30)], [(ROT, -179)], [(ROT, 90)], [(ROT, 360)],
               [(B, 1.2), (SX, -0.3), (I, 0)], [(SY, 0.3), (ROT, 44.999)], [(ROT, 135), (I, 0), (TX, -1)],
               [(ROT, 30), (C, 1.3)], [(C, 1.3), (ROT, 30)], [(E, 0), (SX, 0.5), (A, 0)], [(SY, 0.1), (E, 0), (TY, 1), (C, 0.7), (P, 5)],
               [(ROT, -30), (BLUR, 1.2), (Z, 128)], [(A, 0), (TX, 2), (SY, -0.27), (SH, 1.6), (I, 0)]]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_matches_the_reference(jb, size):
    w, h = size
    changed = 0
    for seed, chain in enumerate(HOST_CHAINS):
        u = content(w, h, seed)
        want = WR.apply_chain(u, chain)
        assert np.array_equal(jb.color_host(u, chain), want), chain
        changed += not np.array_equal(want, u)
    if w * h >= 91:
        assert changed >= len(HOST_CHAINS) - 2


def test_host_in_place_with_strides(jb):
    w, h = 37, 29
    u = content(w, h, seed=1)
    chain = [(E, 0), (ROT, 30), (C, 1.2), (SX, 0.2), (SH, 1.7), (P, 4)]
    want = WR.apply_chain(u, chain)
    c = jb.ColorChain.make(chain)
    stride = 3 * w + 5
    buf = np.full((h, stride), 0xA5, np.uint8)
    buf[:, :3 * w] = u.reshape(h, 3 * w)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert jb.lib().jb_color_host(p, stride, w, h, ctypes.byref(c), p, stride) == 0          # in == out
    assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want) and (buf[:, 3 * w:] == 0xA5).all()


def test_warp_params_against_the_restatement(jb):
    rng = np.random.default_rng(36)
    n = refused = 0
    for w, h in SIZES + [(224, 224), (4000, 3000), (30000, 3), (3, 30000), (40000, 40000), (65535, 65535)]:
        for op in WR.WARPS:
            if op in (TX, TY):
                values = TRANSLATIONS + [65535, -65535, 4096]
            elif op == ROT:
                values = ROTATIONS + [0, 180, -180, 540, 270, -90, 45, 720, 1e6, -1e6] + [float(v) for v in rng.uniform(-400, 400, 40).astype(np.float32)]
            else:
                values = SHEARS + [1, -1, 50, 1e6, -3e38] + [float(v) for v in rng.uniform(-2, 2, 40).astype(np.float32)]
            for v in values:
                got, want = params(jb, op, v, w, h), ref_params(op, v, w, h)
                assert got == want, (op, v, w, h, got, want)
                n += 1
                refused += want == -9
    assert n > 1000 and 50 < refused < n // 2


def test_warp_params_closed_forms(jb):
    for w, h in SIZES:
        for t in TRANSLATIONS + [65535, -65535]:
            assert jb.warp_params(TX, t, w, h) == (jb.WARP_SHIFT, [0, 0, -t, 0, 0, 0])               # a shift by -t
            assert jb.warp_params(TY, t, w, h) == (jb.WARP_SHIFT, [0, 0, 0, 0, 0, -t])
        for op in (SX, SY, ROT):                                                                     # a zero shear, a full turn: the identity
            for v in ((0.0, -0.0) if op != ROT else (0.0, 360.0, -360.0, 720.0)):
                assert jb.warp_params(op, v, w, h) == (jb.WARP_SHIFT, [0] * 6), (op, v)
        # a shear by 1 (45 degrees): tan(atan(1)) is 1 to within 2^-52, far inside FIX's half step
        assert jb.warp_params(SX, 1.0, w, h) == (jb.WARP_FIXED, [65536, 65536, 65536, 0, 65536, 32768])
        assert jb.warp_params(SY, 1.0, w, h) == (jb.WARP_FIXED, [65536, 0, 32768, 65536, 65536, 65536])
    # ROTATE 90 on a square view is a transpose: out[y][x] = u[n - 1 - x][y] (counter-clockwise), for even and odd n
    for n in (1, 2, 5, 64):
        u = content(n, n)
        mode, c = jb.warp_params(ROT, 90, n, n)
        assert (mode, c[0], c[1], c[3], c[4]) == (jb.WARP_FIXED, 0, -65536, 65536, 0)                # (g = -90 degrees: sin g = -1)
        assert np.array_equal(jb.color_host(u, [(ROT, 90)]), np.rot90(u)), n
        assert np.array_equal(jb.color_host(u, [(ROT, -90)]), np.rot90(u, -1)), n
        assert np.array_equal(jb.color_host(u, [(ROT, 90), (ROT, 90)]), np.rot90(u, 2)), n


def test_warp_params_refusals(jb):
    L = jb.lib()
    mode, coef = ctypes.c_int32(77), (ctypes.c_int32 * 6)(*[77] * 6)
    call = lambda op, v, w, h: L.jb_warp_params(op, v, w, h, ctypes.byref(mode), coef)
    inf, nan = float("inf"), float("nan")
    cases = [((B, 1.0, 8, 8), -2), ((0, 0.0, 8, 8), -2), ((31, 0.0, 8, 8), -2), ((37, 0.0, 8, 8), -2), ((SH, 1.0, 8, 8), -2),
             ((SX, 0.1, 0, 8), -2), ((SX, 0.1, 8, 0), -2), ((ROT, 5.0, 65536, 8), -2), ((TX, 1.0, 8, 65536), -2), ((TY, 1.0, -1, 8), -2),
             ((SX, nan, 8, 8), -2), ((SY, inf, 8, 8), -2), ((ROT, -inf, 8, 8), -2), ((TX, nan, 8, 8), -2),
             ((TX, 0.5, 8, 8), -2), ((TY, -1.25, 8, 8), -2), ((TX, 65536.0, 8, 8), -2), ((TY, -65536.0, 8, 8), -2),
             ((ROT, 180.0, 8, 8), -9), ((ROT, -180.0, 61, 47), -9), ((ROT, 540.0, 1, 1), -9),                  # Pillow's scaling path
             ((ROT, 30.0, 40000, 40000), -9), ((SX, 0.3, 32768, 8), -9), ((SY, 50.0, 1000, 8), -9), ((ROT, 1.0, 8, 40000), -9)]   # its float path
    for args, status in cases:
        assert call(*args) == status, args
        assert mode.value == 77 and list(coef) == [77] * 6, args                       # in a refusal nothing is written
        assert ref_params(*args) == status or args[0] not in WR.WARPS or not (1 <= args[2] <= 65535 and 1 <= args[3] <= 65535)
    assert L.jb_warp_params(SX, 0.1, 8, 8, None, coef) == L.jb_warp_params(SX, 0.1, 8, 8, ctypes.byref(mode), None) == -1
    assert call(SX, 0.3, 32760, 8) == 0 and mode.value == 1                   # (32760 + 8 * 0.3 < 32768)


def test_new_refusals(jb):
    """every new refusal of jb_color_check, its status and its index, with an old-style bad chain (an unknown op) BEHIND it: the
    first bad chain decides; and jb_color_host, given the bad chain, writes nothing"""
    inf, nan = float("inf"), float("nan")
    good = [(B, 1.2), (ROT, 30), (E, 0), (SX, -0.3), (C, 0.9), (I, 0), (SH, 1.5), (Z, 128)]
    jb.color_check([good, [(TX, 65535)], [(TY, -65535)], [(ROT, 180)], [(SX, 1e30)], [(SY, 0), (SY, 0)], [(ROT, 1), (BLUR, 1.0)], [(TX, 1), (TY, 1), (SH, 1)],
                    [(A, 0), (SX, 1), (E, 0), (ROT, 3)], None])
    cases = [([(SX, nan)], -2), ([(SX, inf)], -2), ([(SY, -inf)], -2), ([(SY, nan)], -2), ([(ROT, nan)], -2), ([(ROT, inf)], -2),
             ([(TX, nan)], -2), ([(TY, inf)], -2), ([(TX, 0.5)], -2), ([(TY, -2.5)], -2), ([(TX, 65536)], -2), ([(TY, -65536)], -2), ([(TX, 1e9)], -2),
             ([(SX, 0.1), (SY, 0.1), (ROT, 1)], -9), ([(TX, 1), (B, 1.0), (TX, 1), (I, 0), (TX, 1)], -9),          # three geometric operations
             ([(SH, 1.0), (SX, 0.1)], -9), ([(BLUR, 1.0), (ROT, 5)], -9), ([(SH, 1.0), (B, 1.0), (TY, 1)], -9), ([(TX, 1), (BLUR, 0.5), (TX, 1)], -9),
             ([(SH, 1.0), (ROT, 5), (H, 300)], -2), ([(SX, 0.1), (SY, 0.1), (ROT, 1), (TX, 0.5)], -2),             # wrong both ways: GEOMETRY
             ([(SX, 0.1), (SY, 0.1), (ROT, 1), (7, 0)], -2), ([(SH, 1.0), (SX, 0.1), (18, 0)], -2)]
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
    for bad, text in (([(SX, 0.1), (SY, 0.1), (ROT, 1)], "more than JB_COLOR_WARPS_MAX"), ([(SH, 1.0), (SX, 0.1)], "behind a neighbourhood operation")):
        with pytest.raises(jb.JbError) as e:
            jb.color_check([bad])
        assert e.value.status == -9 and text in str(e.value)
    # an old-style bad chain IN FRONT of a new one decides
    with pytest.raises(jb.JbError) as e:
        jb.color_check([[(C, 1.0), (C, 1.0)], [(SX, nan)]])
    assert e.value.status == -9 and e.value.bad_index == 0
    # the refusals that depend on the size are jb_color_host's own, behind jb_color_check's (which passes these chains)
    for bad, w, h in (([(B, 1.1), (ROT, 180)], 5, 4), ([(ROT, -180)], 1, 1), ([(SY, 50.0)], 700, 2), ([(I, 0), (TX, 1), (SX, 1.0)], 2, 40000)):
        jb.color_check([bad])
        v = np.full((h, w, 3), 9, np.uint8)
        out = np.full_like(v, 0x5A)
        c = jb.ColorChain.make(bad)
        rc = jb.lib().jb_color_host(v.ctypes.data_as(ctypes.c_void_p), 3 * w, w, h, ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), 3 * w)
        assert rc == -9 and (out == 0x5A).all() and "colour chain 0" in jb.lib().jb_last_error(None).decode(), bad
    for op in (0, 7, 9, 14, 15, 18, 31, 37, 99):                                     # unassigned numbers stay unknown
        with pytest.raises(jb.JbError) as e:
            jb.color_check([[(op, 0)]])
        assert e.value.status == -2


def test_generators(jb):
    from jpeg_decoder_amd import color
    ra, taw = color.rand_augment, color.trivial_augment_wide
    order = [None, SX, SY, TX, TY, ROT, B, S, C, SH, P, Z, A, E]                   # torchvision's table; None: Identity
    signed = {1, 2, 3, 4, 5, 6, 7, 8, 9}
    # the same generator state gives the same chains
    assert ra(np.random.default_rng(3), 224, 224) == ra(np.random.default_rng(3), 224, 224)
    a, b = np.random.default_rng(8), np.random.default_rng(8)
    assert [ra(a, 96, 224, 3, 17) + taw(a) for _ in range(50)] == [ra(b, 96, 224, 3, 17) + taw(b) for _ in range(50)]
    # every chain can be had, at its size too; every entry is seen
    rng = np.random.default_rng(2025)
    sizes = [(224, 224), (96, 96), (1, 1), (331, 17), (16384, 16384)]
    drawn = [(sizes[i % 5], ra(rng, *sizes[i % 5], int(rng.integers(0, 6)), int(rng.integers(0, 31)))) for i in range(5000)]
    drawn += [(sizes[i % 5], taw(rng)) for i in range(5000)]
    jb.color_check([c for _, c in drawn])
    for (w, h), c in drawn:
        for op, v in c:
            if op in WR.WARPS:
                assert isinstance(params(jb, op, v, w, h), tuple), (op, v, w, h)
    assert {op for _, c in drawn for op, _ in c} == set(order[1:])
    assert max(sum(op in WR.WARPS for op, _ in c) for _, c in drawn) == 2 and max(len(c) for _, c in drawn[:5000]) == 5
    assert any(c == [] for _, c in drawn[5000:]) and max(len(c) for _, c in drawn[5000:]) == 1
    # the table's order and the draws: index, (TrivialAugmentWide: the bin), the sign.  At magnitude 9 no entry is dropped but
    # Identity, and with one operation nothing is redrawn.
    rng, rng2 = np.random.default_rng(13), np.random.default_rng(13)
    for _ in range(400):
        got = ra(rng, 224, 224, 1, 9)
        index = int(rng2.integers(14))
        negative = bool(int(rng2.integers(2))) if index in signed else False
        assert [op for op, _ in got] == ([] if index == 0 else [order[index]]), (index, got)
        if index in (1, 2, 5):
            assert (got[0][1] < 0) == negative
        if index in (3, 4):
            assert got[0][1] == (-1 if negative else 1) * int(float(np.float32(150.0 / 331.0 * 224)) * 9 / 30)
    assert rng.random() == rng2.random()
    rng, rng2 = np.random.default_rng(14), np.random.default_rng(14)
    for _ in range(400):
        got = taw(rng)
        index = int(rng2.integers(14))
        m = int(rng2.integers(31)) if index not in (0, 12, 13) else 0
        negative = bool(int(rng2.integers(2))) if index in signed else False
        if index == 0 or (index == 5 and m == 0):
            assert got == []
        else:
            assert [op for op, _ in got] == [order[index]], (index, got)
        if index in (3, 4):
            assert got[0][1] == (-1 if negative else 1) * int(32 * m / 30 + 1e-4)
    assert rng.random() == rng2.random()
    # the magnitudes: RandAugment's at bins 0, 9 and 30, for a view of 331 x 224
    near = lambda got, want: len(got) == len(want) and all(any(abs(g - w) < 3e-6 * max(1, abs(w)) for g in got) for w in want)
    for m, shear, tx, ty, deg in ((0, 0.0, 0, 0, 0.0), (9, 0.09, 45, 30, 9.0), (30, 0.3, 150, 101, 30.0)):
        seen = {}
        rng = np.random.default_rng(m)
        for _ in range(800):
            for op, v in ra(rng, 331, 224, 1, m):
                seen.setdefault(op, set()).add(v)
        assert near(seen[SX], {shear, -shear}) and near(seen[SY], {shear, -shear}), (m, seen[SX])
        assert seen[TX] == {float(tx), float(-tx)} and seen[TY] == {float(ty), float(-ty)}, (m, seen[TX], seen[TY])
        assert (ROT not in seen) if m == 0 else near(seen[ROT], {deg, -deg})
    # TrivialAugmentWide's: shear linspace(0, 0.99), translate int(linspace(0, 32)), rotate linspace(0, 135); the bin is a draw
    rng = np.random.default_rng(77)
    seen = {}
    for _ in range(30000):
        for op, v in taw(rng):
            seen.setdefault(op, set()).add(v)
    assert near(seen[SX], {s * 0.99 * m / 30 for m in range(31) for s in (-1, 1)}) and near(seen[SY], seen[SX])
    assert seen[TX] == seen[TY] == {float(s * int(32 * m / 30 + 1e-4)) for m in range(31) for s in (-1, 1)}
    assert near(seen[ROT], {s * 4.5 * m for m in range(1, 31) for s in (-1, 1)})
    # the redraw rule: at num_ops = 2, 10 of the 196 ordered pairs are never seen -- rand_augment_color's 5 and Sharpness followed
    # by each geometric entry; every other pair of entries is
    rng = np.random.default_rng(5)
    pairs = {tuple(op for op, _ in c) for c in (ra(rng, 224, 224) for _ in range(20000))}
    refused = {(C, C), (SH, SH), (SH, C), (SH, A), (SH, E)} | {(SH, g) for g in WR.WARPS}
    assert len(refused) == 10 and not pairs & refused
    assert {p for p in pairs if len(p) == 2} == {(x, y) for x in order[1:] for y in order[1:]} - refused
    assert len([p for p in pairs if len(p) == 2]) == 13 * 13 - 10
    for bad in (lambda: ra(rng, 224, 224, 2, 31), lambda: ra(rng, 224, 224, 9, 3), lambda: ra(rng, 0, 224), lambda: ra(rng, 224, 16385), lambda: taw(rng, 0)):
        with pytest.raises(ValueError):
            bad()
    # the two _color functions and their draws stay what they were
    a, b = np.random.default_rng(21), np.random.default_rng(21)
    for _ in range(100):
        got = color.trivial_augment_wide_color(a)
        index = int(b.integers(9))
        if index in (1, 2, 3, 4, 5, 6):
            b.integers(31)
        if index in (1, 2, 3, 4):
            b.integers(2)
        assert (got == []) == (index == 0)
    assert a.random() == b.random()
