"""Output formats, host side (no GPU): jb_output_bytes, the refusals of a bad jb_output_spec, and the NumPy
reference tests/format_ref.py checked by hand -- including the rounding cases the GPU tests rely on."""
import ctypes

import numpy as np
import pytest

import format_ref as fr


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


ESIZE = {0: 1, 1: 1, 2: 4, 3: 2}


@pytest.mark.parametrize("w,h", [(1, 1), (7, 13), (679, 451), (1920, 1080), (4096, 4096), (65535, 1), (65535, 65535)])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_output_bytes(jb, w, h, fmt):
    assert jb.output_bytes(w, h, fmt) == 3 * w * h * ESIZE[fmt]          # (Python integers: no overflow on this side)
    assert jb.output_bytes(w, h, jb.OutputSpec.make(fmt)) == 3 * w * h * ESIZE[fmt]


def test_output_bytes_refusals(jb):
    n = ctypes.c_int64(-1)
    L = jb.lib()
    assert L.jb_output_bytes(16, 16, 0, None) == -1
    for fmt in (-1, 4, 99):
        assert L.jb_output_bytes(16, 16, fmt, ctypes.byref(n)) == -2
    for w, h in ((0, 5), (5, 0), (65536, 5), (5, 65536), (-3, 5)):
        assert L.jb_output_bytes(w, h, 1, ctypes.byref(n)) == -2
    with pytest.raises(jb.JbError) as e:
        jb.output_bytes(16, 16, 7)
    assert e.value.status == -2


def test_output_spec_refusals(jb):
    L = jb.lib()
    check = lambda s, h=10, row=100: L.jb_output_spec_check(ctypes.byref(s), h, row)
    assert L.jb_output_spec_check(None, 10, 100) == -1
    for fmt in (0, 1, 2, 3):
        assert check(jb.OutputSpec.make(fmt)) == 0
        assert check(jb.OutputSpec.imagenet(fmt)) == 0
    for fmt in (-1, 4, 1 << 20):                       # unknown format
        assert check(jb.OutputSpec.make(fmt)) == -2
    for fmt in (0, 1, 2, 3):                           # reserved must be 0
        s = jb.OutputSpec.make(fmt)
        s.reserved = 1
        assert check(s) == -2
    for fmt in (1, 2, 3):                              # planes may not overlap
        assert check(jb.OutputSpec.make(fmt, plane_stride=999)) == -2
        assert check(jb.OutputSpec.make(fmt, plane_stride=1000)) == 0
        assert check(jb.OutputSpec.make(fmt, plane_stride=0)) == 0
    for fmt in (2, 3):                                 # scale / bias must be finite
        for bad in (float("inf"), float("-inf"), float("nan")):
            for c in range(3):
                sc, bi = [1.0] * 3, [0.0] * 3
                sc[c] = bad
                assert check(jb.OutputSpec.make(fmt, sc, bi)) == -2
                sc, bi = [1.0] * 3, [0.0] * 3
                bi[c] = bad
                assert check(jb.OutputSpec.make(fmt, sc, bi)) == -2
    assert check(jb.OutputSpec.make(1, [float("nan")] * 3)) == 0   # (uint8 planes do not look at them)


def test_entry_points_refuse_without_a_context(jb):
    L = jb.lib()
    s = jb.OutputSpec.make(1)
    p, w, h = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
    assert L.jb_blocks_to_rgb_device_fmt(None, None, ctypes.byref(s), None) == -1
    assert L.jb_decode_memory_fmt(None, None, 0, ctypes.byref(s), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)) == -1
    assert L.jb_decode_file_fmt(None, b"x.jpg", ctypes.byref(s), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)) == -1
    assert L.jb_batch_decoder_set_output_format(None, ctypes.byref(s)) == -1


def test_format_ref_by_hand():
    full = np.array([[[0, 1, 2], [3, 4, 5]], [[250, 251, 252], [253, 254, 255]]], np.uint8)   # [2, 2, 3]
    assert np.array_equal(fr.to_format(full, 0), full)
    chw = fr.to_format(full, 1)
    assert chw.dtype == np.uint8 and chw.tolist() == [[[0, 3], [250, 253]], [[1, 4], [251, 254]], [[2, 5], [252, 255]]]
    f = fr.to_format(full, 2, (2.0, 0.5, 1.0), (1.0, 0.0, -2.0))
    assert f.dtype == np.float32
    assert f.tolist() == [[[1.0, 7.0], [501.0, 507.0]], [[0.5, 2.0], [125.5, 127.0]], [[0.0, 3.0], [250.0, 253.0]]]
    h = fr.to_format(full, 3, (2.0, 0.5, 1.0), (1.0, 0.0, -2.0))
    assert h.dtype == np.float16 and h.astype(np.float32).tolist() == f.tolist()          # all exact in f16


def test_format_ref_f16_tie_goes_to_even():
    """128 * (1 + 2**-11) = 128.0625 exactly (the product is exact in float32): f16 has 128.0 (0x5800, even) and 128.125
    (0x5801, odd) there and the value is exactly halfway, so the conversion must give 128.0 -- rounding halves up or
    away from zero gives 0x5801.  The same holds at every power of two 1 .. 128: the set's 8 ties."""
    s, b = fr.F16_TIES
    u = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    v32 = fr.to_format(u, 2, s, b)[0, 0]
    v16 = fr.to_format(u, 3, s, b)[0, 0]
    assert float(v32[128]) == 128.0625
    lo, hi = np.float16(128.0), np.float16(128.125)
    assert lo.view(np.uint16) == 0x5800 and hi.view(np.uint16) == 0x5801
    assert float(hi) - float(v32[128]) == float(v32[128]) - float(lo)                          # exactly halfway
    assert v16[128].view(np.uint16) == 0x5800                                                  # -> the even one
    # all ties of this parameter set, found exactly (float64 holds every value involved): 8, each to the even neighbour
    ties = 0
    for x in range(256):
        v = float(v32[x])
        assert v == x * (1 + 2.0 ** -11)                                                       # products are exact
        got = v16[x]
        below = got if float(got) <= v else np.nextafter(got, np.float16(-np.inf))
        above = np.nextafter(below, np.float16(np.inf))
        if float(below) != v and v - float(below) == float(above) - v:
            ties += 1
            assert got.view(np.uint16) % 2 == 0, x
    assert ties == 8
    assert [x for x in range(256) if v16[x] != np.float16(v32[x])] == []


def _rtz_product(u, s):
    """float32(u) * s rounded toward zero, from the exact product (float64 holds it: 8 + 24 bits)."""
    exact = u.astype(np.float64) * np.float64(s)
    rn = u.astype(np.float32) * s
    over = np.abs(rn.astype(np.float64)) > np.abs(exact)
    rtz = rn.copy()
    rtz[over] = np.nextafter(rn[over], np.float32(0))
    return exact, rn, rtz


def test_format_ref_unit_scale_separates_the_rounding_modes():
    """scale = 1/255: 247 of the 256 products are inexact and 126 round differently toward zero and to nearest, so a
    multiply issued while the wave is in round-toward-zero mode cannot pass the GPU tests.  By hand: 3 * f32(1/255)."""
    s = np.float32(1.0 / 255.0)
    u = np.arange(256)
    exact, rn, rtz = _rtz_product(u, s)
    assert int((rn.astype(np.float64) != exact).sum()) == 247
    differ = rn.view(np.uint32) != rtz.view(np.uint32)
    assert int(differ.sum()) == 126
    ref = fr.to_format(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2), 2, *fr.UNIT)[1, 0]
    assert np.array_equal(ref.view(np.uint32), rn.view(np.uint32))               # the reference rounds to nearest
    x = int(np.flatnonzero(differ)[0])
    assert ref[x].view(np.uint32) == rtz[x].view(np.uint32) + 1                  # one ulp above the truncated product
    # and neither this set nor ImageNet's has a single f16 tie (so only F16_TIES tests the tie rule)
    for scale, bias in (fr.UNIT, fr.IMAGENET):
        for c in range(3):
            v = u.astype(np.float32) * np.float32(scale[c]) + np.float32(bias[c])
            h = v.astype(np.float16)
            below = np.where(h.astype(np.float32) <= v, h, np.nextafter(h, np.float16(-np.inf)))
            above = np.nextafter(below, np.float16(np.inf))
            d0 = v.astype(np.float64) - below.astype(np.float64)
            d1 = above.astype(np.float64) - v.astype(np.float64)
            assert not ((d0 == d1) & (d0 != 0)).any()


def test_imagenet_spec_matches_format_ref(jb):
    s = jb.OutputSpec.imagenet(2)
    assert [np.float32(x) for x in fr.IMAGENET[0]] == [np.float32(x) for x in s.scale]
    assert [np.float32(x) for x in fr.IMAGENET[1]] == [np.float32(x) for x in s.bias]
    assert jb.FMT_DTYPE[3] is np.float16 and jb.OutputSpec.make(3).dtype is np.float16
