"""Fixed output size, host side (no GPU): the numpy reference's own properties, jb_resize_check and the output plan's
statuses and their order, the null pointers, and the Python wrapper's refusal of resize= together with a scale before any
device call."""
import ctypes

import numpy as np
import pytest

from area_reduce import area_reduce
from resize_ref import area_resize, area_sums, weights


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


# ---- the reference checks itself ----------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (1, 5), (5, 1), (7, 7), (33, 7), (9, 20), (679, 224), (520, 65), (4608, 3), (65535, 2)])
def test_weights_sum_to_the_source_length_and_cover_the_grid(n_in, n_out):
    w = weights(n_in, n_out)
    assert w.shape == (n_out, n_in) and (w >= 0).all()
    assert (w.sum(axis=1) == n_in).all()      # every output cell is n_in units long
    assert (w.sum(axis=0) == n_out).all()     # and every source cell is used up, n_out units


def _img(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_reference_identity_and_constant():
    for w, h in ((1, 1), (16, 16), (33, 17), (679, 451)):
        img = _img(w, h, w + h)
        assert np.array_equal(area_resize(img, w, h), img)
    for v in (0, 1, 127, 128, 254, 255):
        img = np.full((17, 33, 3), v, np.uint8)
        for ow, oh in ((7, 5), (1, 1), (40, 31), (80, 3), (33, 17)):
            assert (area_resize(img, ow, oh) == v).all(), (v, ow, oh)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_reference_equals_area_reduce_on_divisible_sizes(k):
    for ow, oh in ((1, 1), (8, 6), (31, 17)):
        img = _img(ow * k, oh * k, k + ow)
        assert np.array_equal(area_resize(img, ow, oh), area_reduce(img, k)), (k, ow, oh)


def test_reference_one_pixel_is_the_rounded_mean():
    img = _img(33, 17, 5)
    s = img.astype(np.int64).sum(axis=(0, 1))
    assert np.array_equal(area_sums(img, 1, 1)[0, 0], s)
    assert np.array_equal(area_resize(img, 1, 1)[0, 0], (s + (33 * 17) // 2) // (33 * 17))


# ---- jb_resize_check and the plan ---------------------------------------------------------------
W, H = 679, 451


def _rc(jb, desc, roi, ow, oh):
    return jb.lib().jb_resize_check(ctypes.byref(desc), ctypes.byref(jb.Roi(*roi)) if roi is not None else None, ow, oh)


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2), (2, 1), (1, 2)])
def test_resize_check_accepts(jb, hs, vs):
    d = jb.make_desc(W, H, hs, vs)
    for roi in (None, (0, 0, W, H), (5, 3, 50, 40), (W - 1, H - 1, 1, 1)):
        for ow, oh in ((1, 1), (224, 224), (W, H), (65535, 65535), (65535, 1), (1, 65535)):
            assert _rc(jb, d, roi, ow, oh) == 0, (roi, ow, oh)
    jb.resize_check(d, (224, 224))
    jb.resize_check(d, (13, 11), roi=(5, 3, 50, 40))
    assert _rc(jb, jb.make_desc(1, 1, hs, vs), None, 5, 3) == 0
    assert _rc(jb, jb.make_desc(65535, 65535, hs, vs), None, 1, 1) == 0


def test_resize_check_refusals_and_their_order(jb):
    L = jb.lib()
    d = jb.make_desc(W, H, 2, 2)
    for ow, oh in ((0, 1), (1, 0), (0, 0), (-1, 5), (5, -1), (65536, 1), (1, 65536), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 1)):
        assert _rc(jb, d, None, ow, oh) == -2, (ow, oh)
        assert _rc(jb, d, (0, 0, 8, 8), ow, oh) == -2, (ow, oh)
    for roi in ((0, 0, W + 1, H), (-1, 0, 4, 4), (0, 0, 0, 4), (2 ** 31 - 1, 0, 2, 1)):
        assert _rc(jb, d, roi, 224, 224) == -2, roi
    with pytest.raises(jb.JbError) as e:
        jb.resize_check(d, (0, 224))
    assert e.value.status == -2
    # the descriptor's own errors come first, whatever the rectangle and the target are
    for roi, (ow, oh) in (((0, 0, 1, 1), (8, 8)), ((-1, -1, 0, 0), (0, 0))):
        assert _rc(jb, jb.make_desc(0, 5, 1, 1), roi, ow, oh) == -2
        assert _rc(jb, jb.make_desc(16, 16, 3, 1), roi, ow, oh) == -3      # sampling
        assert _rc(jb, jb.make_desc(16, 16, 1, 1, (0, 4, 1)), roi, ow, oh) == -4   # table id
    assert L.jb_resize_check(None, None, 8, 8) == -1
    assert L.jb_resize_check(None, ctypes.byref(jb.Roi(0, 0, 1, 1)), 0, 0) == -1


def test_null_pointers(jb):
    L = jb.lib()
    vp, i32 = ctypes.c_void_p(), ctypes.c_int32()
    assert L.jb_blocks_to_rgb_device_resized(None, None, None, 8, 8, None, None) == -1
    assert L.jb_decode_memory_resized(None, None, 0, None, 8, 8, None, ctypes.byref(vp), ctypes.byref(i32), ctypes.byref(i32)) == -1
    assert L.jb_decode_file_resized(None, b"/nonexistent.jpg", None, 8, 8, None, ctypes.byref(vp), ctypes.byref(i32), ctypes.byref(i32)) == -1
    assert L.jb_batch_decoder_set_resize(None, 8, 8) == -1


@pytest.mark.parametrize("fmt,es", [(0, 1), (1, 1), (2, 4), (3, 2)])
def test_resized_output_sizes_are_those_of_the_target(jb, fmt, es):
    for w, h in ((1, 1), (224, 224), (65, 3), (65535, 2)):
        assert jb.output_bytes(w, h, fmt) == 3 * w * h * es


def test_resize_with_a_scale_is_refused_before_any_device_call(jb):
    """The wrapper raises JbError(-9) for resize= with scale=2 itself: nothing here has a context, a decoder, a device or
    a library handle to call into (ctx is a bare object)."""
    ctx = object.__new__(jb.Context)
    ctx._h = ctypes.c_void_p()
    for call in (lambda: ctx.blocks_to_rgb_device(jb.DeviceBatch(), scale=2, resize=(8, 8)),
                 lambda: ctx.decode_file("/nonexistent.jpg", scale=2, resize=(8, 8)),
                 lambda: ctx.decode_memory(b"", scale=4, resize=(8, 8)),
                 lambda: ctx.decode_memory(b"", scale=8, fmt=1, resize=(8, 8)),
                 lambda: jb.BatchDecoder(2, 0, scale=2, resize=(8, 8)),
                 lambda: jb.torch_batch(jb.make_desc(16, 16, 1, 1), 1, None, None, None, scale=2, resize=(8, 8))):
        with pytest.raises(jb.JbError) as e:
            call()
        assert e.value.status == -9
