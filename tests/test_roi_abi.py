"""Region of interest, host side (no GPU): jb_roi_check's accepts and refusals, the sizes of an ROI output, and the
Python wrapper's refusal of roi= together with a scale before any device call."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


ESIZE = {0: 1, 1: 1, 2: 4, 3: 2}
W, H = 679, 451


def _rc(jb, desc, roi):
    return jb.lib().jb_roi_check(ctypes.byref(desc), ctypes.byref(jb.Roi(*roi)))


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2), (2, 1), (1, 2)])
def test_roi_check_accepts(jb, hs, vs):
    d = jb.make_desc(W, H, hs, vs)
    for roi in ((0, 0, W, H),                                                          # the whole image
                (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),   # 1 x 1 at each corner
                (1, 1, W - 1, H - 1), (W - 224, H - 224, 224, 224), (0, 0, W, 1), (0, 0, 1, H)):
        assert _rc(jb, d, roi) == 0, roi
        jb.roi_check(d, roi)
    for w, h in ((1, 1), (65535, 65535), (65535, 1)):
        assert _rc(jb, jb.make_desc(w, h, hs, vs), (0, 0, w, h)) == 0
        assert _rc(jb, jb.make_desc(w, h, hs, vs), (w - 1, h - 1, 1, 1)) == 0


def test_roi_check_refusals(jb):
    d = jb.make_desc(W, H, 2, 2)
    for roi in ((0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (0, 0, 5, -1), (0, 0, -W, -H),      # zero or negative size
                (-1, 0, 5, 5), (0, -1, 5, 5), (-5, -5, 5, 5),                                   # negative origin
                (0, 0, W + 1, H), (0, 0, W, H + 1), (1, 0, W, H), (0, 1, W, H),                 # one pixel past an edge
                (W, 0, 1, 1), (0, H, 1, 1), (W - 1, H - 1, 2, 1), (W - 1, H - 1, 1, 2)):
        assert _rc(jb, d, roi) == -2, roi
    big = 2 ** 31 - 1
    # sums that would wrap in 32 bits: refused, not wrapped -- also against the largest image there is
    for dd in (d, jb.make_desc(65535, 65535, 1, 1)):
        for roi in ((big, 0, 1, 1), (big, 0, 2, 1), (0, big, 1, 1), (0, big, 1, 2), (1, 1, big, big), (big, big, big, big),
                    (2, 0, big, 1), (0, 2, 1, big)):
            assert _rc(jb, dd, roi) == -2, roi
    with pytest.raises(jb.JbError) as e:
        jb.roi_check(d, (0, 0, W + 1, H))
    assert e.value.status == -2


def test_roi_check_descriptor_errors_come_first_and_nulls(jb):
    L = jb.lib()
    good, bad_roi = jb.Roi(0, 0, 1, 1), jb.Roi(-1, -1, 0, 0)
    for roi in (good, bad_roi):
        assert L.jb_roi_check(ctypes.byref(jb.make_desc(0, 5, 1, 1)), ctypes.byref(roi)) == -2     # geometry
        assert L.jb_roi_check(ctypes.byref(jb.make_desc(65536, 5, 1, 1)), ctypes.byref(roi)) == -2
        assert L.jb_roi_check(ctypes.byref(jb.make_desc(16, 16, 3, 1)), ctypes.byref(roi)) == -3   # sampling
        assert L.jb_roi_check(ctypes.byref(jb.make_desc(16, 16, 1, 4)), ctypes.byref(roi)) == -3
        assert L.jb_roi_check(ctypes.byref(jb.make_desc(16, 16, 1, 1, (0, 4, 1))), ctypes.byref(roi)) == -4   # table id
    d = jb.make_desc(16, 16, 1, 1)
    assert L.jb_roi_check(None, ctypes.byref(good)) == -1
    assert L.jb_roi_check(ctypes.byref(d), None) == -1
    assert L.jb_roi_check(None, None) == -1


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_roi_output_sizes_are_those_of_a_w_by_h_image(jb, fmt):
    for w, h in ((1, 1), (224, 224), (3, 45), (1099, 45), (65535, 2)):
        assert jb.output_bytes(w, h, fmt) == 3 * w * h * ESIZE[fmt]


def test_roi_with_a_scale_is_refused_before_any_device_call(jb):
    """The wrapper raises JbError(-9) for roi= with scale=2 itself: nothing here has a context, a decoder, a device or
    a library handle to call into (ctx is a bare object)."""
    ctx = object.__new__(jb.Context)
    ctx._h = ctypes.c_void_p()
    for call in (lambda: ctx.blocks_to_rgb_device(jb.DeviceBatch(), scale=2, roi=(0, 0, 8, 8)),
                 lambda: ctx.decode_file("/nonexistent.jpg", scale=2, roi=(0, 0, 8, 8)),
                 lambda: ctx.decode_memory(b"", scale=2, roi=(0, 0, 8, 8)),
                 lambda: ctx.decode_memory(b"", scale=8, fmt=1, roi=jb.Roi(0, 0, 8, 8)),
                 lambda: jb.BatchDecoder(2, 0, scale=2, roi=(0, 0, 8, 8)),
                 lambda: jb.torch_batch(jb.make_desc(16, 16, 1, 1), 1, None, None, None, scale=2, roi=(0, 0, 8, 8))):
        with pytest.raises(jb.JbError) as e:
            call()
        assert e.value.status == -9
