"""Per-image rectangles, host side (no GPU): jb_crops_check's status and the index of the first rectangle that fails,
the Python request's refusals before any device call, and random_resized_crop."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


W, H = 679, 451
GOOD = [(0, 0, W, H), (5, 3, 50, 40), (W - 1, H - 1, 1, 1), (0, H - 1, W, 1)]


def _cc(jb, desc, rois, ow, oh):
    """-> (status, bad index) of jb_crops_check"""
    arr = (jb.Roi * max(len(rois), 1))(*[jb.Roi(*r) for r in rois])
    bad = ctypes.c_int(12345)
    return jb.lib().jb_crops_check(ctypes.byref(desc), arr, len(rois), ow, oh, ctypes.byref(bad)), bad.value


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2), (2, 1), (1, 2)])
def test_crops_check_accepts_good_rectangles_and_none(jb, hs, vs):
    d = jb.make_desc(W, H, hs, vs)
    assert _cc(jb, d, GOOD, 224, 224) == (0, -1)
    assert _cc(jb, d, GOOD * 20, 1, 65535) == (0, -1)     # more than one launch's table holds
    assert _cc(jb, d, [], 224, 224) == (0, -1)            # n = 0
    jb.crops_check(d, GOOD, (224, 224))
    jb.crops_check(d, [], (8, 8))


@pytest.mark.parametrize("bad", [(W - 9, 0, 10, 4),      # x + w one past the width
                                 (3, 3, 0, 4),            # w = 0
                                 (-1, 0, 4, 4)])          # a negative x
@pytest.mark.parametrize("at", [0, 2, 4])
def test_crops_check_names_the_first_bad_rectangle(jb, bad, at):
    d = jb.make_desc(W, H, 2, 2)
    rois = list(GOOD)
    rois.insert(at, bad)
    rois.append((0, 0, W + 1, H))                         # a later bad one is not the one reported
    assert _cc(jb, d, rois, 224, 224) == (-2, at), (bad, at)
    with pytest.raises(jb.JbError) as e:
        jb.crops_check(d, rois, (224, 224))
    assert e.value.status == -2 and str(at) in str(e.value)


def test_crops_check_bad_target_descriptor_and_nulls(jb):
    L = jb.lib()
    d = jb.make_desc(W, H, 2, 2)
    for ow, oh in ((0, 5), (5, 0), (65536, 1), (-1, 4)):
        assert _cc(jb, d, GOOD, ow, oh) == (-2, -1), (ow, oh)       # the target's: no rectangle is to blame
        assert _cc(jb, d, [], ow, oh) == (-2, -1), (ow, oh)
    # the rectangles come before the target
    assert _cc(jb, d, GOOD + [(0, 0, W, H + 1)], 0, 0) == (-2, len(GOOD))
    # the descriptor's own errors come first
    assert _cc(jb, jb.make_desc(0, 5, 1, 1), GOOD, 8, 8) == (-2, -1)
    assert _cc(jb, jb.make_desc(16, 16, 3, 1), [(-1, 0, 0, 0)], 8, 8) == (-3, -1)
    assert _cc(jb, jb.make_desc(16, 16, 1, 1, (0, 4, 1)), [(0, 0, 1, 1)], 8, 8) == (-4, -1)
    one = (jb.Roi * 1)(jb.Roi(0, 0, 1, 1))
    assert L.jb_crops_check(None, one, 1, 8, 8, None) == -1
    assert L.jb_crops_check(ctypes.byref(d), None, 1, 8, 8, None) == -1
    assert L.jb_crops_check(ctypes.byref(d), one, 1, 8, 8, None) == 0     # (bad_index may be NULL)
    assert L.jb_crops_check(ctypes.byref(d), one, -1, 8, 8, None) == -2
    assert L.jb_blocks_to_rgb_device_crops(None, None, None, 8, 8, None, None) == -1
    assert L.jb_batch_decoder_run_crops(None, None, 0, None, None, None, None, None, None) == -1
    assert L.jb_batch_decoder_submit_crops(None, None, 0, None, None, None, None, None, None) == -1


def test_request_refuses_crops_with_roi_scale_or_no_target(jb):
    from jpeg_decoder_amd.api import _Request, _ROUTES
    crops = [(0, 0, 4, 4), (1, 1, 2, 2)]
    with pytest.raises(jb.JbError) as e:
        _Request(roi=(0, 0, 8, 8), resize=(8, 8), crops=crops)
    assert e.value.status == -9
    with pytest.raises(jb.JbError) as e:
        _Request(scale=2, crops=crops)
    assert e.value.status == -9
    with pytest.raises(jb.JbError):
        _Request(crops=crops)                               # no resize: nothing makes the outputs one size
    with pytest.raises(jb.JbError) as e:                    # and through the public method, before any device call
        jb.Context.blocks_to_rgb_device(None, jb.DeviceBatch(), crops=crops, roi=(0, 0, 8, 8), resize=(8, 8))
    assert e.value.status == -9
    q = _Request(fmt=3, resize=(8, 6), crops=crops)
    route, tail = q.routed()
    assert route == "crops" and q.n_crops == 2 and tail[1:3] == (8, 6)
    assert (q.crops[1].x, q.crops[1].y, q.crops[1].width, q.crops[1].height) == (1, 1, 2, 2)
    assert _ROUTES["crops"][:2] == (None, None) and _ROUTES["crops"][2] == "jb_blocks_to_rgb_device_crops"


SIZES = [(1, 1), (1, 500), (4096, 3), (500, 1), (2, 2), (224, 224), (679, 451), (1920, 1080), (65535, 65535), (7, 4000)]


def test_random_resized_crop_lies_in_the_image_and_is_reproducible(jb):
    from jpeg_decoder_amd.crops import random_resized_crop
    assert jb.random_resized_crop is random_resized_crop
    rng = np.random.default_rng(2024)
    got = []
    for k in range(10000):
        w, h = SIZES[k % len(SIZES)]
        x, y, cw, ch = r = random_resized_crop(w, h, rng)
        assert all(isinstance(v, int) for v in r), r
        assert x >= 0 and y >= 0 and cw >= 1 and ch >= 1 and x + cw <= w and y + ch <= h, (w, h, r)
        got.append(r)
    rng = np.random.default_rng(2024)
    again = [random_resized_crop(*SIZES[k % len(SIZES)], rng) for k in range(10000)]
    assert again == got
    assert len(set(got[5::len(SIZES)])) > 900                  # (224 x 224: they do vary)
    # what the library itself says about them, for a sample
    for k in range(0, 10000, 97):
        w, h = SIZES[k % len(SIZES)]
        d = jb.make_desc(w, h, 2, 2)
        assert jb.lib().jb_roi_check(ctypes.byref(d), ctypes.byref(jb.Roi(*got[k]))) == 0, (w, h, got[k])
    # the usual parameters: within the area share and, before rounding, the ratio bounds, on a roomy image
    rng = np.random.default_rng(7)
    for _ in range(2000):
        x, y, cw, ch = random_resized_crop(1000, 1000, rng)
        assert 0.079 * 1e6 <= cw * ch <= 1.001 * 1e6 and 0.74 <= cw / ch <= 1.34, (cw, ch)
    # the fallback: nothing of the ten draws fits a 4096 x 3 strip at scale (1, 1) -- the centre crop, ratio clamped to 4/3
    assert random_resized_crop(4096, 3, np.random.default_rng(1), scale=(1.0, 1.0)) == (2046, 0, 4, 3)
    assert random_resized_crop(3, 4096, np.random.default_rng(1), scale=(1.0, 1.0)) == (0, 2046, 3, 4)
