"""Resampling filters, host side (no GPU): the numpy restatement (pillow_resize_ref.py) against Pillow's own bits -- the
recorded ones of tests/golden/pillow_resize_kat.npz everywhere, Pillow itself where it imports --, jb_filter_window against
the restatement's bounds, jb_filter_check and the plan's new refusals in their order, and the Python request's routing."""
import ctypes
import os

import numpy as np
import pytest

import pillow_resize_ref as pr
from conftest import GOLD

BILINEAR, BICUBIC = pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
CAP = 160    # include/jpegblk.h: the taps of one axis, counted as floor(2 * sup) + 2


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


# ---- the restatement against Pillow ----------------------------------------------------------------------------------
def test_restatement_equals_every_recorded_pillow_case():
    z = np.load(os.path.join(GOLD, "pillow_resize_kat.npz"))
    n = int(z["n"])
    assert n >= 20 and str(z["pillow_version"])
    for k in range(n):
        x, y, w, h, ow, oh, filt = (int(v) for v in z[f"meta_{k}"])
        got = pr.resize(z[f"full_{k}"], (x, y, w, h), (ow, oh), filt)
        assert np.array_equal(got, z[f"out_{k}"]), (k, (x, y, w, h), (ow, oh), filt)


def _frame(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)   # bicubic's overshoot: both clamps


def _rects(W, H):
    return [(0, 0, W, H),                          # the whole frame
            (W // 4, H // 4, W // 2, H // 2),      # interior
            (0, 7, 30, 21), (W - 30, 5, 30, 21),   # touching the left / the right edge
            (9, 0, 30, 21), (11, H - 21, 30, 21),  # touching the top / the bottom edge
            (W // 3, H // 3, 9, 9),                # (for the 9 x 9 -> 33 x 20 enlargement)
            (W // 2, H // 2, 1, 1)]                # 1 x 1


def _targets(rect):
    x, y, w, h = rect
    return [(w, h), (1, 1), (max(w // 3, 1), max(h // 4, 1)), (33, 20), (max(w // 2, 1), 2 * h + 1)]


@pytest.mark.parametrize("W,H", [(67, 45), (130, 97)])
@pytest.mark.parametrize("kind", ["noise", "binary"])
def test_restatement_equals_pillow(W, H, kind):
    Image = pytest.importorskip("PIL.Image")
    full = _frame(W, H, kind, W + H)
    pil = Image.fromarray(full)
    for rect in _rects(W, H):
        x, y, w, h = rect
        for target in _targets(rect):
            for filt, resample in ((BILINEAR, Image.BILINEAR), (BICUBIC, Image.BICUBIC)):
                want = np.asarray(pil.resize(target, resample, box=(x, y, x + w, y + h)))
                assert np.array_equal(pr.resize(full, rect, target, filt), want), (rect, target, filt)


def test_restatement_identity_and_margin():
    full = _frame(67, 45, "noise", 3)
    for filt in (BILINEAR, BICUBIC):
        assert np.array_equal(pr.resize(full, (5, 6, 40, 30), (40, 30), filt), full[6:36, 5:45])
        # the filter reads outside the rectangle: crop-then-resize is another image
        assert not np.array_equal(pr.resize(full, (20, 12, 30, 20), (11, 9), filt), pr.resize_rect_clamped(full, (20, 12, 30, 20), (11, 9), filt))


def test_restatement_without_a_clamp_is_another_image():
    """mid_clamp / out_clamp restate a kernel that lost a clamp (for the GPU tests' preconditions): on a 0 / 255 image
    bicubic's overshoot makes each of them another image, bilinear -- no negative weight -- never leaves 0..255, and the
    defaults are the definition."""
    full = _frame(67, 45, "binary", 7)
    for rect, target in (((5, 6, 40, 30), (41, 33)), (None, (100, 70))):
        for filt in (BILINEAR, BICUBIC):
            want = pr.resize(full, rect, target, filt)
            assert np.array_equal(pr.resize(full, rect, target, filt, mid_clamp="clip", out_clamp="clip"), want)
            lost = [pr.resize(full, rect, target, filt, mid_clamp="none"), pr.resize(full, rect, target, filt, out_clamp="wrap")]
            assert all(x.dtype == np.uint8 and x.shape == want.shape for x in lost)
            assert all(np.array_equal(x, want) == (filt == BILINEAR) for x in lost), (rect, target, filt)


# ---- jb_filter_window ------------------------------------------------------------------------------------------------
def _rs(jb, target, filt, reserved=0):
    return jb.Resize(target[0], target[1], filt, reserved)


def _taps(filt, n_in, n_out):
    """the taps of an axis as the header's cap counts them"""
    scale = n_in / n_out
    return int(2.0 * ((2.0 if filt == BICUBIC else 1.0) * (1.0 if scale < 1.0 else scale))) + 2


@pytest.mark.parametrize("W,H", [(67, 45), (130, 97)])
def test_filter_window_is_the_union_of_the_bounds(jb, W, H):
    d = jb.make_desc(W, H, 2, 2)
    n_windows = 0
    for rect in _rects(W, H):
        for target in _targets(rect):
            for filt in (BILINEAR, BICUBIC):
                want = pr.window(filt, W, H, rect, target)
                if max(_taps(filt, rect[2], target[0]), _taps(filt, rect[3], target[1])) > CAP:
                    with pytest.raises(jb.JbError) as e:      # (beyond the kernel's cap there is no request to have a window)
                        jb.filter_window(d, target, filt, roi=rect)
                    assert e.value.status == -9
                    continue
                n_windows += 1
                assert jb.filter_window(d, target, filt, roi=rect) == want, (rect, target, filt)
                x, y, w, h = want      # it holds the rectangle and lies in the frame
                assert x <= rect[0] and y <= rect[1] and x + w >= rect[0] + rect[2] and y + h >= rect[1] + rect[3]
                assert x >= 0 and y >= 0 and x + w <= W and y + h <= H
            assert jb.filter_window(d, target, jb.FILTER_AREA, roi=rect) == rect
    assert n_windows >= 2 * 5 * 8 - 6      # (the whole 130 x 97 frame to 1 x 1, and 67 x 45 under bicubic, are over the cap)
    assert jb.filter_window(d, (20, 10), BICUBIC) == pr.window(BICUBIC, W, H, (0, 0, W, H), (20, 10)) == (0, 0, W, H)


# ---- jb_filter_check and the plan's refusals ---------------------------------------------------------------------------
def _fc(jb, d, roi, target, filt, reserved=0):
    return jb.lib().jb_filter_check(ctypes.byref(d), ctypes.byref(jb.Roi(*roi)) if roi is not None else None,
                                    ctypes.byref(_rs(jb, target, filt, reserved)))


def test_filter_check_accepts_and_refuses_in_order(jb):
    L = jb.lib()
    d = jb.make_desc(679, 451, 2, 2)
    for filt in (0, 1, 2):
        assert _fc(jb, d, None, (224, 224), filt) == 0
        assert _fc(jb, d, (5, 3, 30, 24), (1, 1), filt) == 0
        assert _fc(jb, d, (5, 3, 50, 40), (65535, 65535), filt) == 0
    # the new refusals
    for filt in (-1, 3, 7, 2 ** 31 - 1):
        assert _fc(jb, d, None, (8, 8), filt) == -2, filt             # unknown filter
    for filt in (0, 1, 2):
        assert _fc(jb, d, None, (8, 8), filt, reserved=1) == -2       # reserved
    for filt in (1, 2):
        assert _fc(jb, d, None, (0, 0), filt) == -7                   # a filter and no target size
    assert _fc(jb, d, None, (0, 0), 0) == -2                          # (filter 0: what jb_resize_check says of (0, 0))
    assert L.jb_resize_check(ctypes.byref(d), None, 0, 0) == -2
    # the order: the descriptor, the rectangle, the target's size before the filter's own
    assert _fc(jb, jb.make_desc(16, 16, 3, 1), (-1, 0, 1, 1), (0, 5), 9) == -3
    assert _fc(jb, d, (0, 0, 680, 4), (0, 5), 9) == -2
    assert _fc(jb, d, None, (0, 5), 1) == -2 and _fc(jb, d, None, (70000, 5), 2) == -2
    assert _fc(jb, d, None, (0, 0), 9) == -2                          # unknown filter before "no target size"
    big = jb.make_desc(8000, 8000, 1, 1)
    assert _fc(jb, big, None, (10, 10), 9) == -2                      # unknown filter before the cap
    assert _fc(jb, big, None, (10, 10), 1, reserved=2) == -2
    # null pointers
    assert L.jb_filter_check(None, None, ctypes.byref(_rs(jb, (8, 8), 1))) == -1
    assert L.jb_filter_check(ctypes.byref(d), None, None) == -1
    assert L.jb_filter_window(ctypes.byref(d), None, ctypes.byref(_rs(jb, (8, 8), 1)), None) == -1
    win = jb.Roi()
    assert L.jb_filter_window(ctypes.byref(d), None, ctypes.byref(_rs(jb, (0, 0), 1)), ctypes.byref(win)) == -7
    with pytest.raises(jb.JbError) as e:
        jb.filter_check(d, (8, 8), 5)
    assert e.value.status == -2
    jb.filter_check(d, (8, 8), BICUBIC, roi=(1, 1, 100, 100))


def test_tap_cap(jb):
    """The header's cap: an axis counts floor(2 * sup) + 2 taps, sup = S * max(scale, 1), and more than 160 is refused.
    The largest reduction that passes and the smallest that does not, per filter and per axis, from that formula."""
    d = jb.make_desc(20000, 20000, 1, 1)
    for filt, S in ((BILINEAR, 1), (BICUBIC, 2)):
        n = 10
        ok = (CAP - 2) * n // (2 * S)             # floor(2 * S * ok / n) + 2 == CAP
        assert int(2.0 * (S * (ok / n))) + 2 == CAP and int(2.0 * (S * ((ok + n) / n))) + 2 > CAP
        assert _fc(jb, d, (0, 0, ok, 50), (n, 50), filt) == 0
        assert _fc(jb, d, (0, 0, 50, ok), (50, n), filt) == 0
        assert _fc(jb, d, (3, 5, ok + n, 50), (n, 50), filt) == -9
        assert _fc(jb, d, (3, 5, 50, ok + n), (50, n), filt) == -9
        assert _fc(jb, d, (0, 0, 32 * n, 32 * n), (n, n), filt) == 0        # a 32x reduction always passes
        assert _fc(jb, d, (3, 5, ok + n, 50), (n, 50), 0) == 0              # the area filter has no cap
    with pytest.raises(jb.JbError) as e:
        jb.filter_check(d, (10, 10), BICUBIC)
    assert e.value.status == -9
    assert jb.lib().jb_blocks_to_rgb_device_crops_filtered(None, None, None, None, None, None) == -1


# ---- the Python request ----------------------------------------------------------------------------------------------
def test_filter_area_routes_to_todays_calls(jb):
    from jpeg_decoder_amd.api import _Request, _ROUTES
    crops = [(0, 0, 4, 4), (1, 1, 2, 2)]
    for kw in (dict(), dict(scale=2), dict(fmt=3), dict(roi=(0, 0, 8, 8)), dict(resize=(8, 6)), dict(roi=(1, 1, 5, 5), resize=(8, 6), fmt=1),
               dict(resize=(8, 6), crops=crops)):
        a, b = _Request(**kw), _Request(filter=jb.FILTER_AREA, **kw)
        (ra, ta), (rb, tb) = a.routed(), b.routed()
        assert ra == rb and len(ta) == len(tb) and "filtered" not in ra
        assert [type(v) for v in ta] == [type(v) for v in tb]
        assert [v for v in ta if isinstance(v, int)] == [v for v in tb if isinstance(v, int)]
    assert _Request(resize=(8, 6)).routed()[0] == "resized" and _Request(resize=(8, 6), crops=crops).routed()[0] == "crops"
    # the filtered routes
    route, tail = _Request(fmt=3, roi=(1, 2, 3, 4), resize=(8, 6), filter=jb.FILTER_BICUBIC).routed()
    assert route == "filtered" and len(tail) == 3
    rs = tail[1]._obj
    assert (rs.out_w, rs.out_h, rs.filter, rs.reserved) == (8, 6, 2, 0) and tail[0]._obj.width == 3
    route, tail = _Request(resize=(8, 6), crops=crops, filter=jb.FILTER_BILINEAR).routed()
    assert route == "crops_filtered" and tail[0][1].width == 2 and tail[1]._obj.filter == 1 and tail[2] is None
    assert _ROUTES["filtered"] == ("jb_decode_file_filtered", "jb_decode_memory_filtered", "jb_blocks_to_rgb_device_filtered")
    assert _ROUTES["crops_filtered"] == (None, None, "jb_blocks_to_rgb_device_crops_filtered")
    for name in _ROUTES["filtered"] + ("jb_blocks_to_rgb_device_crops_filtered", "jb_batch_decoder_set_filter", "jb_filter_check", "jb_filter_window"):
        assert hasattr(jb.lib(), name), name


def test_filter_without_a_target_is_refused_before_any_device_call(jb):
    ctx = object.__new__(jb.Context)
    ctx._h = ctypes.c_void_p()
    for call in (lambda: ctx.blocks_to_rgb_device(jb.DeviceBatch(), filter=jb.FILTER_BILINEAR),
                 lambda: ctx.decode_file("/nonexistent.jpg", filter=jb.FILTER_BICUBIC),
                 lambda: ctx.decode_memory(b"", roi=(0, 0, 4, 4), filter=jb.FILTER_BICUBIC),
                 lambda: jb.BatchDecoder(2, 0, filter=jb.FILTER_BILINEAR),
                 lambda: jb.torch_batch(jb.make_desc(16, 16, 1, 1), 1, None, None, None, filter=jb.FILTER_BILINEAR)):
        with pytest.raises(jb.JbError) as e:
            call()
        assert e.value.status == -7
    with pytest.raises(jb.JbError) as e:     # a filter changes nothing about a scale's refusal
        ctx.decode_memory(b"", scale=2, resize=(8, 8), filter=jb.FILTER_BILINEAR)
    assert e.value.status == -9
    assert jb.lib().jb_batch_decoder_set_filter(None, 1) == -1
