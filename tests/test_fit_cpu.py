"""Fit without a GPU: jb_fit_check's geometry against tests/fit_ref.py and against live Pillow (ImageOps.pad), its refusals
in their order, the binding's request and route, and the body of the fill kernel on the CPU under sanitizers
(tools/fuzz/fit_kernel_check, a stand-alone program)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fit_ref
import pillow_resize_ref as pr
from conftest import ROOT


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


ANCHORS = (fit_ref.CENTER, fit_ref.START, fit_ref.END)


def _geometry(jb, w, h, target, mode, anchor, roi=None):
    return jb.fit_geometry(w, h, target, jb.Fit(mode, anchor), roi=roi)


def test_constants_and_struct(jb):
    assert (jb.FIT_STRETCH, jb.FIT_PAD, jb.FIT_COVER) == (0, 1, 2) and (jb.FIT_CENTER, jb.FIT_START, jb.FIT_END) == (0, 1, 2)
    assert ctypes.sizeof(jb.Fit) == 16 and [f[0] for f in jb.Fit._fields_] == ["mode", "anchor", "fill", "reserved8", "reserved"]
    assert ctypes.sizeof(jb.FitGeometry) == 32
    f = jb.Fit.pad((124, 116, 104), jb.FIT_END)
    assert (f.mode, f.anchor, list(f.fill), f.reserved8, f.reserved) == (1, 2, [124, 116, 104], 0, 0)
    f = jb.Fit.cover()
    assert (f.mode, f.anchor, list(f.fill)) == (2, 0, [0, 0, 0])
    for name in ("jb_fit_check", "jb_blocks_to_rgb_device_fit", "jb_decode_memory_fit", "jb_decode_file_fit", "jb_batch_decoder_set_fit"):
        assert hasattr(jb.lib(), name), name


def test_named_geometries(jb):
    # equal aspect: nothing pads, nothing is cut
    for mode in (1, 2):
        assert _geometry(jb, 32, 48, (16, 24), mode, 0) == ((0, 0, 32, 48), (0, 0, 16, 24))
    # a border of 1, 3 and 5 rows: round-half-even puts 0, 2 and 2 of them in front
    for sh, dh, off in ((15, 15, 0), (13, 13, 2), (11, 11, 2)):
        assert _geometry(jb, 16, sh, (16, 16), 1, jb.FIT_CENTER) == ((0, 0, 16, sh), (0, off, 16, dh))
        assert _geometry(jb, sh, 16, (16, 16), 1, jb.FIT_CENTER) == ((0, 0, sh, 16), (off, 0, dh, 16))
        assert _geometry(jb, 16, sh, (16, 16), 1, jb.FIT_START)[1] == (0, 0, 16, dh)
        assert _geometry(jb, 16, sh, (16, 16), 1, jb.FIT_END)[1] == (0, 16 - dh, 16, dh)
    # an extent that rounds to 0 is raised to 1 (Pillow raises an error there)
    assert _geometry(jb, 64, 1, (8, 8), 1, 0) == ((0, 0, 64, 1), (0, 4, 8, 1))
    assert _geometry(jb, 1, 64, (8, 8), 1, 0) == ((0, 0, 1, 64), (4, 0, 1, 8))
    # the issue's headline shape
    assert _geometry(jb, 1920, 1080, (224, 224), 1, 0) == ((0, 0, 1920, 1080), (0, 49, 224, 126))
    assert _geometry(jb, 1920, 1080, (224, 224), 2, 0) == ((420, 0, 1080, 1080), (0, 0, 224, 224))
    assert _geometry(jb, 1920, 1080, (224, 224), 2, jb.FIT_START)[0] == (0, 0, 1080, 1080)
    assert _geometry(jb, 1920, 1080, (224, 224), 2, jb.FIT_END)[0] == (840, 0, 1080, 1080)
    # cover of a rectangle stays inside the rectangle
    assert _geometry(jb, 100, 50, (8, 8), 2, 0, roi=(10, 5, 37, 23)) == ((17, 5, 23, 23), (0, 0, 8, 8))
    # stretch, as None, as a number and as a struct: the source and the whole target
    for fit in (None, 0, jb.Fit(0, 0)):
        assert jb.fit_geometry(37, 23, (16, 16), fit, roi=(1, 2, 30, 20)) == ((1, 2, 30, 20), (0, 0, 16, 16))


def test_geometry_sweep_against_the_reference(jb):
    rng = np.random.default_rng(20260)
    n = 0
    for _ in range(400):
        fw, fh, W, H = (int(v) for v in rng.integers(1, 120, 4))
        roi = None
        if rng.random() < 0.5:
            rw, rh = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
            roi = (int(rng.integers(0, fw - rw + 1)), int(rng.integers(0, fh - rh + 1)), rw, rh)
        source = roi if roi is not None else (0, 0, fw, fh)
        for mode in (fit_ref.PAD, fit_ref.COVER):
            for anchor in ANCHORS:
                got = _geometry(jb, fw, fh, (W, H), mode, anchor, roi)
                want = fit_ref.geometry(source, (W, H), mode, anchor)
                assert got == want, (fw, fh, roi, W, H, mode, anchor)
                (sx, sy, sw, sh), (ix, iy, iw, ih) = got
                assert source[0] <= sx and source[1] <= sy and sx + sw <= source[0] + source[2] and sy + sh <= source[1] + source[3]
                assert 0 <= ix and 0 <= iy and iw >= 1 and ih >= 1 and ix + iw <= W and iy + ih <= H
                assert mode == fit_ref.COVER or (iw == W or ih == H)     # only one axis pads
                n += 1
    assert n == 2400


@pytest.mark.parametrize("filt", [pr.FILTER_BILINEAR, pr.FILTER_BICUBIC])
def test_geometry_and_pixels_equal_live_pillow(jb, filt):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    method = {pr.FILTER_BILINEAR: Image.BILINEAR, pr.FILTER_BICUBIC: Image.BICUBIC}[filt]
    rng = np.random.default_rng(31 + filt)
    fill = (124, 116, 104)
    cases = [(37, 23, 16, 16), (23, 37, 16, 16), (37, 23, 15, 16), (23, 37, 16, 13), (16, 15, 16, 16), (16, 13, 16, 16), (16, 11, 16, 16),
             (32, 48, 16, 24), (5, 9, 40, 31)]
    cases += [tuple(int(v) for v in rng.integers(1, 60, 4)) for _ in range(30)]
    compared = 0
    for w, h, W, H in cases:
        full = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        (_, (ix, iy, iw, ih)) = fit_ref.geometry((0, 0, w, h), (W, H), fit_ref.PAD)
        if round(h / w * W) == 0 or round(w / h * H) == 0:
            continue                                              # Pillow raises: the contract raises the extent to 1
        for anchor, centering in ((fit_ref.CENTER, (0.5, 0.5)), (fit_ref.START, (0.0, 0.0)), (fit_ref.END, (1.0, 1.0))):
            want = np.asarray(ImageOps.pad(Image.fromarray(full), (W, H), method, color=fill, centering=centering))
            ref = fit_ref.fit_u8(full, None, (W, H), fit_ref.PAD, anchor, fill, filt)
            assert np.array_equal(ref, want), (w, h, W, H, anchor)
            # the geometry the library reports is where Pillow's picture lies: everything outside it is the fill
            (_, (ix, iy, iw, ih)) = jb.fit_geometry(w, h, (W, H), jb.Fit.pad(fill, anchor), filter=filt)
            mask = np.ones((H, W), bool)
            mask[iy:iy + ih, ix:ix + iw] = False
            assert (want[mask] == np.asarray(fill, np.uint8)).all(), (w, h, W, H, anchor)
            assert np.array_equal(want[iy:iy + ih, ix:ix + iw], np.asarray(Image.fromarray(full).resize((iw, ih), method))), (w, h, W, H, anchor)
            compared += 1
    assert compared >= 90


def _check(jb, desc, roi, rs, fit, out=True):
    g = jb.FitGeometry()
    return jb.lib().jb_fit_check(ctypes.byref(desc) if desc is not None else None, ctypes.byref(jb.Roi(*roi)) if roi is not None else None,
                                 ctypes.byref(jb.Resize(*rs)) if rs is not None else None, ctypes.byref(fit) if fit is not None else None,
                                 ctypes.byref(g) if out else None)


def test_fit_check_statuses_in_order(jb):
    d = jb.make_desc(40, 24, 2, 2)
    T = (8, 8, 0, 0)
    pad, cover = jb.Fit.pad(), jb.Fit.cover()
    bad_mode, bad_anchor = jb.Fit(3, 0), jb.Fit(1, 3)
    bad_r8, bad_r = jb.Fit.pad(), jb.Fit.cover()
    bad_r8.reserved8, bad_r.reserved = 1, 1
    for fit in (None, pad, cover, jb.Fit(0, 0)):
        assert _check(jb, d, None, T, fit) == 0
        assert _check(jb, d, (1, 2, 30, 20), (8, 8, 2, 0), fit, out=False) == 0
    # null arguments, then the descriptor's own errors, whatever else is wrong
    assert _check(jb, None, None, T, bad_mode) == -1
    assert _check(jb, d, None, None, bad_mode) == -1
    assert _check(jb, jb.make_desc(40, 24, 3, 1), (0, 0, 99, 99), T, bad_mode) == -3
    assert _check(jb, jb.make_desc(0, 24, 2, 2), None, T, bad_mode) == -2
    # the rectangle, the target and the filter come before the fit
    assert _check(jb, d, (0, 0, 41, 24), (0, 0, 0, 0), pad) == -2
    assert _check(jb, d, None, (0, 5, 0, 0), pad) == -2
    assert _check(jb, d, None, (8, 8, 3, 0), pad) == -2
    assert _check(jb, d, None, (8, 8, 0, 1), pad) == -2
    assert _check(jb, d, None, (0, 0, 1, 0), bad_mode) == -7             # "a filter wants a target size" is an older refusal
    # the fit's own: unknown mode, anchor, reserved fields
    for fit in (bad_mode, jb.Fit(-1, 0), bad_anchor, jb.Fit(2, -1), bad_r8, bad_r):
        assert _check(jb, d, None, T, fit) == -2
        assert _check(jb, d, None, (8, 8, 2, 0), fit) == -2
    # then a mode without a target size
    for fit in (pad, cover):
        assert _check(jb, d, None, (0, 0, 0, 0), fit) == -7
        assert _check(jb, d, None, (0, 0, 2, 0), fit) == -7
    assert _check(jb, d, None, (0, 0, 0, 0), jb.Fit(0, 0)) == -2          # (stretch: jb_filter_check's answer for no size)
    # the tap cap is that of the pair that is resampled: a 4000 x 30 frame to 8 x 8 reduces 500-fold stretched and
    # letterboxed, and 3.75-fold once the centred 30 x 30 square is cut
    wide = jb.make_desc(4000, 30, 2, 2)
    assert _check(jb, wide, None, (8, 8, 2, 0), None) == -9
    assert _check(jb, wide, None, (8, 8, 2, 0), pad) == -9
    assert _check(jb, wide, None, (8, 8, 2, 0), cover) == 0
    assert _check(jb, wide, None, (8, 8, 2, 0), bad_mode) == -9          # (a fit that is none is a stretch until it is refused)
    assert jb.fit_geometry(4000, 30, (8, 8), jb.FIT_COVER, filter=2) == ((1985, 0, 30, 30), (0, 0, 8, 8))


def test_fit_geometry_of_the_binding_raises(jb):
    with pytest.raises(jb.JbError) as e:
        jb.fit_geometry(40, 24, (8, 8), 3)
    assert e.value.status == -2
    with pytest.raises(jb.JbError) as e:
        jb.fit_geometry(40, 24, None, jb.FIT_PAD)
    assert e.value.status == -7
    with pytest.raises(jb.JbError) as e:
        jb.fit_geometry(40, 24, (8, 8), jb.FIT_PAD, roi=(0, 0, 41, 1))
    assert e.value.status == -2


def test_request_fit(jb):
    from jpeg_decoder_amd import api
    assert api._ROUTES["fit"] == ("jb_decode_file_fit", "jb_decode_memory_fit", "jb_blocks_to_rgb_device_fit")
    q = api._Request(resize=(8, 9), roi=(1, 2, 3, 4), filter=jb.FILTER_BICUBIC, fmt=3, fit=jb.Fit.pad((1, 2, 3)))
    route, tail = q.routed()
    assert route == "fit" and len(tail) == 4 and q.fit.mode == jb.FIT_PAD and list(q.fit.fill) == [1, 2, 3]
    assert api._Request(resize=(8, 9), fit=jb.FIT_COVER).routed()[0] == "fit"        # the area filter takes the same route
    # None and FIT_STRETCH route exactly as before
    for kw, route in ((dict(), "plain"), (dict(scale=2), "scaled"), (dict(fmt=3), "fmt"), (dict(roi=(0, 0, 1, 1)), "roi"),
                      (dict(resize=(8, 9)), "resized"), (dict(resize=(8, 9), filter=1), "filtered"),
                      (dict(resize=(8, 9), crops=[(0, 0, 1, 1)]), "crops"), (dict(resize=(8, 9), crops=[(0, 0, 1, 1)], filter=2), "crops_filtered"),
                      (dict(resize=(8, 9), views=[[(0, 0, 1, 1)]]), "views")):
        for fit in (None, jb.FIT_STRETCH, jb.Fit(0, 0)):
            q = api._Request(fit=fit, **kw)
            assert q.fit is None and q.routed()[0] == route == api._Request(**kw).routed()[0], (kw, fit)
    # the refusals, behind the older ones and before any C call
    for fit in (jb.FIT_PAD, jb.Fit.cover()):
        for kw, status in ((dict(), -7), (dict(roi=(0, 0, 1, 1)), -7), (dict(resize=(8, 9), crops=[(0, 0, 1, 1)]), -9),
                           (dict(resize=(8, 9), views=[[(0, 0, 1, 1)]]), -9), (dict(scale=2, resize=(8, 9)), -9), (dict(crops=[(0, 0, 1, 1)]), -7),
                           (dict(filter=1), -7)):
            with pytest.raises(jb.JbError) as e:
                api._Request(fit=fit, **kw)
            assert e.value.status == status, kw


def test_fill_kernel_body_under_sanitizers():
    """tools/fuzz/fit_kernel_check: the body of jb_fit_fill_kernel on the CPU -- formats 0-3 x bands above and below, left and
    right, on one side only, one element wide, longer than a workgroup, and no border at all x one image and a batch of
    three with odd pads -- into exactly-sized sentinel-filled buffers, under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "fit_kernel_check"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "fit_kernel_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) >= 4 * 12 * 2, r.stdout
