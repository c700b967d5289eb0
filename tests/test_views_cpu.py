"""Views without a GPU: jb_views_check's refusals in their order, the binding's request and route, random_views, and the
bodies of both view kernels on the CPU under sanitizers (tools/fuzz/views_kernel_check, a stand-alone program)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


def _check(jb, desc, views, n, k, resize, filt=0, reserved=0, null=False):
    """-> (status, bad_index) of jb_views_check; views: a flat list of (x, y, w, h, flags, reserved)"""
    arr = (jb.View * max(len(views), 1))(*[jb.View(*v) for v in views])
    bad = ctypes.c_int(77)
    rs = jb.Resize(resize[0], resize[1], filt, reserved) if resize is not None else None
    rc = jb.lib().jb_views_check(ctypes.byref(desc) if desc is not None else None, None if null else arr, n, k,
                                 ctypes.byref(rs) if rs is not None else None, ctypes.byref(bad))
    return rc, bad.value


W, H = 40, 24
GOOD = [(0, 0, W, H, 0, 0), (39, 23, 1, 1, 1, 0), (3, 2, 20, 10, 1, 0), (0, 0, 1, 1, 0, 0)]     # two images of two views


def test_views_check_statuses_in_order(jb):
    d = jb.make_desc(W, H, 2, 2)
    T = (8, 8)
    assert _check(jb, d, GOOD, 2, 2, T) == (0, -1)
    assert _check(jb, d, GOOD, 2, 2, T, 2) == (0, -1)
    assert _check(jb, d, [], 0, 3, T) == (0, -1)                        # n = 0: the count, the target and the filter alone
    assert _check(jb, d, [], 0, 3, T, null=True) == (0, -1)
    assert _check(jb, d, [], 0, 3, (0, 5)) == (-2, -1)
    # null arguments first
    assert _check(jb, None, GOOD, 2, 2, T) == (-1, -1)
    assert _check(jb, d, GOOD, 2, 2, None) == (-1, -1)
    assert _check(jb, d, GOOD, 2, 2, T, null=True) == (-1, -1)
    # then the descriptor's own errors, whatever else is wrong
    assert _check(jb, jb.make_desc(W, H, 3, 1), GOOD, 2, 17, T)[0] == -3
    assert _check(jb, jb.make_desc(0, H, 2, 2), GOOD, 2, 0, T)[0] == -2
    # then the count
    for k in (0, 17, -1):
        assert _check(jb, d, GOOD, 2, k, (0, 0)) == (-2, -1), k
    assert _check(jb, d, GOOD, -1, 2, T) == (-2, -1)
    assert _check(jb, d, GOOD * 8, 2, 16, T) == (0, -1)
    # then the first view that fails: flags and reserved before any rectangle, with the FLAT index
    outside = list(GOOD)
    outside[0] = (0, 0, W + 1, H, 0, 0)
    flagged = list(outside)
    flagged[2] = (3, 2, 20, 10, 2, 0)                                   # flag bit 1
    assert _check(jb, d, flagged, 2, 2, T) == (-2, 2)
    flagged[2] = (3, 2, 20, 10, 1, 1)                                   # reserved
    assert _check(jb, d, flagged, 2, 2, T) == (-2, 2)
    assert _check(jb, d, outside, 2, 2, (0, 0)) == (-2, 0)              # the rectangle before the target
    # a rectangle one pixel outside the frame, as view 0 and as view K - 1 of the last image
    for at, v in ((0, (1, 0, W, H, 0, 0)), (0, (0, 1, W, H, 1, 0)), (3, (W - 1, H - 1, 2, 1, 0, 0)), (3, (W - 1, H - 1, 1, 2, 0, 0)),
                  (3, (-1, 0, 1, 1, 0, 0)), (3, (0, 0, 0, 1, 0, 0)), (2, (2 ** 31 - 1, 0, 1, 1, 0, 0))):
        bad = list(GOOD)
        bad[at] = v
        assert _check(jb, d, bad, 2, 2, T) == (-2, at), v
        assert _check(jb, d, bad, 1, 4, T) == (-2, at), v
    # then the target and the filter: no target size is JB_ERR_STATE with either kind of filter
    assert _check(jb, d, GOOD, 2, 2, (0, 0)) == (-7, -1)
    assert _check(jb, d, GOOD, 2, 2, (0, 0), 1) == (-7, -1)
    assert _check(jb, d, GOOD, 2, 2, (0, 5)) == (-2, -1)
    assert _check(jb, d, GOOD, 2, 2, (65536, 5)) == (-2, -1)
    assert _check(jb, d, GOOD, 2, 2, T, 3) == (-2, -1)
    assert _check(jb, d, GOOD, 2, 2, T, 0, 1) == (-2, -1)
    assert _check(jb, d, GOOD, 2, 2, (0, 0), 3) == (-2, -1)             # an unknown filter before "no target"
    # the tap cap names the view
    big = jb.make_desc(4000, 30, 2, 2)
    views = [(0, 0, 10, 10, 0, 0), (0, 0, 4000, 30, 1, 0)]
    assert _check(jb, big, views, 1, 2, (8, 8), 0) == (0, -1)
    assert _check(jb, big, views, 1, 2, (8, 8), 2) == (-9, 1)
    assert _check(jb, big, views, 2, 1, (8, 8), 1) == (-9, 1)


def test_views_check_of_the_binding(jb):
    d = jb.make_desc(W, H, 2, 2)
    jb.views_check(d, [[(0, 0, W, H), (39, 23, 1, 1, True)]], (8, 8))
    jb.views_check(d, [[(0, 0, W, H)], [(1, 1, 5, 5, 1)]], (8, 8), jb.FILTER_BICUBIC)
    with pytest.raises(jb.JbError) as e:
        jb.views_check(d, [[(0, 0, W, H), (39, 23, 2, 1)]], (8, 8))
    assert e.value.status == -2 and "view 1" in str(e.value)
    with pytest.raises(jb.JbError) as e:
        jb.views_check(d, [[(0, 0, W, H)] * 17], (8, 8))
    assert e.value.status == -2
    with pytest.raises(jb.JbError) as e:
        jb.views_check(d, [[(0, 0, W, H)]], None)
    assert e.value.status == -7


def test_request_views(jb):
    from jpeg_decoder_amd import api
    assert ctypes.sizeof(jb.View) == 24
    assert [f[0] for f in jb.View._fields_] == ["x", "y", "width", "height", "flags", "reserved"]
    assert jb.VIEW_MIRROR == 1
    views = [[(1, 2, 3, 4), (5, 6, 7, 8, True)], [jb.View(9, 10, 11, 12, 1, 0), (13, 14, 15, 16, 0)]]
    q = api._Request(resize=(8, 9), views=views, filter=jb.FILTER_BILINEAR, fmt=3)
    assert (q.views_per_image, q.n_view_rows, q.target, q.filter) == (2, 2, (8, 9), 1)
    assert [(v.x, v.y, v.width, v.height, v.flags, v.reserved) for v in q.views] == \
        [(1, 2, 3, 4, 0, 0), (5, 6, 7, 8, 1, 0), (9, 10, 11, 12, 1, 0), (13, 14, 15, 16, 0, 0)]
    route, tail = q.routed()
    assert route == "views" and api._ROUTES["views"] == (None, None, "jb_blocks_to_rgb_device_views")
    assert tail[0] is q.views and tail[1] == 2 and len(tail) == 4
    assert api._Request(resize=(8, 9), views=views).routed()[0] == "views"       # the area filter takes the same route
    assert hasattr(jb.lib(), "jb_blocks_to_rgb_device_views")
    # the four refusals, and ragged rows, before any C call
    for kw, status in ((dict(scale=2), -9), (dict(roi=(0, 0, 1, 1), resize=(8, 9)), -9), (dict(crops=[(0, 0, 1, 1)] * 2, resize=(8, 9)), -9),
                       (dict(), -7)):
        with pytest.raises(jb.JbError) as e:
            api._Request(views=views, **kw)
        assert e.value.status == status, kw
    with pytest.raises(jb.JbError) as e:
        api._Request(resize=(8, 9), views=[views[0], views[1][:1]])
    assert e.value.status == -2
    assert api._Request(resize=(8, 9)).views is None


def test_random_views(jb):
    from jpeg_decoder_amd.crops import random_resized_crop, random_views
    d = jb.make_desc(123, 77, 2, 2)
    a = random_views(123, 77, np.random.default_rng(5), 4)
    assert a == random_views(123, 77, np.random.default_rng(5), 4) and len(a) == 4
    assert a != random_views(123, 77, np.random.default_rng(6), 4)
    # per view: random_resized_crop's draws in its order, then one more
    rng = np.random.default_rng(5)
    for v in a:
        assert v[:4] == random_resized_crop(123, 77, rng) and v[4] == (rng.random() < 0.5)
    mirrors = 0
    rng = np.random.default_rng(9)
    for w, h in ((123, 77), (1, 1), (7, 300), (300, 7)):
        d = jb.make_desc(w, h, 1, 1)
        for v in random_views(w, h, rng, 16):
            assert len(v) == 5 and isinstance(v[4], bool)
            assert jb.lib().jb_roi_check(ctypes.byref(d), ctypes.byref(jb.Roi(*v[:4]))) == 0, v
            mirrors += v[4]
        jb.views_check(d, [random_views(w, h, rng, 16)], (8, 8))
    assert 0 < mirrors < 64
    assert not any(v[4] for v in random_views(123, 77, rng, 16, p_mirror=0))
    assert all(v[4] for v in random_views(123, 77, rng, 16, p_mirror=1))
    assert random_views(123, 77, rng, 0) == []


def test_view_kernel_bodies_under_sanitizers():
    """tools/fuzz/views_kernel_check: the bodies of both view kernels on the CPU -- area, bilinear and bicubic x formats
    0-3 x mirror on / off x targets 1x1, 1x5, 64x3, 65x3, 70x9, the last view ending on the scratch's last pixel,
    exactly-sized buffers -- under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "views_kernel_check"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "views_kernel_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) >= 3 * 4 * 5 * 2, r.stdout
