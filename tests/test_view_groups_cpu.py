"""View groups without a GPU: the two structs, jb_view_groups_check against a restatement that asks the existing
jb_views_check group by group (seeded random requests), G = 1 against jb_views_check itself, every structural refusal in
its order, jb_view_groups_bytes against jb_output_bytes, the binding's request and route, random_multicrop, and the
kViewGroups instantiations of both view kernels on the CPU under sanitizers (tools/fuzz/view_groups_kernel_check, a
stand-alone program)."""
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


def _views(jb, views):
    return (jb.View * max(len(views), 1))(*[jb.View(*v) for v in views])


def _groups(jb, groups):
    """groups: [(k, (w, h), filter, rs.reserved, reserved), ...]"""
    return (jb.ViewGroup * max(len(groups), 1))(*[jb.ViewGroup(jb.Resize(g[1][0], g[1][1], g[2], g[3]), g[0], g[4]) for g in groups])


def _check(jb, desc, views, n, groups, n_groups=None, null=()):
    """-> (status, bad_index) of jb_view_groups_check; views: a flat list of (x, y, w, h, flags, reserved)"""
    bad = ctypes.c_int(77)
    rc = jb.lib().jb_view_groups_check(None if "desc" in null else ctypes.byref(desc), None if "views" in null else _views(jb, views), n,
                                       None if "groups" in null else _groups(jb, groups), len(groups) if n_groups is None else n_groups,
                                       ctypes.byref(bad))
    return rc, bad.value


def _views_check(jb, desc, views, n, k, g):
    bad = ctypes.c_int(77)
    rc = jb.lib().jb_views_check(ctypes.byref(desc), _views(jb, views), n, k, ctypes.byref(jb.Resize(g[1][0], g[1][1], g[2], g[3])), ctypes.byref(bad))
    return rc, bad.value


def _restated(jb, desc, views, n, groups):
    """The contract of include/jpegblk.h, "view groups", written out: the counts, every view's flags and reserved, every
    rectangle, then group by group what jb_views_check says for that group's views alone."""
    geo = jb.Geometry()
    rc = jb.lib().jb_geometry_of(ctypes.byref(desc), ctypes.byref(geo))
    if rc:
        return rc, -1
    if n < 0 or not 1 <= len(groups) <= 4:
        return -2, -1
    if any(g[0] < 1 or g[4] != 0 for g in groups):
        return -2, -1
    K = sum(g[0] for g in groups)
    if K > 16:
        return -2, -1
    for i, v in enumerate(views[:n * K]):
        if (v[4] & ~1) or v[5]:
            return -2, i
    for i, (x, y, w, h, _, _) in enumerate(views[:n * K]):
        if x < 0 or y < 0 or w < 1 or h < 1 or x + w > desc.width or y + h > desc.height:
            return -2, i
    first = 0
    for g in groups:
        mine = [views[i * K + first + v] for i in range(n) for v in range(g[0])]
        rc, bad = _views_check(jb, desc, mine, n, g[0], g)
        if rc:
            return rc, (bad // g[0]) * K + first + bad % g[0] if bad >= 0 else -1
        first += g[0]
    return 0, -1


def test_struct_sizes(jb):
    assert ctypes.sizeof(jb.ViewGroup) == 24 and ctypes.sizeof(jb.ViewOutput) == 40
    assert [f[0] for f in jb.ViewGroup._fields_] == ["rs", "n_views", "reserved"]
    assert [f[0] for f in jb.ViewOutput._fields_] == ["d_out", "image_stride", "view_stride", "row_stride", "plane_stride"]
    assert jb.VIEW_GROUPS_MAX == 4
    assert jb.lib().jb_abi_version() == 1


def _random_request(rng):
    W, H = int(rng.integers(1, 120)), int(rng.integers(1, 120))
    n = int(rng.integers(0, 4))
    groups = []
    for _ in range(int(rng.integers(1, 5))):
        k = int(rng.integers(1, 5)) if rng.random() < 0.9 else int(rng.integers(-1, 12))
        t = (int(rng.integers(1, 120)), int(rng.integers(1, 120)))
        r = rng.random()
        if r < 0.25:
            t = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))      # small targets: the tap cap of long reductions
        elif r < 0.29:
            t = (0, 0)
        elif r < 0.32:
            t = (0, 5)
        filt = int(rng.integers(0, 3)) if rng.random() < 0.97 else 3
        groups.append((k, t, filt, int(rng.random() < 0.01), int(rng.random() < 0.01)))
    K = max(sum(max(g[0], 0) for g in groups), 1)
    views = []
    for _ in range(n * K):
        if rng.random() < 0.5:
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        else:
            w, h = W - int(rng.integers(0, min(W, 3))), H - int(rng.integers(0, min(H, 3)))   # long reductions
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        r = rng.random()
        if r < 0.01:
            w += W - w - x + 1
        elif r < 0.02:
            y = -1
        flags = int(rng.integers(0, 2)) if rng.random() < 0.99 else 2
        views.append((x, y, w, h, flags, int(rng.random() < 0.005)))
    return W, H, n, groups, views


def test_check_against_the_views_check_per_group(jb):
    rng = np.random.default_rng(16)
    seen = {}
    for _ in range(4000):
        W, H, n, groups, views = _random_request(rng)
        desc = jb.make_desc(W, H, 2, 2) if rng.random() < 0.98 else jb.make_desc(W, H, 3, 1)
        got, want = _check(jb, desc, views, n, groups), _restated(jb, desc, views, n, groups)
        assert got == want, (W, H, n, groups, views)
        seen[got[0], got[1] >= 0] = seen.get((got[0], got[1] >= 0), 0) + 1
        if len(groups) == 1:        # G = 1 is jb_views_check
            assert got == _views_check(jb, desc, views, n, groups[0][0], groups[0]) or groups[0][4] != 0, (W, H, n, groups, views)
    # the run has seen every kind of answer: good calls, a view to blame for a rectangle and for the tap cap, no target
    assert seen[0, False] > 500 and seen[-2, True] > 50 and seen[-9, True] > 50 and seen[-7, False] > 20 and seen[-2, False] > 50, seen
    assert seen[-3, False] > 10, seen


W, H = 40, 24
GOOD = [(0, 0, W, H, 0, 0), (39, 23, 1, 1, 1, 0), (3, 2, 20, 10, 1, 0),          # two images of K = 3 views: groups of 2 and 1
        (0, 0, 1, 1, 0, 0), (5, 5, 30, 10, 1, 0), (1, 1, 38, 22, 0, 0)]
G21 = [(2, (8, 8), 0, 0, 0), (1, (5, 3), 2, 0, 0)]


def test_structural_refusals_in_their_order(jb):
    d = jb.make_desc(W, H, 2, 2)
    assert _check(jb, d, GOOD, 2, G21) == (0, -1)
    assert _check(jb, d, [], 0, G21) == (0, -1)
    assert _check(jb, d, [], 0, G21, null=("views",)) == (0, -1)          # no views to read
    # 1. NULLs, whatever else is wrong
    assert _check(jb, jb.make_desc(W, H, 3, 1), GOOD, 2, G21, null=("desc",)) == (-1, -1)
    assert _check(jb, jb.make_desc(W, H, 3, 1), GOOD, 2, G21, null=("groups",)) == (-1, -1)
    assert _check(jb, jb.make_desc(W, H, 3, 1), GOOD, 2, G21, null=("views",)) == (-1, -1)
    # 2. the descriptor's own errors, whatever the counts
    assert _check(jb, jb.make_desc(W, H, 3, 1), GOOD, 2, G21, n_groups=5) == (-3, -1)
    assert _check(jb, jb.make_desc(0, H, 2, 2), GOOD, -1, G21) == (-2, -1)
    # 3. the counts, in front of every view: a view outside the frame is not named
    outside = list(GOOD)
    outside[0] = (0, 0, W + 1, H, 0, 0)
    assert _check(jb, d, outside, -1, G21) == (-2, -1)
    for n_groups in (0, 5, -1):
        assert _check(jb, d, outside, 2, G21, n_groups=n_groups) == (-2, -1), n_groups
    assert _check(jb, d, outside, 2, [(2, (8, 8), 0, 0, 0), (0, (5, 3), 0, 0, 0)]) == (-2, -1)
    assert _check(jb, d, outside, 2, [(2, (8, 8), 0, 0, 0), (-1, (5, 3), 0, 0, 0)]) == (-2, -1)
    assert _check(jb, d, outside, 2, [(2, (8, 8), 0, 0, 0), (1, (5, 3), 0, 0, 1)]) == (-2, -1)          # a group's reserved
    assert _check(jb, d, outside * 3, 1, [(8, (8, 8), 0, 0, 0), (8, (5, 3), 0, 0, 0), (1, (2, 2), 0, 0, 0)]) == (-2, -1)   # K = 17
    assert _check(jb, d, GOOD * 3, 1, [(8, (8, 8), 0, 0, 0), (8, (5, 3), 0, 0, 0)])[0] == 0                  # K = 16
    assert _check(jb, d, GOOD, 1, [(1, (8, 8), 0, 0, 0), (2, (5, 3), 0, 0, 0), (2, (2, 2), 1, 0, 0), (1, (1, 1), 0, 0, 0)]) == (0, -1)   # G = 4
    # 4. the views in flat order: flags and reserved of EVERY view before any rectangle; in front of every group's target
    no_target = [(2, (0, 0), 0, 0, 0), (1, (0, 5), 3, 0, 0)]
    assert _check(jb, d, outside, 2, no_target) == (-2, 0)
    flagged = list(outside)
    flagged[5] = (1, 1, 38, 22, 2, 0)
    assert _check(jb, d, flagged, 2, no_target) == (-2, 5)
    flagged[5] = (1, 1, 38, 22, 1, 1)
    assert _check(jb, d, flagged, 2, no_target) == (-2, 5)
    late = list(GOOD)
    late[5] = (1, 1, 38, 24, 0, 0)                                      # the last view of the last image, in group 1
    assert _check(jb, d, late, 2, no_target) == (-2, 5)
    # 5. the groups in order: no target -7, the target's and the filter's own
    assert _check(jb, d, GOOD, 2, no_target) == (-7, -1)
    assert _check(jb, d, GOOD, 2, [(2, (8, 8), 0, 0, 0), (1, (0, 0), 1, 0, 0)]) == (-7, -1)
    assert _check(jb, d, GOOD, 2, [(2, (8, 8), 0, 0, 0), (1, (0, 5), 0, 0, 0)]) == (-2, -1)
    assert _check(jb, d, GOOD, 2, [(2, (8, 8), 3, 0, 0), (1, (0, 0), 0, 0, 0)]) == (-2, -1)       # group 0's filter before group 1's target
    assert _check(jb, d, GOOD, 2, [(2, (8, 8), 0, 1, 0), (1, (5, 3), 0, 0, 0)]) == (-2, -1)       # a jb_resize's reserved
    # the tap cap in one group only, with the view's FLAT index in the caller's array
    big = jb.make_desc(4000, 30, 2, 2)
    views = [(0, 0, 10, 10, 0, 0), (0, 0, 4000, 30, 1, 0), (0, 0, 4000, 30, 0, 0)] * 2
    assert _check(jb, big, views, 2, [(2, (8, 8), 0, 0, 0), (1, (900, 8), 2, 0, 0)]) == (0, -1)
    assert _check(jb, big, views, 2, [(2, (8, 8), 0, 0, 0), (1, (8, 8), 2, 0, 0)]) == (-9, 2)
    assert _check(jb, big, views, 2, [(1, (8, 8), 2, 0, 0), (2, (8, 8), 1, 0, 0)]) == (-9, 1)
    views[2] = (0, 0, 10, 10, 0, 0)
    assert _check(jb, big, views, 2, [(2, (8, 8), 0, 0, 0), (1, (8, 8), 2, 0, 0)]) == (-9, 5)


def test_bytes_against_output_bytes(jb):
    L = jb.lib()

    def raw(groups, fmt, n_groups=None, offsets=True):
        off, total = (ctypes.c_int64 * 4)(-1, -1, -1, -1), ctypes.c_int64(-1)
        rc = L.jb_view_groups_bytes(_groups(jb, groups), len(groups) if n_groups is None else n_groups, fmt, off if offsets else None, ctypes.byref(total))
        return rc, list(off), total.value

    rng = np.random.default_rng(4)
    for _ in range(200):
        groups = [(int(rng.integers(1, 5)), (int(rng.integers(1, 300)), int(rng.integers(1, 300))), int(rng.integers(0, 3)), 0, 0)
                  for _ in range(int(rng.integers(1, 5)))]
        for fmt in range(4):
            at, want = 0, []
            for k, (w, h), *_ in groups:
                want.append(at)
                at += k * jb.output_bytes(w, h, fmt)
            rc, off, total = raw(groups, fmt)
            assert (rc, off[:len(groups)], total) == (0, want, at) and off[len(groups):] == [-1] * (4 - len(groups))
            assert raw(groups, fmt, offsets=False) == (0, [-1] * 4, at)
            assert jb.view_groups_bytes([(g[0], g[1], g[2]) for g in groups], fmt) == (want, at)
    assert jb.view_groups_bytes([(2, (224, 224)), (8, (96, 96))], jb.OutputSpec.imagenet(3)) == ([0, 2 * 3 * 224 * 224 * 2], (2 * 224 * 224 + 8 * 96 * 96) * 6)
    good = [(2, (8, 8), 0, 0, 0)]
    assert L.jb_view_groups_bytes(None, 1, 0, None, ctypes.byref(ctypes.c_int64())) == -1
    assert L.jb_view_groups_bytes(_groups(jb, good), 1, 0, None, None) == -1
    for bad in (raw(good, 0, n_groups=0), raw(good * 5, 0), raw(good, 4), raw([(0, (8, 8), 0, 0, 0)], 0), raw([(2, (8, 8), 0, 0, 1)], 0),
                raw([(2, (0, 8), 0, 0, 0)], 0), raw([(2, (8, 65536), 0, 0, 0)], 0), raw([(9, (8, 8), 0, 0, 0), (8, (8, 8), 0, 0, 0)], 0)):
        assert bad[0] == -2 and bad[2] == -1, bad


def test_request_and_route(jb):
    from jpeg_decoder_amd import api
    views = [[(1, 2, 3, 4), (5, 6, 7, 8, True), (0, 0, 1, 1)], [jb.View(9, 10, 11, 12, 1, 0), (13, 14, 15, 16, 0), (2, 2, 2, 2, True)]]
    groups = [(2, (8, 9)), (1, (5, 3), jb.FILTER_BICUBIC)]
    outs = [(4096, 1000, 300, 24), jb.ViewOutput(8192, 500, 0, 15, 45)]
    q = api._Request(fmt=3, views=views, view_groups=groups, view_outputs=outs)
    assert (q.n_groups, q.views_per_image, q.n_view_rows, q.target) == (2, 3, 2, None)
    assert [(g.n_views, g.rs.out_w, g.rs.out_h, g.rs.filter, g.rs.reserved, g.reserved) for g in q.groups] == [(2, 8, 9, 0, 0, 0), (1, 5, 3, 2, 0, 0)]
    assert [(o.d_out, o.image_stride, o.view_stride, o.row_stride, o.plane_stride) for o in q.outputs] == [(4096, 1000, 300, 24, 0), (8192, 500, 0, 15, 45)]
    route, tail = q.routed()
    assert route == "view_groups" and api._ROUTES["view_groups"] == (None, None, "jb_blocks_to_rgb_device_view_groups")
    assert tail[0] is q.views and tail[1] is q.groups and tail[2] is q.outputs and tail[3] == 2 and len(tail) == 5
    assert hasattr(jb.lib(), "jb_blocks_to_rgb_device_view_groups")
    for name in ("jb_batch_decoder_run_view_groups", "jb_batch_decoder_submit_view_groups", "jb_view_groups_check", "jb_view_groups_bytes"):
        assert hasattr(jb.lib(), name), name
    # groups bring their own targets and filters: nothing else that names a size, a source or a filter goes with them
    for kw in (dict(resize=(8, 9)), dict(filter=jb.FILTER_BILINEAR), dict(roi=(0, 0, 1, 1)), dict(crops=[(0, 0, 1, 1)] * 2), dict(scale=2),
               dict(fit=jb.Fit.cover())):
        with pytest.raises(jb.JbError) as e:
            api._Request(views=views, view_groups=groups, **kw)
        assert e.value.status == -9, kw
    with pytest.raises(jb.JbError) as e:
        api._Request(view_groups=groups)
    assert e.value.status == -7
    for rows in ([views[0], views[1][:2]], [r[:2] for r in views], [r + r for r in views]):
        with pytest.raises(jb.JbError) as e:
            api._Request(views=rows, view_groups=groups)
        assert e.value.status == -2
    with pytest.raises(jb.JbError) as e:
        api._Request(views=views, view_groups=groups, view_outputs=outs[:1])
    assert e.value.status == -2
    assert api._Request(resize=(8, 9), views=views).routed()[0] == "views"       # views alone keep their route
    # the binding's check
    d = jb.make_desc(100, 100, 2, 2)
    jb.view_groups_check(d, views, groups)
    with pytest.raises(jb.JbError) as e:
        jb.view_groups_check(d, [views[0], [(0, 0, 100, 100), (0, 0, 101, 100), (0, 0, 1, 1)]], groups)
    assert e.value.status == -2 and "image 1, view 1" in str(e.value)
    with pytest.raises(jb.JbError) as e:
        jb.view_groups_check(d, views, [(2, (8, 9)), (1, (0, 0))])
    assert e.value.status == -7


def test_random_multicrop(jb):
    from jpeg_decoder_amd.crops import random_multicrop, random_views
    assert jb.random_multicrop is random_multicrop
    a = random_multicrop(1920, 1080, np.random.default_rng(5))
    assert len(a) == 10 and a == random_multicrop(1920, 1080, np.random.default_rng(5)) != random_multicrop(1920, 1080, np.random.default_rng(6))
    rng = np.random.default_rng(5)
    assert a == random_views(1920, 1080, rng, 2, 0.5, (0.4, 1.0)) + random_views(1920, 1080, rng, 8, 0.5, (0.05, 0.4))
    # the local crops are the smaller ones
    assert min(v[2] * v[3] for v in a[:2]) > max(v[2] * v[3] for v in a[2:])
    spec = ((1, (0.5, 1.0)), (3, (0.1, 0.3)), (2, (0.02, 0.1)))
    rng, again = np.random.default_rng(9), np.random.default_rng(9)
    for w, h in ((123, 77), (1, 1), (7, 300), (300, 7)):
        row = random_multicrop(w, h, rng, spec, p_mirror=0.3, ratio=(0.5, 2.0))
        want = []
        for k, scale in spec:
            want += random_views(w, h, again, k, 0.3, scale, (0.5, 2.0))
        assert row == want and len(row) == 6
        jb.view_groups_check(jb.make_desc(w, h, 1, 1), [row, row], [(1, (32, 32)), (3, (16, 16), jb.FILTER_BILINEAR), (2, (8, 8))])
    assert random_multicrop(123, 77, rng, ()) == []


def test_view_group_kernel_bodies_under_sanitizers():
    """tools/fuzz/view_groups_kernel_check: the kViewGroups instantiations of both view kernels on the CPU -- area, bilinear
    and bicubic x formats 0-3 x mirror on / off, two images in the groups (2 @ 70x9, 1 @ 1x5, 1 @ 65x3) into one exactly-sized
    block buffer, tight and padded -- under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "view_groups_kernel_check"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "view_groups_kernel_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) >= 3 * 4 * 2, r.stdout
