"""View groups on the GPU (-m gpu): with views= and view_groups=[(K_g, (w_g, h_g)[, filter_g]), ...] output (i, v) of group g is

    u   = the reference of its rectangle alone at the GROUP's target under the GROUP's filter (resize_ref / pillow_resize_ref)
    out = format_ref.to_format(u[:, ::-1] if mirror else u, fmt, scale, bias)

bit for bit -- and, bit for bit, what the existing views= route writes on the same device for that group's views alone
(include/jpegblk.h, "view groups": the definition).  Every comparison is made against both.  At the seam whole
sentinel-filled buffers with an odd lead and padded strides are compared, the groups in separate buffers and interleaved
in one buffer in the batch decoder's block layout."""
import ctypes
import os

import numpy as np
import pytest

import format_ref as fr
import orient_ref
from seam_harness import DT, LAYOUTS, NO_PARAMS, SENT, _oracle_full
from test_gpu_views import AREA, BH, BICUBIC, BILINEAR, BW, NAMES, ViewSeam, _batch3, _gold, _params, _view_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def ctx(jb):
    c = jb.Context(0)
    yield c
    c.close()


def _norm(groups):
    return [(g[0], tuple(g[1]), g[2] if len(g) > 2 else AREA) for g in groups]


_refs = {}


def _ref_u8(key, full, view, target, filt):
    """one view's uint8 reference, computed once per (image, view, target, filter) and shared by the formats"""
    k = (key, tuple(view), tuple(target), filt)
    if k not in _refs:
        _refs[k] = np.ascontiguousarray(_view_ref(full, view, target, filt))
    return _refs[k]


class Layout:
    """Where the groups' outputs lie: per group a buffer of its own, or all groups interleaved in ONE buffer in the batch
    decoder's block layout (group 0's outputs of an image, then group 1's, ...).  Rows, planes, views and images are padded
    (in elements) and every buffer starts at an odd address; idx[g][i, v] are the byte indices of output (i, v) of group g
    in buffer buf_of[g]."""

    def __init__(self, n, fmt, groups, pads, interleaved):
        pad_row, pad_plane, pad_view, pad_img = pads
        es = np.dtype(DT[fmt]).itemsize
        self.lead = 256 + 5 if es == 1 else 256 + 3 * es
        self.outs, self.idx, self.buf_of, self.sizes = [], [], [], []
        geo = []
        for k, (w, h), _ in groups:
            row = 3 * w + pad_row if fmt == 0 else (w + pad_row) * es
            plane = 0 if fmt == 0 else row * h + pad_plane * es
            view = (row * h if fmt == 0 else 3 * plane) + pad_view * es
            geo.append((k, w, h, row, plane, view))
        block = sum(k * view for k, _, _, _, _, view in geo) + pad_img * es
        at = 0
        for g, (k, w, h, row, plane, view) in enumerate(geo):
            img = block if interleaved else k * view + pad_img * es
            off = self.lead + (at if interleaved else 0)
            at += k * view
            inner = (np.arange(h)[:, None] * row + np.arange(3 * w)[None, :] if fmt == 0 else
                     np.arange(3)[:, None, None] * plane + np.arange(h)[None, :, None] * row + np.arange(w * es)[None, None, :])
            self.idx.append(off + (np.arange(n)[:, None] * img + np.arange(k)[None, :] * view).reshape((n, k) + (1,) * inner.ndim) + inner)
            self.outs.append((off, img, view, row, plane))
            self.buf_of.append(0 if interleaved else g)
            if not interleaved:
                self.sizes.append(self.lead + n * img + 256)
        if interleaved:
            self.sizes = [self.lead + n * block + 256]


def run_groups(s, ctx, fmt, views, groups, scale_bias=NO_PARAMS, interleaved=False, pads=(13, 7, 31, 77), call=None):
    """One grouped launch of the ViewSeam's images -> (the buffers as host bytes, the Layout).  call(ctx, batch, spec, outputs):
    another launch than the binding's; a JbError is kept in s.error when s.catch is set."""
    import torch
    jb = s.jb
    groups = _norm(groups)
    lay = Layout(s.n, fmt, groups, pads, interleaved)
    bufs = [torch.full((size,), SENT, dtype=torch.uint8, device="cuda:0") for size in lay.sizes]
    assert all(b.data_ptr() % 256 == 0 for b in bufs)
    outs = [(bufs[lay.buf_of[g]].data_ptr() + off, img, view, row, plane) for g, (off, img, view, row, plane) in enumerate(lay.outs)]
    spec = None if fmt == 0 else jb.OutputSpec.make(fmt, *scale_bias)
    b = jb.DeviceBatch()
    b.desc, b.n_images = s.desc, s.n
    b.d_coef, b.coef_image_stride = s.coef_t.data_ptr(), s.coef_t.stride(0) * 2
    b.d_qtabs, b.qtab_image_stride = s.q_t.data_ptr(), 768
    b.d_rgb, b.rgb_row_stride, b.rgb_image_stride = 0, -1, -1          # not read
    torch.cuda.synchronize()
    s.error = None
    try:
        if call is not None:
            call(ctx, b, spec, outs)
        else:
            ctx.blocks_to_rgb_device(b, fmt=spec, views=views, view_groups=groups, view_outputs=outs)
    except jb.JbError as e:
        if not s.catch:
            raise
        s.error = e
    ctx.synchronize()
    return [x.cpu().numpy() for x in bufs], lay


def check_groups(s, ctx, key, fulls, views, groups, fmt, scale=(1, 1, 1), bias=(0, 0, 0), interleaved=False, old=True, **kw):
    """The grouped launch: every output has the bits of its reference and every other byte of every buffer the sentinel;
    and (old) group by group the outputs are those of views= with that group's views alone.  -> the buffers"""
    groups = _norm(groups)
    hosts, lay = run_groups(s, ctx, fmt, views, groups, (scale, bias), interleaved, **kw)
    wants = [np.full(h.size, SENT, np.uint8) for h in hosts]
    first = 0
    for g, (k, target, filt) in enumerate(groups):
        for i, (full, row) in enumerate(zip(fulls, views)):
            for v in range(k):
                ref = fr.to_format(_ref_u8((key, i), full, row[first + v], target, filt), fmt, scale, bias)
                wants[lay.buf_of[g]][lay.idx[g][i, v]] = fr.bits(ref).view(np.uint8).reshape(lay.idx[g][i, v].shape)
        first += k
    for n, (host, want) in enumerate(zip(hosts, wants)):
        if not np.array_equal(host, want):
            bad = np.flatnonzero(host != want)
            inside = np.isin(bad, np.concatenate([lay.idx[g].ravel() for g in range(len(groups)) if lay.buf_of[g] == n]))
            raise AssertionError(f"{key} groups {groups} fmt {fmt} interleaved {interleaved} buffer {n}: {bad.size} bytes differ, "
                                 f"{int((~inside).sum())} of them outside the outputs; first at buffer byte {bad[0]}")
    if old:
        first = 0
        for g, (k, target, filt) in enumerate(groups):
            mine = [row[first:first + k] for row in views]
            host, idx = s.run_views(ctx, fmt, mine, target, filt, (scale, bias))
            assert np.array_equal(hosts[lay.buf_of[g]][lay.idx[g]].reshape(s.n * k, -1), host[idx].reshape(s.n * k, -1)), (key, g, fmt)
            first += k
    return hosts


# ---- three images of 600 x 100 (test_gpu_views' batch), K = 5 and K = 4 ------------------------------------------------------
V5 = [[(0, 0, BW, BH), (0, 0, BW, BH, True), (599, 99, 1, 1, True), (3, 2, 20, 10), (570, 85, 30, 15, True)],
      [(3, 2, 20, 10), (570, 85, 30, 15, True), (509, 3, 10, 90), (1, 50, 598, 1, True), (100, 20, 300, 60)],
      [(100, 20, 300, 60), (200, 40, 250, 50, True), (1, 50, 598, 1), (0, 0, 1, 1), (0, 0, BW, BH, True)]]
GROUPS_A = [(2, (37, 29)), (3, (70, 9))]               # (70, 9): two 64-column workgroups, mirrored stores cross their seam
V4 = [[(0, 0, BW, BH, True), (570, 85, 30, 15), (3, 2, 20, 10, True), (599, 99, 1, 1)],
      [(509, 3, 10, 90), (0, 0, BW, BH, True), (100, 20, 300, 60, True), (200, 40, 250, 50)],
      [(1, 50, 598, 1, True), (100, 20, 300, 60, True), (0, 0, 16, 16), (584, 84, 16, 16, True)]]
GROUPS_B = [(1, (1, 4)), (1, (65, 3)), (2, (16, 16))]  # three groups; (65, 3): one column into the second workgroup


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_groups_per_layout(jb, ctx, oracle, hs, vs):
    s, fulls = _batch3(jb, oracle, hs, vs)
    for k, fmt in enumerate((0, 1, 2, 3)):
        for views, groups in ((V5, GROUPS_A), (V4, GROUPS_B)):
            for interleaved in (False, True):
                check_groups(s, ctx, (hs, vs), fulls, views, groups, fmt, *_params(k, fmt), interleaved=interleaved)


@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_seam_groups_with_mixed_filters(jb, ctx, oracle, hs, vs):
    """bicubic, area and bilinear by group: every view's window is taken at ITS group's target, the union over all of them"""
    s, fulls = _batch3(jb, oracle, hs, vs)
    groups = [(2, (37, 29), BICUBIC), (1, (70, 9), AREA), (2, (16, 16), BILINEAR)]
    assert jb.filter_window(s.desc, (16, 16), BILINEAR, V5[0][3][:4]) != jb.filter_window(s.desc, (37, 29), BICUBIC, V5[0][3][:4])
    for k, fmt in enumerate((0, 3)):
        for interleaved in (False, True):
            check_groups(s, ctx, (hs, vs), fulls, V5, groups, fmt, *_params(k, fmt), interleaved=interleaved)
    check_groups(s, ctx, (hs, vs), fulls, V5, [(3, (37, 29), BILINEAR), (2, (70, 9), BICUBIC)], 2, *_params(0, 2), interleaved=True)


@pytest.mark.parametrize("filt", [AREA, BICUBIC])
def test_seam_one_group_is_the_views_route(jb, ctx, oracle, filt):
    """G = 1 with the strides of views=: byte for byte the buffer of views="""
    s, fulls = _batch3(jb, oracle, 2, 2)
    for k, fmt in enumerate((0, 3)):
        old, idx = s.run_views(ctx, fmt, V5, (70, 9), filt, _params(k, fmt))
        assert not (old[idx] == SENT).all()
        new, lay = run_groups(s, ctx, fmt, V5, [(5, (70, 9), filt)], _params(k, fmt), pads=(13, 7, 77, 0))
        assert len(new) == 1 and np.array_equal(new[0], old), (fmt, filt)


def test_seam_more_rows_than_a_table_holds(jb, ctx, oracle, monkeypatch):
    """12 images x groups (3, 1): 36 rows of group 0 against 32 per launch, the second launch starts in the middle of image
    10; then on contexts whose scratch ends the sub-batches early (the knob is read when a context is created)."""
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.crops import random_multicrop
    w, h, n = 40, 24, 12
    q = synth.annex_k_qtabs(60)
    coefs = [synth.synth_blocks(w, h, 2, 2, image_index=100 + i, qtabs=q)[0] for i in range(n)]
    fulls = [_oracle_full(oracle, w, h, 2, 2, c, q) for c in coefs]
    rng = np.random.default_rng(36)
    spec = ((3, (0.3, 1.0)), (1, (0.05, 0.3)))
    views = [random_multicrop(w, h, rng, spec) for _ in range(n)]
    assert any(v[4] for row in views for v in row) and not all(v[4] for row in views for v in row)
    groups = [(3, (8, 8)), (1, (5, 3), BILINEAR)]
    s = ViewSeam(jb, w, h, 2, 2, coefs, [q] * n, pad_row=3, pad_plane=5, pad_img=7)
    first = {(fmt, il): check_groups(s, ctx, "twelve", fulls, views, groups, fmt, *_params(1, fmt), interleaved=il, pads=(3, 5, 7, 9))
             for fmt in (0, 3) for il in (False, True)}
    for cap in (4000, 1000):
        monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
        with jb.Context(0) as small:
            for (fmt, il), want in first.items():
                hosts, _ = run_groups(s, small, fmt, views, groups, _params(1, fmt), il, pads=(3, 5, 7, 9))
                assert all(np.array_equal(a, b) for a, b in zip(hosts, want)), (cap, fmt, il)


def test_seam_groups_under_libjpeg_arithmetic(jb):
    """ARITH_LIBJPEG composes unchanged: one KAT file's blocks, views of Pillow's own decode of it."""
    import libjpeg_ref
    name, jpeg, rgb = [k for k in libjpeg_ref.load_kat() if k[0] == "420_521x37_noise_q95"][0]
    desc, q, coef = jb.entropy_decode(jpeg)
    full = libjpeg_ref.decode_blocks(desc, q, np.ascontiguousarray(coef.reshape(-1, 64)))
    assert np.array_equal(full, rgb)
    s = ViewSeam(jb, desc.width, desc.height, 2, 2, [np.ascontiguousarray(coef.reshape(-1, 64))], [q], qtab_id=tuple(desc.qtab_id),
                 pad_row=3, pad_plane=5, pad_img=7)
    views = [[(0, 0, 521, 37, True), (500, 30, 21, 7), (17, 3, 300, 20, True)]]
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as c:
        check_groups(s, c, "kat", [full], views, [(2, (70, 9)), (1, (16, 16), BILINEAR)], 0, interleaved=True)
        check_groups(s, c, "kat", [full], views, [(1, (70, 9), BILINEAR), (2, (37, 5))], 3, *fr.IMAGENET)


def test_seam_groups_under_an_orientation(jb, oracle):
    """orientation=6 (a transposing one) on a 131 x 70 frame: views in ORIENTED coordinates (70 x 131), the mirror last."""
    from jpeg_decoder_amd import synth
    w, h = 131, 70
    coefs, qs = zip(*[synth.synth_blocks(w, h, 2, 2, image_index=50 + i) for i in range(2)])
    fulls = [np.ascontiguousarray(orient_ref.orient(_oracle_full(oracle, w, h, 2, 2, c, q), 6)) for c, q in zip(coefs, qs)]
    s = ViewSeam(jb, w, h, 2, 2, list(coefs), list(qs), pad_row=3, pad_plane=5, pad_img=7)
    views = [[(0, 0, 70, 131, True), (69, 130, 1, 1), (5, 100, 60, 31, True)], [(3, 2, 20, 10), (40, 90, 30, 41, True), (10, 64, 50, 3)]]
    with jb.Context(0, orientation=6) as c:
        check_groups(s, c, "o6", fulls, views, [(1, (37, 29)), (2, (16, 9))], 0, interleaved=True)
        check_groups(s, c, "o6", fulls, views, [(2, (37, 29), BICUBIC), (1, (65, 3))], 3, *fr.IMAGENET)


def test_seam_refusals_write_nothing(jb, ctx, oracle):
    s, fulls = _batch3(jb, oracle, 2, 2)
    L = jb.lib()

    def raw(views=V5, groups=GROUPS_A, n_groups=None, plane_stride=0, edit=None, null=()):
        """straight to the C entry point (what the binding would refuse or cannot say); edit(outputs): strides to spoil"""
        def call(c, b, spec, outs):
            arr = (jb.View * 15)(*[jb.View(*v[:4], jb.VIEW_MIRROR if len(v) > 4 and v[4] else 0, 0) for row in views for v in row])
            gs = (jb.ViewGroup * 5)(*[jb.ViewGroup(jb.Resize(g[1][0], g[1][1], g[2] if len(g) > 2 else 0, 0), g[0], g[3] if len(g) > 3 else 0) for g in groups])
            os_ = (jb.ViewOutput * 5)(*[jb.ViewOutput(*o) for o in outs])
            if edit:
                edit(os_)
            sp = jb.OutputSpec.make(3, plane_stride=plane_stride) if plane_stride else None
            rc = L.jb_blocks_to_rgb_device_view_groups(c._h, ctypes.byref(b), None if "views" in null else arr, None if "groups" in null else gs,
                                                       None if "outputs" in null else os_, len(groups) if n_groups is None else n_groups,
                                                       ctypes.byref(sp) if sp else None, None)
            if rc:
                raise jb.JbError(rc, L.jb_last_error(c._h).decode())
        return call

    def spoil(g, field, value):
        def edit(outs):
            setattr(outs[g], field, value(getattr(outs[g], field)) if callable(value) else value)
        return edit

    outside = [list(r) for r in V5]
    outside[1][4] = (100, 20, BW - 100 + 1, 60)             # image 1, view 4 (group 1): one pixel too wide
    one = lambda o: o - 1
    cases = [("n_groups 0", raw(n_groups=0), -2), ("n_groups 5", raw(groups=GROUPS_A * 2 + GROUPS_A[:1], n_groups=5), -2),
             ("a group of no views", raw(groups=[(5, (37, 29)), (0, (70, 9))]), -2),
             ("a group's reserved", raw(groups=[(2, (37, 29)), (3, (70, 9), 0, 1)]), -2),
             ("K = 17", raw(groups=[(9, (37, 29)), (8, (70, 9))]), -2),
             ("outside", raw(views=outside), -2),
             ("no target", raw(groups=[(2, (37, 29)), (3, (0, 0))]), -7),
             ("bad target", raw(groups=[(2, (37, 29)), (3, (0, 9))]), -2),
             ("unknown filter", raw(groups=[(2, (37, 29), 3), (3, (70, 9))]), -2),
             ("the tap cap in group 1 only", raw(groups=[(2, (37, 29), BILINEAR), (3, (1, 9), BILINEAR)]), -9),
             ("spec plane_stride", raw(plane_stride=1 << 20), -2),
             ("null views", raw(null=("views",)), -1), ("null groups", raw(null=("groups",)), -1), ("null outputs", raw(null=("outputs",)), -1),
             ("null d_out", raw(edit=spoil(1, "d_out", None)), -1),
             ("short row", raw(edit=spoil(1, "row_stride", 3 * 70 - 1)), -2),
             ("short view stride", raw(edit=spoil(1, "view_stride", 9 * (3 * 70 + 13) - 1)), -2),
             ("short image stride", raw(edit=spoil(0, "image_stride", lambda o: o - 78)), -2),
             ("short image stride, group 1", raw(edit=spoil(1, "image_stride", lambda o: o - 78)), -2)]
    s.catch = True
    try:
        for name, call, status in cases:
            hosts, _ = run_groups(s, ctx, 0, V5, GROUPS_A, call=call, pads=(13, 7, 0, 77))
            assert s.error is not None and s.error.status == status, (name, s.error)
            assert all((h == SENT).all() for h in hosts), name
            if name == "outside":
                assert "image 1" in str(s.error) and "view 4" in str(s.error), str(s.error)
        # planar: a plane stride shorter than the rows, a pointer that is no multiple of the element size
        for name, edit in (("short plane", spoil(0, "plane_stride", one)), ("odd pointer", spoil(1, "d_out", lambda p: p + 1))):
            def call(c, b, spec, outs, edit=edit):
                arr, gs, os_ = jb.api._view_array(V5)[0], jb.api._group_array(GROUPS_A)[0], jb.api._output_array(outs, 2)
                edit(os_)
                rc = L.jb_blocks_to_rgb_device_view_groups(c._h, ctypes.byref(b), arr, gs, os_, 2, ctypes.byref(spec), None)
                if rc:
                    raise jb.JbError(rc, "")
            hosts, _ = run_groups(s, ctx, 3, V5, GROUPS_A, call=call)
            assert s.error is not None and s.error.status == -2 and all((h == SENT).all() for h in hosts), name
        with jb.Context(0, orientation=jb.ORIENT_EXIF) as c:
            hosts, _ = run_groups(s, c, 0, V5, GROUPS_A)
            assert s.error is not None and s.error.status == -7 and all((h == SENT).all() for h in hosts)
        # the binding's own, before any C call
        for kw, status in ((dict(resize=(8, 8)), -9), (dict(filter=BILINEAR), -9), (dict(roi=(0, 0, 5, 5)), -9), (dict(scale=2), -9),
                           (dict(fit=jb.Fit.cover()), -9), (dict(crops=[(0, 0, 5, 5)] * 3), -9)):
            hosts, _ = run_groups(s, ctx, 0, V5, GROUPS_A,
                                  call=lambda c, b, spec, outs: c.blocks_to_rgb_device(b, views=V5, view_groups=GROUPS_A, view_outputs=outs, **kw))
            assert s.error is not None and s.error.status == status and all((h == SENT).all() for h in hosts), (kw, s.error)
        for views, status in ((None, -7), ([r[:4] for r in V5], -2), (V5[:2], -2)):
            hosts, _ = run_groups(s, ctx, 0, V5, GROUPS_A,
                                  call=lambda c, b, spec, outs: c.blocks_to_rgb_device(b, views=views, view_groups=GROUPS_A, view_outputs=outs))
            assert s.error is not None and s.error.status == status and all((h == SENT).all() for h in hosts), (status, s.error)
    finally:
        s.catch = False
    check_groups(s, ctx, (2, 2), fulls, V5, GROUPS_A, 0)     # and the context still serves a good call


# ---- the batch decoder -------------------------------------------------------------------------
GV = [[(0, 0, 400, 266), (13, 7, 224, 200, True), (399, 265, 1, 1), (100, 100, 64, 64, True), (0, 0, 400, 266, True)],
      [(13, 7, 224, 200, True), (399, 265, 1, 1), (0, 0, 400, 266), (5, 5, 40, 24), (200, 100, 100, 100, True)],
      [(399, 265, 1, 1, True), (0, 0, 1, 1), (1, 1, 398, 264, True), (0, 0, 400, 266), (7, 9, 20, 12)],
      [(100, 50, 512, 300), (0, 0, 800, 400, True), (1, 2, 3, 4, True), (0, 0, 800, 400), (300, 100, 200, 120, True)],
      [(5, 600, 400, 40, True), (0, 0, 427, 640), (9, 9, 9, 9), (0, 0, 427, 640, True), (20, 30, 200, 120)],
      [(300, 200, 37, 29), (3, 1, 670, 449, True), (0, 0, 679, 451, True), (100, 100, 20, 12), (3, 1, 670, 449)]]
GOTHER = [row[1::-1] + row[:1:-1] for row in GV]
GG = [(2, (32, 32)), (3, (20, 12), BILINEAR)]


def _want(rgbs, spec, views, first, k, target, filt):
    return [np.stack([fr.to_format(_ref_u8(("gold", i), rgb, v, target, filt), spec.format, list(spec.scale), list(spec.bias))
                      for v in row[first:first + k]]) for i, (rgb, row) in enumerate(zip(rgbs, views))]


def _all_good(imgs, st, tm, rgbs, spec, views, olds=None, skip=()):
    """every file's entry is a list of G arrays [K_g, 3, h_g, w_g] with the references' bits (and the views= route's)"""
    # (a batch with a file that failed reports that file's status as its own, as every run does)
    assert tm["rc"] == (0 if not skip else st[skip[0]]) and [x for i, x in enumerate(st) if i not in skip] == [0] * (len(views) - len(skip)), (tm, st)
    first = 0
    for g, (k, target, filt) in enumerate(_norm(GG)):
        want = _want(rgbs, spec, views, first, k, target, filt)
        for i in range(len(views)):
            if i in skip:
                continue
            got = np.ascontiguousarray(imgs[i][g])
            assert tuple(got.shape) == (k, 3, target[1], target[0]), got.shape
            assert fr.same_bits(got, want[i]), (g, i)
            if olds is not None:
                assert fr.same_bits(got, np.ascontiguousarray(olds[g][i])), (g, i)
        first += k


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("huff", ["0", None, "2"])
def test_batch_decoder_view_groups_every_route(jb, monkeypatch, huff, threads):
    import torch
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    paths, n = list(paths), len(NAMES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    offsets, per = jb.view_groups_bytes(GG, spec)
    assert offsets == [0, 2 * 3 * 32 * 32 * 2] and per == offsets[1] + 3 * 3 * 20 * 12 * 2
    # what a user does today: one run(views=) per group, each with its own target size and filter
    olds, first = [], 0
    for k, target, filt in _norm(GG):
        with jb.BatchDecoder(threads, 0, resize=target, fmt=spec) as dec:
            dec.set_filter(filt)
            imgs, st, tm = dec.run(paths, views=[row[first:first + k] for row in GV])
            assert tm["rc"] == 0 and st == [0] * n
            olds.append(imgs)
        first += k
    with jb.BatchDecoder(threads, 0, fmt=spec, arena_bytes=1 << 20) as dec:      # a pinned arena; no target size of its own
        _all_good(*dec.run(paths, views=GV, view_groups=GG), rgbs, spec, GV, olds)
    with jb.BatchDecoder(threads, 0, resize=(7, 7), fmt=spec) as dec:            # the decoder's own target and filter are not read
        # the entropy stage runs once per FILE: the counter rises as it does for one rectangle per file
        n0 = dec.device_entropy_images
        imgs, st, tm = dec.run(paths, crops=[row[0][:4] for row in GV])
        assert st == [0] * n
        per_file = dec.device_entropy_images - n0
        assert (per_file > 0) if huff == "2" else (per_file == 0) if huff == "0" else True
        dec.set_filter(BICUBIC)                                    # (under which the 7 x 7 target would be beyond the tap cap)
        n0 = dec.device_entropy_images
        imgs, st, tm = dec.run(paths, views=GV, view_groups=GG)
        assert dec.device_entropy_images - n0 == per_file
        assert [w.shape[0] for w in imgs[0]] == [2, 3] and tm["rc"] == 0
        _all_good(imgs, st, tm, rgbs, spec, GV, olds)
        outs = [torch.full((n, 2, 3, 32, 32), 7.0, dtype=torch.float16, device="cuda:0"), torch.full((n, 3, 3, 12, 20), 7.0, dtype=torch.float16, device="cuda:0")]
        ret, st, tm = dec.run_to_tensor(paths, outs, views=GV, view_groups=GG)
        assert ret[0] is outs[0] and ret[1] is outs[1]
        _all_good([[o[i].cpu().numpy() for o in outs] for i in range(n)], st, tm, rgbs, spec, GV, olds)
        t0 = dec.submit(paths, views=GV, view_groups=GG)
        t1 = dec.submit(paths, views=GOTHER, view_groups=GG)       # two in flight, each with its own views
        _all_good(*dec.collect(t0), rgbs, spec, GV, olds)
        _all_good(*dec.collect(t1), rgbs, spec, GOTHER)
        # one view that does not fit its file: -2 and None for that file only; its slices of the tensors stay
        bad = [list(r) for r in GV]
        bad[1][3] = (5, 5, 396, 24)                                # img2 is 400 wide; a view of group 1
        imgs, st, tm = dec.run(paths, views=bad, view_groups=GG)
        assert st[1] == -2 and imgs[1] is None
        _all_good(imgs, st, tm, rgbs, spec, bad, skip=(1,))
        for o in outs:
            o.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, outs, views=bad, view_groups=GG)
        assert st[1] == -2 and all((o[1] == 7.0).all() for o in outs)
        _all_good([[o[i].cpu().numpy() for o in outs] for i in range(n)], st, tm, rgbs, spec, bad, skip=(1,))
        # device output: a file's pointer is its block; a region too small for a block is JB_ERR_CAPACITY, nothing partial
        region = torch.full((n * (per + 256) + 256,), SENT, dtype=torch.uint8, device="cuda:0")
        dec.set_device_output(region.data_ptr(), region.numel())
        ptrs, sizes, st, tm = dec.run_to_device(paths, views=GV, view_groups=GG)
        torch.cuda.synchronize()
        assert tm["rc"] == 0 and st == [0] * n and sizes == [(32, 32)] * n           # group 0's target
        host = region.cpu().numpy()
        blocks = []
        for i in range(n):
            off = ptrs[i] - region.data_ptr()
            blocks.append([host[off:off + offsets[1]].view(np.float16).reshape(2, 3, 32, 32), host[off + offsets[1]:off + per].view(np.float16).reshape(3, 3, 12, 20)])
        _all_good(blocks, st, tm, rgbs, spec, GV, olds)
        small = torch.full((per - 256,), SENT, dtype=torch.uint8, device="cuda:0")   # group 0 and most of group 1
        dec.set_device_output(small.data_ptr(), small.numel())
        ptrs, sizes, st, tm = dec.run_to_device(paths[:1], views=GV[:1], view_groups=GG)
        torch.cuda.synchronize()
        assert st == [-5] and ptrs == [0], (st, tm)
        assert (small.cpu().numpy() == SENT).all()
        dec.set_device_output(0, 0)
        # refusals: rows of the wrong count or length, no views; bad counts; a decoder-wide rectangle, a fit, a scale
        for call in (dec.run, dec.submit):
            for views, status in ((GV[:5], -2), ([r[:4] for r in GV], -2), (None, -7)):
                with pytest.raises(jb.JbError) as e:
                    call(paths, views=views, view_groups=GG)
                assert e.value.status == status
        assert dec.run(paths, views=[r * 4 for r in GV], view_groups=[(10, (32, 32)), (10, (20, 12))])[2]["rc"] == -2
        assert dec.run(paths, views=GV, view_groups=[(1, (32, 32))] * 5)[2]["rc"] == -2
        dec.set_roi((0, 0, 100, 100))
        assert dec.run(paths, views=GV, view_groups=GG)[2]["rc"] == -9
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, views=GV, view_groups=GG)
        assert e.value.status == -9
        dec.set_roi(None)
        dec.set_fit(jb.Fit.cover())
        assert dec.run(paths, views=GV, view_groups=GG)[2]["rc"] == -9
        dec.set_fit(None)
        _all_good(*dec.run(paths, views=GV, view_groups=GG), rgbs, spec, GV, olds)    # the decoder is as good as before
    with jb.BatchDecoder(threads, 0, scale=2) as dec:
        assert dec.run(paths, views=GV, view_groups=GG)[2]["rc"] == -9


def test_batch_decoder_view_groups_on_a_two_part_decoder(jb):
    """file i, its K views and the groups go to the same part of a multi-device decoder (here: device 0 twice)"""
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(2, devices=[0, 0], fmt=spec) as dec:
        _all_good(*dec.run(list(paths), views=GV, view_groups=GG), rgbs, spec, GV)
        _all_good(*dec.collect(dec.submit(list(paths), views=GOTHER, view_groups=GG)), rgbs, spec, GOTHER)


def test_batch_decoder_view_groups_on_two_devices(jb):
    if jb.lib().jb_device_count() < 2:
        pytest.skip("one device")
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(2, devices=[0, 1], fmt=spec) as dec:
        _all_good(*dec.run(list(paths), views=GV, view_groups=GG), rgbs, spec, GV)
        _all_good(*dec.collect(dec.submit(list(paths), views=GOTHER, view_groups=GG)), rgbs, spec, GOTHER)
