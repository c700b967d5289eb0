"""Views on the GPU (-m gpu): with views=[[v_0 .. v_K-1], ...] and resize=(ow, oh) output i * K + v of a launch, or view v of
file i of a batch, is

    u   = the reference of the rectangle v alone: resize_ref.area_resize(full_i[slice], ow, oh), or with a filter
          pillow_resize_ref.resize(full_i, rect, (ow, oh), filter)
    out = format_ref.to_format(u[:, ::-1] if mirror else u, fmt, scale, bias)

bit for bit, where full_i is the oracle's full-size decode (seam), libjpeg_ref's / Pillow's (ARITH_LIBJPEG), orient_ref's
turn of it (orientation) or the reference's golden RGB (batch decoder): never something the code under test computed.
At the seam the whole sentinel-filled buffer is compared, pads included."""
import ctypes
import os

import numpy as np
import pytest

import format_ref as fr
import orient_ref
import pillow_resize_ref as pr
from conftest import GOLD, load_golden
from resize_ref import area_resize
from seam_harness import DT, LAYOUTS, NO_PARAMS, SENT, Seam, _oracle_full

pytestmark = pytest.mark.gpu

SETS = list(fr.PARAM_SETS.items())
AREA, BILINEAR, BICUBIC = 0, pr.FILTER_BILINEAR, pr.FILTER_BICUBIC


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


def _params(i, fmt):
    return SETS[(i + fmt) % 3][1] if fmt >= 2 else ((1, 1, 1), (0, 0, 0))


class ViewSeam(Seam):
    """The harness's launch with K outputs per image: the buffer, its strides and the index array describe n * K outputs
    (seam_harness.Seam.run's layout, output for image), the batch still has n images.  call(ctx, batch, spec): the
    launch; a JbError it raises is kept in .error when .catch is set, so that run() still returns the buffer."""
    catch = False
    error = None

    def run_outputs(self, ctx, fmt, out_size, n_out, call, scale_bias=NO_PARAMS):
        import torch
        jb = self.jb
        pad_row, pad_plane, pad_img = self.pads
        w, h = out_size
        es = np.dtype(DT[fmt]).itemsize
        lead = 256 + 5 if es == 1 else 256 + 3 * es   # uint8: the output starts at an odd address
        if fmt == 0:
            row = 3 * w + pad_row
            img = row * h + pad_img
            spec = None
            idx = lead + np.arange(n_out)[:, None, None] * img + np.arange(h)[None, :, None] * row + np.arange(3 * w)[None, None, :]
        else:
            row = (w + pad_row) * es
            plane = row * h + pad_plane * es
            img = 3 * plane + pad_img * es
            spec = jb.OutputSpec.make(fmt, *scale_bias, plane_stride=plane if (pad_plane or pad_row) else 0)
            idx = (lead + np.arange(n_out)[:, None, None, None] * img + np.arange(3)[None, :, None, None] * plane +
                   np.arange(h)[None, None, :, None] * row + np.arange(w * es)[None, None, None, :])
        buf = torch.full((lead + n_out * img + 256,), SENT, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 256 == 0
        b = jb.DeviceBatch()
        b.desc, b.n_images = self.desc, self.n
        b.d_coef, b.coef_image_stride = self.coef_t.data_ptr(), self.coef_t.stride(0) * 2
        b.d_qtabs, b.qtab_image_stride = self.q_t.data_ptr(), 768
        b.d_rgb, b.rgb_row_stride, b.rgb_image_stride = buf.data_ptr() + lead, row, img
        torch.cuda.synchronize()
        self.error = None
        try:
            call(ctx, b, spec)
        except jb.JbError as e:
            if not self.catch:
                raise
            self.error = e
        ctx.synchronize()
        return buf.cpu().numpy(), idx

    def run_views(self, ctx, fmt, views, resize, filt=AREA, scale_bias=NO_PARAMS):
        k = len(views[0])
        return self.run_outputs(ctx, fmt, resize, self.n * k,
                                lambda c, b, spec: c.blocks_to_rgb_device(b, fmt=spec, resize=resize, filter=filt, views=views), scale_bias)

    def run_crops(self, ctx, fmt, crops, resize, filt=AREA, scale_bias=NO_PARAMS):
        return self.run_outputs(ctx, fmt, resize, self.n,
                                lambda c, b, spec: c.blocks_to_rgb_device(b, fmt=spec, resize=resize, filter=filt, crops=crops), scale_bias)


def _view_ref(full, view, resize, filt):
    """one view's uint8 output: the rectangle's reference, THEN the mirror"""
    x, y, w, h = view[:4]
    u = area_resize(full[y:y + h, x:x + w], *resize) if filt == AREA else pr.resize(full, (x, y, w, h), resize, filt)
    return u[:, ::-1] if len(view) > 4 and view[4] else u


def _check(s, ctx, fulls, views, resize, fmt, filt=AREA, scale=(1, 1, 1), bias=(0, 0, 0), tag=None):
    """The launch with `views`: output i * K + v has the bits of its reference, every other byte the sentinel."""
    host, idx = s.run_views(ctx, fmt, views, resize, filt, (scale, bias))
    want = np.full(host.size, SENT, np.uint8)
    n = 0
    for full, row in zip(fulls, views):
        for v in row:
            ref = fr.to_format(np.ascontiguousarray(_view_ref(full, v, resize, filt)), fmt, scale, bias)
            want[idx[n]] = fr.bits(ref).view(np.uint8).reshape(idx[n].shape)
            n += 1
    if not np.array_equal(host, want):
        bad = np.flatnonzero(host != want)
        inside = np.isin(bad, idx.ravel())
        first = int(np.argmax((idx.reshape(idx.shape[0], -1) == bad[0]).any(axis=1))) if inside[0] else -1
        raise AssertionError(f"{tag} resize {resize} fmt {fmt} filter {filt}: {bad.size} bytes differ, {int((~inside).sum())} of them "
                             f"outside the outputs; first at buffer byte {bad[0]} (output {first})")
    return host, idx


# ---- three images of 600 x 100 (wider than one tile's 512 pixels), per-image tables, K = 3 ---------------------------
BW, BH = 600, 100
VIEWS3 = [[(0, 0, BW, BH), (0, 0, BW, BH, True), (599, 99, 1, 1, True)],
          [(3, 2, 20, 10), (570, 85, 30, 15, True), (509, 3, 10, 90)],        # disjoint corners: the union is nearly the frame
          [(100, 20, 300, 60), (200, 40, 250, 50, True), (1, 50, 598, 1)]]    # overlapping; a one-row strip
TARGETS = [(37, 29), (70, 9), (1, 4)]     # (70, 9): two 64-column workgroups, mirrored stores cross their seam
_three = {}


def _batch3(jb, oracle, hs, vs, qid=(0, 1, 2)):
    """-> (ViewSeam, the oracle's three full-size images), made once per layout and not changed"""
    from jpeg_decoder_amd import synth
    key = (hs, vs, qid)
    if key not in _three:
        coefs, qs, fulls = [], [], []
        for i in range(3):
            q = synth.annex_k_qtabs(40 + 12 * i).copy()          # per-image quantisation tables
            q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1, 1, 255)
            c = synth.synth_blocks(BW, BH, hs, vs, image_index=20 + i, qtabs=q, qtab_id=qid, dense=(i == 2))[0]
            coefs.append(c), qs.append(q)
            fulls.append(_oracle_full(oracle, BW, BH, hs, vs, c, q, qid))
        _three[key] = ViewSeam(jb, BW, BH, hs, vs, coefs, qs, qid, pad_row=13, pad_plane=7, pad_img=77), fulls
    return _three[key]


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_three_views_per_layout(jb, ctx, oracle, hs, vs):
    s, fulls = _batch3(jb, oracle, hs, vs)
    for k, fmt in enumerate((0, 1, 2, 3) if (hs, vs) == (2, 2) else (0, 3)):
        for t in TARGETS:
            _check(s, ctx, fulls, VIEWS3, t, fmt, AREA, *_params(k, fmt), tag=(hs, vs))


@pytest.mark.parametrize("filt", [BILINEAR, BICUBIC])
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_seam_three_views_filtered(jb, ctx, oracle, hs, vs, filt):
    """(1, 4) is no target here: a 600-pixel view to one column is beyond the tap cap (refused: see the refusals below)."""
    s, fulls = _batch3(jb, oracle, hs, vs)
    d = s.desc
    # a window strictly larger than its rectangle, and a view on the frame's edge
    assert jb.filter_window(d, TARGETS[0], filt, VIEWS3[1][0][:4]) != VIEWS3[1][0][:4]
    assert VIEWS3[1][1][0] + VIEWS3[1][1][2] == BW and VIEWS3[1][1][1] + VIEWS3[1][1][3] == BH
    for t in TARGETS[:2]:
        for k, fmt in enumerate((0, 3)):
            _check(s, ctx, fulls, VIEWS3, t, fmt, filt, *_params(k, fmt), tag=(hs, vs))


def _mirrored(host, idx, fmt, size):
    """`host` with the rows of every output reversed"""
    w, h = size
    out = host.copy()
    es = np.dtype(DT[fmt]).itemsize
    for i in range(idx.shape[0]):
        px = host[idx[i]]
        out[idx[i]] = (px.reshape(h, w, 3)[:, ::-1].reshape(idx[i].shape) if fmt == 0 else
                       px.reshape(3, h, w, es)[:, :, ::-1].reshape(idx[i].shape))
    return out


@pytest.mark.parametrize("filt", [AREA, BICUBIC])
def test_seam_one_view_is_the_crops_route(jb, ctx, oracle, filt):
    """K = 1 without mirrors: byte for byte the buffer of crops=; all mirrored: that buffer with every row reversed."""
    s, fulls = _batch3(jb, oracle, 2, 2)
    crops = [(0, 0, BW, BH), (509, 3, 10, 90), (200, 40, 250, 50)]
    t = TARGETS[1]
    for k, fmt in enumerate((0, 3)):
        old, idx = s.run_crops(ctx, fmt, crops, t, filt, _params(k, fmt))
        assert not (old[idx] == SENT).all()
        new, _ = s.run_views(ctx, fmt, [[c] for c in crops], t, filt, _params(k, fmt))
        assert np.array_equal(new, old), (fmt, filt)
        flipped, _ = s.run_views(ctx, fmt, [[c + (True,)] for c in crops], t, filt, _params(k, fmt))
        assert np.array_equal(flipped, _mirrored(old, idx, fmt, t)), (fmt, filt)
        assert not np.array_equal(flipped, old)


def test_seam_more_views_than_a_table_holds(jb, ctx, oracle, monkeypatch):
    """12 images x 3 views = 36 rows against 32 per launch; then on contexts whose scratch ends the sub-batches early
    (1,000 bytes: one image each): identical buffers.  (The knob is read when a context is created.)"""
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.crops import random_views
    w, h, n, k = 40, 24, 12, 3
    q = synth.annex_k_qtabs(60)
    coefs = [synth.synth_blocks(w, h, 2, 2, image_index=100 + i, qtabs=q)[0] for i in range(n)]
    fulls = [_oracle_full(oracle, w, h, 2, 2, c, q) for c in coefs]
    rng = np.random.default_rng(36)
    views = [random_views(w, h, rng, k) for _ in range(n)]
    assert any(v[4] for row in views for v in row) and not all(v[4] for row in views for v in row)
    s = ViewSeam(jb, w, h, 2, 2, coefs, [q] * n, pad_row=3, pad_plane=5, pad_img=7)
    first = {fmt: _check(s, ctx, fulls, views, (8, 8), fmt, AREA, *_params(1, fmt))[0] for fmt in (0, 3)}
    for cap in (4000, 1000):
        monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
        with jb.Context(0) as small:
            for fmt in (0, 3):
                host, _ = s.run_views(small, fmt, views, (8, 8), AREA, _params(1, fmt))
                assert np.array_equal(host, first[fmt]), (cap, fmt)


def test_seam_views_under_libjpeg_arithmetic(jb):
    """ARITH_LIBJPEG composes unchanged: one KAT file's blocks, views of Pillow's own decode of it."""
    import libjpeg_ref
    name, jpeg, rgb = [k for k in libjpeg_ref.load_kat() if k[0] == "420_521x37_noise_q95"][0]
    desc, q, coef = jb.entropy_decode(jpeg)
    assert (desc.hs, desc.vs) == (2, 2)
    full = libjpeg_ref.decode_blocks(desc, q, np.ascontiguousarray(coef.reshape(-1, 64)))
    assert np.array_equal(full, rgb)
    s = ViewSeam(jb, desc.width, desc.height, 2, 2, [np.ascontiguousarray(coef.reshape(-1, 64))], [q], qtab_id=tuple(desc.qtab_id),
                 pad_row=3, pad_plane=5, pad_img=7)
    views = [[(0, 0, 521, 37, True), (500, 30, 21, 7), (17, 3, 300, 20, True)]]
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as c:
        _check(s, c, [full], views, (70, 9), 0, AREA)
        _check(s, c, [full], views, (70, 9), 3, BILINEAR, *fr.IMAGENET)


def test_seam_views_under_an_orientation(jb, oracle):
    """orientation=6 (a transposing one) on a 131 x 70 frame: views in ORIENTED coordinates (70 x 131), the mirror last."""
    from jpeg_decoder_amd import synth
    w, h = 131, 70
    coefs, qs = zip(*[synth.synth_blocks(w, h, 2, 2, image_index=50 + i) for i in range(2)])
    fulls = [np.ascontiguousarray(orient_ref.orient(_oracle_full(oracle, w, h, 2, 2, c, q), 6)) for c, q in zip(coefs, qs)]
    assert fulls[0].shape == (131, 70, 3)
    s = ViewSeam(jb, w, h, 2, 2, list(coefs), list(qs), pad_row=3, pad_plane=5, pad_img=7)
    views = [[(0, 0, 70, 131, True), (69, 130, 1, 1), (5, 100, 60, 31, True)], [(3, 2, 20, 10), (40, 90, 30, 41, True), (10, 64, 50, 3)]]
    with jb.Context(0, orientation=6) as c:
        _check(s, c, fulls, views, (37, 29), 0, AREA)
        _check(s, c, fulls, views, (37, 29), 3, BICUBIC, *fr.IMAGENET)


def test_seam_refusals_write_nothing(jb, ctx, oracle):
    s, fulls = _batch3(jb, oracle, 2, 2)
    t = TARGETS[0]
    L = jb.lib()

    def raw(views, k, resize, filt=AREA, reserved=0):
        """straight to the C entry point (what the binding would refuse or cannot say)"""
        def call(c, b, spec):
            rs = ctypes.byref(jb.Resize(resize[0], resize[1], filt, reserved)) if resize is not None else None
            rc = L.jb_blocks_to_rgb_device_views(c._h, ctypes.byref(b), views, k, rs, None, None)
            if rc:
                raise jb.JbError(rc, L.jb_last_error(c._h).decode())
        return call

    def flat(views, flags=None, reserved=None):
        arr = (jb.View * 9)(*[jb.View(*v[:4], jb.VIEW_MIRROR if len(v) > 4 and v[4] else 0, 0) for row in views for v in row])
        if flags is not None:
            arr[flags[0]].flags = flags[1]
        if reserved is not None:
            arr[reserved].reserved = 1
        return arr

    outside = [list(r) for r in VIEWS3]
    outside[1][2] = (509, 3, BW - 509 + 1, 90)              # image 1, view 2: one pixel too wide
    cases = [("outside", raw(flat(outside), 3, t), -2),
             ("null views", raw(None, 3, t), -1),
             ("null resize", raw(flat(VIEWS3), 3, None), -1),
             ("no target", raw(flat(VIEWS3), 3, (0, 0)), -7),
             ("no target, filtered", raw(flat(VIEWS3), 3, (0, 0), BICUBIC), -7),
             ("bad target", raw(flat(VIEWS3), 3, (0, 5)), -2),
             ("K = 0", raw(flat(VIEWS3), 0, t), -2),
             ("K = 17", raw(flat(VIEWS3), 17, t), -2),
             ("flag bit 1", raw(flat(VIEWS3, flags=(4, 2)), 3, t), -2),
             ("reserved", raw(flat(VIEWS3, reserved=8), 3, t), -2),
             ("unknown filter", raw(flat(VIEWS3), 3, t, 3), -2),
             ("resize reserved", raw(flat(VIEWS3), 3, t, AREA, 1), -2),
             ("tap cap", raw(flat(VIEWS3), 3, TARGETS[2], BILINEAR), -9)]
    s.catch = True
    try:
        for name, call, status in cases:
            host, _ = s.run_outputs(ctx, 0, t, 9, call)
            assert s.error is not None and s.error.status == status, (name, s.error)
            assert (host == SENT).all(), name
            if name == "outside":
                text = str(s.error)
                assert "image 1" in text and "view 2" in text and f"{BW} x {BH}" in text, text
        # the binding's own: a scale, roi or crops with views, no target, ragged rows -- before any C call
        for kw, status in ((dict(scale=2, resize=None), -9), (dict(roi=(0, 0, 5, 5), resize=t), -9), (dict(crops=[(0, 0, 5, 5)] * 3, resize=t), -9),
                           (dict(resize=None), -7)):
            host, _ = s.run_outputs(ctx, 0, t, 9, lambda c, b, spec: c.blocks_to_rgb_device(b, views=VIEWS3, **kw))
            assert s.error is not None and s.error.status == status and (host == SENT).all(), (kw, s.error)
        host, _ = s.run_outputs(ctx, 0, t, 9, lambda c, b, spec: c.blocks_to_rgb_device(b, views=[VIEWS3[0], VIEWS3[1][:2], VIEWS3[2]], resize=t))
        assert s.error.status == -2 and (host == SENT).all()
        host, _ = s.run_outputs(ctx, 0, t, 9, lambda c, b, spec: c.blocks_to_rgb_device(b, views=VIEWS3[:2], resize=t))
        assert s.error.status == -2 and (host == SENT).all()
    finally:
        s.catch = False
    _check(s, ctx, fulls, VIEWS3, t, 0)                      # and the context still serves a good call


# ---- the batch decoder -------------------------------------------------------------------------
NAMES = ["img2", "img2", "img2", "img4", "img6", "img"]     # the files of test_batch_decoder_crops_every_route
VIEWS = [[(0, 0, 400, 266), (13, 7, 224, 200, True)], [(13, 7, 224, 200, True), (399, 265, 1, 1)], [(399, 265, 1, 1, True), (0, 0, 1, 1)],
         [(100, 50, 512, 300), (0, 0, 800, 400, True)], [(5, 600, 400, 40, True), (0, 0, 427, 640)], [(300, 200, 37, 29), (3, 1, 670, 449, True)]]
OTHER = [[(200, 100, 100, 100, True), (0, 0, 400, 266)]] * 3 + [[(0, 0, 800, 400), (1, 2, 3, 4, True)], [(0, 0, 427, 640, True), (9, 9, 9, 9)],
                                                               [(3, 1, 670, 449), (300, 200, 37, 29, True)]]
BT = (32, 32)


def _gold(name):
    return os.path.join(GOLD, "images", name + ".jpg"), load_golden(name)[3]


def _want(rgb, spec, row, filt=AREA):
    return np.stack([fr.to_format(np.ascontiguousarray(_view_ref(rgb, v, BT, filt)), spec.format, list(spec.scale), list(spec.bias)) for v in row])


def _all_good(imgs, st, tm, rgbs, spec, views, filt=AREA):
    assert tm["rc"] == 0 and st == [0] * len(views), (tm, st)
    for i, row in enumerate(views):
        assert tuple(imgs[i].shape) == (len(row), 3, BT[1], BT[0]), imgs[i].shape
        assert fr.same_bits(np.ascontiguousarray(imgs[i]), _want(rgbs[i], spec, row, filt)), (i, row)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("huff", ["0", None, "2"])
def test_batch_decoder_views_every_route(jb, monkeypatch, huff, threads):
    import torch
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    paths, n = list(paths), len(NAMES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    per = 2 * 3 * BT[0] * BT[1] * 2                          # a file's two f16 outputs
    with jb.BatchDecoder(threads, 0, resize=BT, fmt=spec, arena_bytes=1 << 20) as dec:      # a pinned arena
        _all_good(*dec.run(paths, views=VIEWS), rgbs, spec, VIEWS)
    with jb.BatchDecoder(threads, 0, resize=BT, fmt=spec) as dec:
        # the entropy stage runs once per FILE: the counter rises as it does for one rectangle per file
        n0 = dec.device_entropy_images
        dec.run(paths, crops=[row[0][:4] for row in VIEWS])
        per_file = dec.device_entropy_images - n0
        assert (per_file > 0) if huff == "2" else (per_file == 0) if huff == "0" else True
        n0 = dec.device_entropy_images
        _all_good(*dec.run(paths, views=VIEWS), rgbs, spec, VIEWS)
        assert dec.device_entropy_images - n0 == per_file
        out = torch.full((n, 2, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, views=VIEWS)
        assert ret is out
        _all_good(out.cpu().numpy(), st, tm, rgbs, spec, VIEWS)
        t0 = dec.submit(paths, views=VIEWS)
        t1 = dec.submit(paths, views=OTHER)                  # two in flight, each with its own views
        for t, views in ((t0, VIEWS), (t1, OTHER)):
            _all_good(*dec.collect(t), rgbs, spec, views)
        # one view that does not fit its file: -2 and None for that file only; its slice of the tensor stays
        bad = [list(r) for r in VIEWS]
        bad[1][1] = (13, 7, 388, 200)                        # img2 is 400 wide
        imgs, st, tm = dec.run(paths, views=bad)
        for i in range(n):
            if i == 1:
                assert st[i] == -2 and imgs[i] is None, st
            else:
                assert st[i] == 0 and fr.same_bits(np.ascontiguousarray(imgs[i]), _want(rgbs[i], spec, bad[i])), (i, st)
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, views=bad)
        assert st[1] == -2 and (out[1] == 7.0).all() and fr.same_bits(out[2].cpu().numpy(), _want(rgbs[2], spec, bad[2]))
        # device output: K outputs per file, back to back; a region too small for them is JB_ERR_CAPACITY, nothing partial
        region = torch.full((n * (per + 256) + 256,), SENT, dtype=torch.uint8, device="cuda:0")
        dec.set_device_output(region.data_ptr(), region.numel())
        ptrs, sizes, st, tm = dec.run_to_device(paths, views=VIEWS)
        torch.cuda.synchronize()
        assert tm["rc"] == 0 and st == [0] * n and sizes == [BT] * n
        host = region.cpu().numpy()
        for i in range(n):
            off = ptrs[i] - region.data_ptr()
            assert fr.same_bits(host[off:off + per].view(np.float16).reshape(2, 3, BT[1], BT[0]), _want(rgbs[i], spec, VIEWS[i])), i
        small = torch.full((per - 256,), SENT, dtype=torch.uint8, device="cuda:0")          # one output and most of the second
        dec.set_device_output(small.data_ptr(), small.numel())
        ptrs, sizes, st, tm = dec.run_to_device(paths[:1], views=VIEWS[:1])
        torch.cuda.synchronize()
        assert st == [-5] and ptrs == [0], (st, tm)
        assert (small.cpu().numpy() == SENT).all()
        dec.set_device_output(0, 0)
        # refusals: rows of the wrong count or of unequal length; a scale, a decoder-wide rectangle; no target; K = 17
        for call in (dec.run, dec.submit):
            for views in (VIEWS[:5], VIEWS[:5] + [VIEWS[5][:1]]):
                with pytest.raises(jb.JbError) as e:
                    call(paths, views=views)
                assert e.value.status == -2
        dec.set_roi((0, 0, 100, 100))
        assert dec.run(paths, views=VIEWS)[2]["rc"] == -9
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, views=VIEWS)
        assert e.value.status == -9
        dec.set_roi(None)
        assert dec.run(paths, views=[[VIEWS[i][0]] * 17 for i in range(n)])[2]["rc"] == -2
        dec.set_resize(None)
        imgs, st, tm = dec.run(paths, views=VIEWS)
        assert tm["rc"] == -7 and imgs == [None] * n
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, views=VIEWS)
        assert e.value.status == -7
        dec.set_resize(BT)
        dec.set_filter(BICUBIC)
        _all_good(*dec.run(paths, views=VIEWS), rgbs, spec, VIEWS, BICUBIC)   # the decoder is as good as before, and filters
    with jb.BatchDecoder(threads, 0, scale=2) as dec:
        assert dec.run(paths, views=VIEWS)[2]["rc"] == -9


def test_batch_decoder_views_on_a_multi_device_decoder(jb):
    """file i and its K views go to the same part of a multi-device decoder (here: device 0 twice)"""
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(2, devices=[0, 0], resize=BT, fmt=spec) as dec:
        _all_good(*dec.run(list(paths), views=VIEWS), rgbs, spec, VIEWS)
        _all_good(*dec.collect(dec.submit(list(paths), views=OTHER)), rgbs, spec, OTHER)
