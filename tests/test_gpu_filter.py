"""Resampling filters on the GPU (-m gpu): with resize=(ow, oh) and filter=FILTER_BILINEAR / FILTER_BICUBIC an image of a
launch (or its rectangle roi=, or its own rectangle crops[i]) comes out as
format_ref.to_format(pillow_resize_ref.resize(full, rectangle, (ow, oh), filter), fmt, scale, bias) bit for bit, where full
is the oracle's full-size decode (seam) or the reference's golden RGB (files): never something the code under test
computed, and pillow_resize_ref is held against Pillow's own bits in test_filter_cpu.py.  At the seam the whole
sentinel-filled buffer is compared, pads included."""
import ctypes
import os

import numpy as np
import pytest

import format_ref as fr
import pillow_resize_ref as pr
from conftest import GOLD, load_golden
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, Seam, _oracle_full

pytestmark = pytest.mark.gpu

SETS = list(fr.PARAM_SETS.items())
BILINEAR, BICUBIC = pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
FILTERS = (BILINEAR, BICUBIC)


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


class _Through:
    """What Seam.run sees as its context: the launch goes out with filter= (and crops=), or -- raw -- straight to the
    filtered C entry points (the only way to hand them JB_FILTER_AREA: the Python request routes filter 0 to the old ones).
    catch: a refusal is kept in .error instead of raised."""

    def __init__(self, seam, ctx):
        self.s, self.ctx, self.error = seam, ctx, None

    def blocks_to_rgb_device(self, batch, **kw):
        s, jb = self.s, self.s.jb
        try:
            if s.raw:
                rs = jb.Resize(kw["resize"][0], kw["resize"][1], s.filter, 0)
                spec, roi = kw["fmt"], kw["roi"]
                if s.crops is not None:
                    rois = (jb.Roi * len(s.crops))(*[jb.Roi(*c) for c in s.crops])
                    rc = jb.lib().jb_blocks_to_rgb_device_crops_filtered(self.ctx._h, ctypes.byref(batch), rois, ctypes.byref(rs),
                                                                         ctypes.byref(spec) if spec is not None else None, None)
                else:
                    rc = jb.lib().jb_blocks_to_rgb_device_filtered(self.ctx._h, ctypes.byref(batch), ctypes.byref(jb.Roi(*roi)) if roi else None,
                                                                   ctypes.byref(rs), ctypes.byref(spec) if spec is not None else None, None)
                if rc:
                    raise jb.JbError(rc, jb.lib().jb_last_error(self.ctx._h).decode())
            else:
                self.ctx.blocks_to_rgb_device(batch, crops=s.crops, filter=s.filter, **kw)
        except jb.JbError as e:
            if not s.catch:
                raise
            self.error = e

    def synchronize(self):
        self.ctx.synchronize()


class FilterSeam(Seam):
    """Seam whose run passes filter= (self.filter) and crops= (self.crops)."""
    filter = 0
    crops = None
    raw = False
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        through = _Through(self, ctx)
        out = super().run(through, fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)
        self.error = through.error
        return out


def _check(s, ctx, fulls, rect, target, filt, fmt, scale=(1, 1, 1), bias=(0, 0, 0), crops=None, tag=None):
    """One launch: every image's output is the restatement of its rectangle (`rect` for all, or crops[i]) of fulls[i]."""
    rects = crops if crops is not None else [rect] * len(fulls)
    wants = [pr.resize_to_format(f, r, target, filt, fmt, scale, bias) for f, r in zip(fulls, rects)]
    s.filter, s.crops = filt, (list(crops) if crops is not None else None)
    try:
        return s.check(ctx, wants, fmt, (scale, bias), roi=rect, resize=target, tag=(tag, filt, rect, crops, target))
    finally:
        s.filter, s.crops = 0, None


_frames = {}


def _frame(jb, oracle, w, h, hs, vs, n=1):
    """-> (FilterSeam over n noise images of w x h, the oracle's full-size images), made once and not changed"""
    from jpeg_decoder_amd import synth
    key = (w, h, hs, vs, n)
    if key not in _frames:
        coefs, qs = zip(*[synth.synth_blocks(w, h, hs, vs, image_index=w + h + 7 * i) for i in range(n)])
        fulls = [_oracle_full(oracle, w, h, hs, vs, c, q) for c, q in zip(coefs, qs)]
        seam = FilterSeam(jb, w, h, hs, vs, list(coefs), list(qs), pad_row=3, pad_plane=5, pad_img=7)
        seam.coefs, seam.qs = list(coefs), list(qs)
        _frames[key] = seam, fulls
    return _frames[key]


# ---- layouts, margin, edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_every_layout(jb, ctx, oracle, hs, vs, filt):
    """67 x 45 and 130 x 97: ragged MCUs in both axes in every layout; the whole frame and an interior rectangle."""
    k = hs + 2 * vs + filt
    for w, h in ((67, 45), (130, 97)):
        s, fulls = _frame(jb, oracle, w, h, hs, vs)
        for rect, target in ((None, (29, 19)), ((w // 4, h // 4, w // 2, h // 2), (21, 30))):
            for fmt in (0, 1 + k % 3):
                _check(s, ctx, fulls, rect, target, filt, fmt, *_params(k, fmt), tag=(hs, vs, w, h))
                k += 1


@pytest.mark.parametrize("filt", FILTERS)
def test_seam_margin_comes_from_the_frame(jb, ctx, oracle, filt):
    """An interior rectangle of noise: its edge outputs depend on the pixels outside it, so a kernel that clamps at the
    rectangle instead of the frame computes another image."""
    s, fulls = _frame(jb, oracle, 130, 97, 2, 2)
    for rect, target in (((40, 30, 50, 40), (17, 13)), ((33, 21, 40, 31), (64, 50))):
        assert not np.array_equal(pr.resize(fulls[0], rect, target, filt), pr.resize_rect_clamped(fulls[0], rect, target, filt))
        _check(s, ctx, fulls, rect, target, filt, 0)
        _check(s, ctx, fulls, rect, target, filt, 3, *fr.IMAGENET)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2)])
def test_seam_edges_and_corners(jb, ctx, oracle, hs, vs, filt):
    """A rectangle flush with each frame edge and one in each corner: the window is clamped on those sides only."""
    W, H = 130, 97
    s, fulls = _frame(jb, oracle, W, H, hs, vs)
    rw, rh = 40, 30
    rects = [(0, 20, rw, rh), (W - rw, 20, rw, rh), (30, 0, rw, rh), (30, H - rh, rw, rh),
             (0, 0, rw, rh), (W - rw, 0, rw, rh), (0, H - rh, rw, rh), (W - rw, H - rh, rw, rh)]
    d = jb.make_desc(W, H, hs, vs)
    for k, rect in enumerate(rects):
        win = jb.filter_window(d, (13, 11), filt, roi=rect)
        assert win == pr.window(filt, W, H, rect, (13, 11))
        assert (win[0] == 0) == (rect[0] == 0) and (win[0] + win[2] == W) == (rect[0] + rw == W)
        assert (win[1] == 0) == (rect[1] == 0) and (win[1] + win[3] == H) == (rect[1] + rh == H)
        _check(s, ctx, fulls, rect, (13, 11), filt, 0 if k % 2 else 3, *_params(k, 3), tag=(hs, vs))


# ---- targets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_seam_identity_is_the_slice(jb, ctx, oracle, filt):
    s, fulls = _frame(jb, oracle, 130, 97, 2, 2)
    x, y, w, h = rect = (17, 9, 70, 19)
    host, idx = _check(s, ctx, fulls, rect, (w, h), filt, 0)
    assert np.array_equal(host[idx[0]].reshape(h, w, 3), fulls[0][y:y + h, x:x + w])
    host, idx = _check(s, ctx, fulls, None, (130, 97), filt, 0)
    assert np.array_equal(host[idx[0]].reshape(97, 130, 3), fulls[0])


@pytest.mark.parametrize("filt", FILTERS)
def test_seam_targets_across_tiles_and_enlarging(jb, ctx, oracle, filt):
    """70 x 19 and 130 x 9: more than 64 columns and no multiple of the 8 rows of a workgroup -- tiles in both
    directions, partly empty; 224 x 224 from a 200 x 120 rectangle enlarges both axes over many tiles; 20 x 150 from
    100 x 60 reduces x and enlarges y, 150 x 20 the other way round."""
    s, fulls = _frame(jb, oracle, 130, 97, 2, 1)
    for k, target in enumerate(((70, 19), (130, 9))):
        _check(s, ctx, fulls, None, target, filt, (0, 2)[k], *_params(k, 2))
    s, fulls = _frame(jb, oracle, 233, 131, 2, 2)
    _check(s, ctx, fulls, (21, 7, 200, 120), (224, 224), filt, 3, *fr.IMAGENET)
    _check(s, ctx, fulls, (30, 40, 100, 60), (20, 150), filt, 0)
    _check(s, ctx, fulls, (30, 40, 100, 60), (150, 20), filt, 1)


def test_seam_one_pixel_and_the_tap_cap(jb, ctx, oracle):
    """1 x 1 from 64 x 64: 130 taps per axis under bilinear, next to the cap of 160; under bicubic that reduction counts
    258 taps and is refused with the cap in the text, nothing written -- its 1 x 1 comes from 32 x 32 (130 taps).  One
    pixel's vertical footprint is also longer than the rows of horizontally filtered pixels a workgroup keeps: the
    chunked passes."""
    s, fulls = _frame(jb, oracle, 130, 97, 1, 1)
    _check(s, ctx, fulls, (40, 20, 64, 64), (1, 1), BILINEAR, 0)
    _check(s, ctx, fulls, (40, 20, 64, 64), (1, 1), BILINEAR, 2, *fr.UNIT)
    _check(s, ctx, fulls, (50, 30, 32, 32), (1, 1), BICUBIC, 0)
    _check(s, ctx, fulls, None, (2, 3), BILINEAR, 3, *fr.F16_TIES)       # 130 x 97 -> 2 x 3: 132 x 66 taps
    s.catch, s.filter = True, BICUBIC
    try:
        host, _ = s.run(ctx, 0, (1, 1), roi=(40, 20, 64, 64), resize=(1, 1))
        assert s.error is not None and s.error.status == -9 and "160" in str(s.error), s.error
        assert (host == SENT).all()
        s.crops = [(40, 20, 64, 64)]
        host, _ = s.run(ctx, 0, (1, 1), resize=(1, 1))
        assert s.error is not None and s.error.status == -9 and "160" in str(s.error), s.error
        assert (host == SENT).all()
    finally:
        s.catch, s.filter, s.crops = False, 0, None


# ---- formats and strides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_seam_every_format_every_parameter_set(jb, ctx, oracle, filt, fmt):
    """scale = 1/255, scale = 1 + 2^-11 and ImageNet scale / bias; rows, planes and images at odd strides (the harness
    pads 3, 5 and 7 elements); a batch of two."""
    s, fulls = _frame(jb, oracle, 67, 45, 2, 2, n=2)
    for name, (scale, bias) in SETS if fmt >= 2 else SETS[:1]:
        _check(s, ctx, fulls, (3, 2, 60, 40), (23, 17), filt, fmt, scale, bias, tag=name)
    t, fulls1 = _frame(jb, oracle, 67, 45, 2, 2)
    tight = FilterSeam(jb, 67, 45, 2, 2, t.coefs, t.qs)        # and no padding at all
    _check(tight, ctx, fulls1, None, (23, 17), filt, fmt, *_params(1, fmt), tag="tight")


# ---- per-image rectangles -------------------------------------------------------------------------------------------------
FW, FH = 130, 97
FIVE = [(0, 0, FW, FH),            # the whole image
        (FW - 1, FH - 1, 1, 1),    # the last pixel: 1 x 1, in the corner
        (0, FH - 30, 40, 30),      # the bottom-left corner
        (37, 18, 64, 50),          # interior
        (1, 50, 128, 3)]           # a strip


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_crops_five_rectangles_and_the_single_rectangle_route(jb, ctx, oracle, hs, vs, filt):
    s, fulls = _frame(jb, oracle, FW, FH, hs, vs, n=5)
    target = (21, 13)
    for k, fmt in enumerate((0, 3)):
        host, idx = _check(s, ctx, fulls, None, target, filt, fmt, *_params(k, fmt), crops=FIVE, tag=(hs, vs))
        # image by image what roi= + resize= + filter= writes
        for i, r in enumerate(FIVE):
            one, at = _check(s, ctx, fulls, r, target, filt, fmt, *_params(k, fmt))
            assert np.array_equal(host[idx[i]], one[at[i]]), (i, r, fmt)


def test_crops_more_images_than_a_table_and_windows_decide_the_split(jb, ctx, oracle, monkeypatch):
    """34 images of a 32 x 32 4:4:4 frame (two launch pairs at 32 rows per table); then on a context whose scratch is so
    small that the windows, not the rectangles, decide where the sub-batches end: identical buffers."""
    w = h = 32
    n = 34
    s, fulls = _frame(jb, oracle, w, h, 1, 1, n=n)
    rng = np.random.default_rng(34)
    crops = []
    for _ in range(n):
        cw, ch = int(rng.integers(4, 17)), int(rng.integers(4, 17))
        crops.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    crops[5], crops[33] = (31, 0, 1, 1), (0, 0, w, h)
    target = (6, 5)
    d = jb.make_desc(w, h, 1, 1)

    def split(sizes, cap):
        out, i = [], 0
        while i < n:
            m, tot = 1, sizes[i]
            while i + m < n and m < 32 and tot + sizes[i + m] <= cap:
                tot += sizes[i + m]
                m += 1
            out.append(m)
            i += m
        return out

    for filt in FILTERS:
        first = {fmt: _check(s, ctx, fulls, None, target, filt, fmt, *_params(2, fmt), crops=crops)[0] for fmt in (0, 3)}
        wins = [jb.filter_window(d, target, filt, roi=r) for r in crops]
        assert wins == [pr.window(filt, w, h, r, target) for r in crops]
        by_window, by_rect = [3 * a[2] * a[3] for a in wins], [3 * r[2] * r[3] for r in crops]
        cap = 1500
        assert split(by_window, cap) != split(by_rect, cap) and max(by_window) > cap > min(by_window)
        monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
        with jb.Context(0) as small:                      # (the knob is read when a context is created)
            for fmt in (0, 3):
                s.filter, s.crops = filt, crops
                try:
                    host, _ = s.run(small, fmt, target, _params(2, fmt), resize=target)
                finally:
                    s.filter, s.crops = 0, None
                assert np.array_equal(host, first[fmt]), (filt, fmt)
        monkeypatch.delenv("JPEGBLK_RESIZE_TMP_BYTES")


def test_single_rectangle_batch_in_sub_batches(jb, ctx, oracle, monkeypatch):
    """Five images, one rectangle: a scratch that holds two windows (but three rectangles) runs 2 + 2 + 1."""
    s, fulls = _frame(jb, oracle, FW, FH, 2, 2, n=5)
    rect, target = (37, 18, 64, 50), (9, 7)
    win = jb.filter_window(jb.make_desc(FW, FH, 2, 2), target, BICUBIC, roi=rect)
    cap = 3 * win[2] * win[3] * 5 // 2
    assert 3 * rect[2] * rect[3] * 3 <= cap
    first = _check(s, ctx, fulls, rect, target, BICUBIC, 3, *fr.IMAGENET)[0]
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
    with jb.Context(0) as small:
        assert np.array_equal(_check(s, small, fulls, rect, target, BICUBIC, 3, *fr.IMAGENET)[0], first)


# ---- FILTER_AREA through the new entry points -------------------------------------------------------------------------------
def test_filter_area_through_the_new_entry_points_is_todays_output(jb, ctx, oracle):
    s, fulls = _frame(jb, oracle, FW, FH, 2, 2, n=5)
    for fmt in (0, 3):
        for rect, target in ((None, (29, 19)), ((37, 18, 64, 50), (80, 9))):
            src = [f if rect is None else f[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] for f in fulls]
            wants = [fr.to_format(area_resize(x, *target), fmt, *_params(0, fmt)) for x in src]
            old, _ = s.check(ctx, wants, fmt, _params(0, fmt), roi=rect, resize=target)       # jb_blocks_to_rgb_device_resized
            s.raw = True
            try:
                new, _ = s.check(ctx, wants, fmt, _params(0, fmt), roi=rect, resize=target)   # _filtered with JB_FILTER_AREA
            finally:
                s.raw = False
            assert np.array_equal(old, new)
        wants = [fr.to_format(area_resize(f[r[1]:r[1] + r[3], r[0]:r[0] + r[2]], 21, 13), fmt, *_params(0, fmt)) for f, r in zip(fulls, FIVE)]
        s.crops = FIVE
        try:
            old, _ = s.check(ctx, wants, fmt, _params(0, fmt), resize=(21, 13))               # jb_blocks_to_rgb_device_crops
            s.raw = True
            new, _ = s.check(ctx, wants, fmt, _params(0, fmt), resize=(21, 13))               # _crops_filtered with JB_FILTER_AREA
        finally:
            s.raw, s.crops = False, None
        assert np.array_equal(old, new)


# ---- files ----------------------------------------------------------------------------------------------------------------
def _gold(name):
    return os.path.join(GOLD, "images", name + ".jpg"), load_golden(name)[3]


@pytest.mark.parametrize("huff", ["2", "0"])
@pytest.mark.parametrize("name", ["img2", "img4"])
def test_decode_file_and_memory_filtered_golden(jb, monkeypatch, name, huff):
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    path, rgb = _gold(name)
    h, w = rgb.shape[:2]
    data = open(path, "rb").read()
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.Context(0) as c:   # (the knob is read when the context is created)
        for k, (roi, t) in enumerate(((None, (56, 40)), ((w // 4, h // 4, w // 2, h // 2), (33, 47)), ((w - 3, h - 2, 3, 2), (8, 8)))):
            filt = FILTERS[k % 2] if huff == "2" else FILTERS[(k + 1) % 2]
            for fmt, sp in ((0, None), (3, spec)):
                want = pr.resize_to_format(rgb, roi, t, filt, fmt, list(spec.scale), list(spec.bias))
                assert fr.same_bits(c.decode_file(path, fmt=sp, roi=roi, resize=t, filter=filt), want), (name, roi, t, fmt)
                assert fr.same_bits(c.decode_memory(data, fmt=sp, roi=roi, resize=t, filter=filt), want), (name, roi, t, fmt)
        with pytest.raises(jb.JbError) as e:
            c.decode_file(path, resize=(8, 8), filter=5)
        assert e.value.status == -2
        with pytest.raises(jb.JbError) as e:
            c.decode_memory(data, resize=(2, 2), filter=BICUBIC)       # more than 160 taps
        assert e.value.status == -9 and "160" in str(e.value)
        assert np.array_equal(c.decode_file(path), rgb)   # and the context still decodes whole images


NAMES = ["img2", "img4", "img6", "img", "img2"]     # 400x266 4:2:0, 800x400 4:4:4, 427x640 4:2:0, 679x451 4:2:0
CROPS = [(0, 0, 400, 266), (100, 50, 512, 300), (5, 600, 400, 40), (300, 200, 37, 29), (399, 265, 1, 1)]
BT = (32, 32)


def test_batch_decoder_set_filter(jb):
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    paths, n = list(paths), len(NAMES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.BatchDecoder(4, 0, fmt=spec, resize=BT, filter=BILINEAR) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert fr.same_bits(imgs[i], pr.resize_to_format(rgbs[i], None, BT, BILINEAR, 3, *sb)), i
        dec.set_filter(BICUBIC)                             # governs the per-image rectangles too
        imgs, st, tm = dec.run(paths, crops=CROPS)
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert fr.same_bits(imgs[i], pr.resize_to_format(rgbs[i], CROPS[i], BT, BICUBIC, 3, *sb)), i
        t0 = dec.submit(paths, crops=CROPS)                 # the twin side has the filter too
        t1 = dec.submit(paths)
        with pytest.raises(jb.JbError) as e:
            dec.set_filter(BILINEAR)
        assert e.value.status == -7
        for t, rects in ((t0, CROPS), (t1, [None] * n)):
            imgs, st, tm = dec.collect(t)
            assert tm["rc"] == 0 and st == [0] * n, (tm, st)
            for i in range(n):
                assert fr.same_bits(imgs[i], pr.resize_to_format(rgbs[i], rects[i], BT, BICUBIC, 3, *sb)), i
        # a target that asks one file for more taps than the cap: -9 for that file only
        dec.set_resize((20, 20))
        imgs, st, tm = dec.run(paths)
        for i in range(n):
            if NAMES[i] == "img4":                          # 800 wide: 4 * 40 + 2 taps
                assert st[i] == -9 and imgs[i] is None, st
            else:
                assert st[i] == 0 and fr.same_bits(imgs[i], pr.resize_to_format(rgbs[i], None, (20, 20), BICUBIC, 3, *sb)), (i, st)
        with pytest.raises(jb.JbError) as e:
            dec.set_filter(3)
        assert e.value.status == -2
        dec.set_filter(jb.FILTER_AREA)                      # and the area filter again
        dec.set_resize(BT)
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert fr.same_bits(imgs[i], fr.to_format(area_resize(rgbs[i], *BT), 3, *sb)), i


# ---- Pillow itself ----------------------------------------------------------------------------------------------------------
def test_device_output_equals_pillow(jb, ctx, oracle):
    Image = pytest.importorskip("PIL.Image")
    s, fulls = _frame(jb, oracle, 233, 131, 2, 2)
    x, y, w, h = rect = (21, 7, 200, 120)
    for filt, resample, target in ((BILINEAR, Image.BILINEAR, (56, 56)), (BICUBIC, Image.BICUBIC, (224, 224))):
        want = np.asarray(Image.fromarray(fulls[0]).resize(target, resample, box=(x, y, x + w, y + h)))
        s.filter = filt
        try:
            s.check(ctx, [want], 0, roi=rect, resize=target)
        finally:
            s.filter = 0
