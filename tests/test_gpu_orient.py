"""Orientation on the GPU (-m gpu): under orientation o every output option acts on T_o(full), where full is the SAME
context arithmetic's orientation-1 full-size output (itself held against the oracle, libjpeg and Pillow by the other
GPU tests) and T_o is numpy's (orient_ref.py); behind T_o come the existing numpy references of the options
(format_ref, resize_ref, pillow_resize_ref).  At the seam whole sentinel-filled buffers are compared, pads included."""
import ctypes

import numpy as np
import pytest

import format_ref as fr
import orient_ref as ot
import pillow_resize_ref as pr
from libjpeg_ref import load_kat
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, Seam

pytestmark = pytest.mark.gpu

T = 64                      # jb_orient_kernel's tile (csrc/jb_orient.h kJbOrientTile)
AREA, BILINEAR, BICUBIC = pr.FILTER_AREA, pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
PADS = (3, 5, 7)


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


class _Through:
    """What Seam.run sees as its context: the launch goes out with crops= and filter= too; catch: a refusal is kept in
    .error instead of raised, so that run() still returns the buffer the refused call was given."""

    def __init__(self, seam, ctx):
        self.s, self.ctx, self.error = seam, ctx, None

    def blocks_to_rgb_device(self, batch, **kw):
        try:
            self.ctx.blocks_to_rgb_device(batch, crops=self.s.crops, filter=self.s.filter, **kw)
        except self.s.jb.JbError as e:
            if not self.s.catch:
                raise
            self.error = e

    def synchronize(self):
        self.ctx.synchronize()


class OrientSeam(Seam):
    crops = None
    filter = AREA
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        through = _Through(self, ctx)
        out = super().run(through, fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)
        self.error = through.error
        return out


_frames, _fulls = {}, {}


def _frame(jb, w, h, hs, vs, n=1):
    """-> OrientSeam over n noise images of w x h, made once"""
    from jpeg_decoder_amd import synth
    key = (w, h, hs, vs, n)
    if key not in _frames:
        coefs, qs = zip(*[synth.synth_blocks(w, h, hs, vs, image_index=w + 3 * h + 7 * i) for i in range(n)])
        _frames[key] = OrientSeam(jb, w, h, hs, vs, list(coefs), list(qs))
        _frames[key].key = key
    return _frames[key]


def _full(jb, s, arithmetic=0):
    """-> the orientation-1 full-size images [n, H, W, 3] of `s` in an arithmetic, from a context whose orientation was
    never set: computed once, shared, not changed"""
    key = s.key + (arithmetic,)
    if key not in _fulls:
        w, h = s.desc.width, s.desc.height
        pads, s.pads = s.pads, (0, 0, 0)
        with jb.Context(0, arithmetic=arithmetic) as plain:
            host, idx = s.run(plain, 0, (w, h))
        s.pads = pads
        _fulls[key] = host[idx].reshape(s.n, h, w, 3).copy()
        _fulls[key].flags.writeable = False
    return _fulls[key]


def _cut(a, r):
    x, y, w, h = r
    return a[y:y + h, x:x + w]


def _want(full, o, fmt, params, roi=None, resize=None, filt=AREA):
    """The contract: orientation first, then the option's own reference."""
    a = ot.orient(full, o)
    if resize is None:
        out = a if roi is None else _cut(a, roi)
    elif filt == AREA:
        out = area_resize(a if roi is None else _cut(a, roi), *resize)
    else:
        out = pr.resize(a, roi, resize, filt)
    return fr.to_format(np.ascontiguousarray(out), fmt, *params)


def _check(s, ctx, fulls, o, fmt, params=NO_PARAMS, roi=None, resize=None, filt=AREA, crops=None):
    rois = crops if crops is not None else [roi] * len(fulls)
    wants = [_want(f, o, fmt, params, r, resize, filt) for f, r in zip(fulls, rois)]
    s.filter, s.crops = filt, (list(crops) if crops is not None else None)
    try:
        return s.check(ctx, wants, fmt, params, roi=roi, resize=resize, tag=("orientation", o, filt, crops))
    finally:
        s.filter, s.crops = AREA, None


# ---- 1. the seam without a target size -------------------------------------------------------------------------------------
SIZES = [(1, 1, 1), (1, T + 3, 1), (T + 3, 1, 1), (T - 1, T + 1, 1), (2 * T + 5, T + 9, 3)]


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_every_orientation(jb, hs, vs):
    """Sizes around the tile, o = 1..8: format 0 with tight rows (an odd stride: every width here is odd) and with padded
    ones, normalised f16 with padded rows, planes and images.  Orientation 1 is the buffer of a context never set."""
    with jb.Context(0) as ctx, jb.Context(0) as never_set:
        for w, h, n in SIZES:
            s = _frame(jb, w, h, hs, vs, n)
            fulls = _full(jb, s)
            for o in range(1, 9):
                ctx.set_orientation(o)
                assert ctx.orientation == o
                for pads, fmt, params in (((0, 0, 0), 0, NO_PARAMS), (PADS, 0, NO_PARAMS), (PADS, 3, fr.IMAGENET)):
                    s.pads = pads
                    host, _ = _check(s, ctx, fulls, o, fmt, params)
                    if o == 1:
                        assert np.array_equal(host, s.run(never_set, fmt, (w, h), params)[0])
            s.pads = (0, 0, 0)


def test_seam_other_planar_formats(jb):
    """Planar uint8 and f32 (the two formats the test above leaves out), a transposing and a mirroring orientation."""
    s = _frame(jb, 2 * T + 5, T + 9, 2, 2, 3)
    fulls = _full(jb, s)
    s.pads = PADS
    with jb.Context(0) as ctx:
        for o in (4, 7):
            ctx.set_orientation(o)
            _check(s, ctx, fulls, o, 1)
            _check(s, ctx, fulls, o, 2, fr.UNIT)
    s.pads = (0, 0, 0)


# ---- 2. roi= in oriented coordinates ---------------------------------------------------------------------------------------
W, H = 131, 70


@pytest.mark.parametrize("o", [2, 6, 7])
def test_roi_is_in_oriented_coordinates(jb, o):
    s = _frame(jb, W, H, 2, 2)
    fulls = _full(jb, s)
    ow, oh = ot.size(W, H, o)
    rects = [(0, 9, 30, 21), (ow - 30, 5, 30, 21), (9, 0, 30, 21), (11, oh - 21, 30, 21), (0, 0, ow, oh), (ow - 1, oh - 1, 1, 1),
             (17, 13, 33, 40)]
    if o >= 5:
        rects.append((3, 50, 60, 81))       # taller than the stored frame: width and height have swapped for real
        assert rects[-1][3] > H and jb.lib().jb_orient_check(ctypes.byref(s.desc), 1, 1, ctypes.byref(jb.Roi(*rects[-1]))) == -2
    s.pads = PADS
    with jb.Context(0, orientation=o) as ctx:
        for k, r in enumerate(rects):
            _check(s, ctx, fulls, o, 0 if k % 2 else 3, NO_PARAMS if k % 2 else fr.IMAGENET, roi=r)
        # a rectangle of the stored frame that the oriented one does not hold
        if o >= 5:
            s.catch = True
            host, _ = s.run(ctx, 0, (100, 20), roi=(20, 10, 100, 20))
            s.catch = False
            assert s.error is not None and s.error.status == -2 and np.all(host == SENT)
    s.pads = (0, 0, 0)


# ---- 3. resize= and filter= ------------------------------------------------------------------------------------------------
TARGET = (48, 40)


def test_rotating_last_is_another_image(jb):
    """The reason orientation comes first: Pillow filters horizontally, rounds to uint8, then vertically, so for a
    transposing orientation resizing T_o(full) and turning the resized stored image disagree."""
    full = _full(jb, _frame(jb, W, H, 2, 2))[0]
    for o in (5, 8):
        first = pr.resize(ot.orient(full, o), None, TARGET, BICUBIC)
        last = ot.orient(pr.resize(full, None, TARGET[::-1], BICUBIC), o)
        assert first.shape == last.shape and np.count_nonzero(first != last) >= 1


@pytest.mark.parametrize("o", [3, 5, 8])
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_resize_and_filters(jb, hs, vs, o):
    s = _frame(jb, W, H, hs, vs)
    fulls = _full(jb, s)
    ow, oh = ot.size(W, H, o)
    rect = (ow // 5, oh // 7, ow // 2 + 3, oh // 3 + 1)      # asymmetric, in oriented coordinates
    s.pads = PADS
    with jb.Context(0, orientation=o) as ctx:
        for k, filt in enumerate((AREA, BILINEAR, BICUBIC)):
            for roi in (None, rect):
                _check(s, ctx, fulls, o, 0, roi=roi, resize=TARGET, filt=filt)
                _check(s, ctx, fulls, o, 3, fr.IMAGENET, roi=roi, resize=TARGET, filt=filt)
                if filt != AREA:    # the window the caller can ask for is the oriented frame's
                    d = jb.make_desc(ow, oh, hs, vs)
                    assert jb.filter_window(d, TARGET, filt, roi=roi) == pr.window(filt, ow, oh, roi or (0, 0, ow, oh), TARGET)
    s.pads = (0, 0, 0)


def test_resize_and_filters_three_images_in_one_sub_batch(jb):
    """Three images, no cap: images 1 and 2 of the second scratch region are read at their own offsets."""
    s = _frame(jb, W, H, 2, 2, 3)
    fulls = _full(jb, s)
    s.pads = PADS
    with jb.Context(0, orientation=6) as ctx:
        for filt in (AREA, BILINEAR, BICUBIC):
            _check(s, ctx, fulls, 6, 0, resize=TARGET, filt=filt)
            _check(s, ctx, fulls, 6, 3, fr.IMAGENET, roi=(3, 50, 60, 81), resize=TARGET, filt=filt)
    s.pads = (0, 0, 0)


# ---- 4. crops= -------------------------------------------------------------------------------------------------------------
def test_crops(jb, monkeypatch):
    """Three images, three rectangles of the oriented 70 x 131 frame, o = 6; then again with a scratch cap that forces one
    image per sub-batch, on a fresh context."""
    o = 6
    s = _frame(jb, W, H, 2, 2, 3)
    fulls = _full(jb, s)
    ow, oh = ot.size(W, H, o)
    crops = [(0, 0, ow, oh), (ow - 9, 3, 9, 100), (5, oh - 33, 40, 33)]
    s.pads = PADS
    first = {}
    with jb.Context(0, orientation=o) as ctx:
        for filt in (AREA, BILINEAR):
            first[filt] = _check(s, ctx, fulls, o, 3, fr.IMAGENET, resize=(32, 24), filt=filt, crops=crops)[0]
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", "1000")     # less than any of the three: every image runs alone
    with jb.Context(0, orientation=o) as small:                  # (the knob is read when a context is created)
        for filt in (AREA, BILINEAR):
            assert np.array_equal(_check(s, small, fulls, o, 3, fr.IMAGENET, resize=(32, 24), filt=filt, crops=crops)[0], first[filt])
        # and the single-rectangle routes in sub-batches of one image
        _check(s, small, fulls, o, 0)
        _check(s, small, fulls, o, 3, fr.IMAGENET, roi=(3, 50, 60, 81), resize=TARGET, filt=BICUBIC)
    monkeypatch.delenv("JPEGBLK_RESIZE_TMP_BYTES")
    s.pads = (0, 0, 0)


# ---- 5. JB_ARITH_LIBJPEG ---------------------------------------------------------------------------------------------------
def test_under_libjpeg_arithmetic(jb):
    """One case each of 1, 2 and 3 with the orientation-1 output of THAT arithmetic as full."""
    s = _frame(jb, W, H, 2, 2)
    fulls = _full(jb, s, jb.ARITH_LIBJPEG)
    assert not np.array_equal(fulls, _full(jb, s))         # (it is another decode)
    s.pads = PADS
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, orientation=6) as ctx:
        _check(s, ctx, fulls, 6, 3, fr.IMAGENET)
        _check(s, ctx, fulls, 6, 0, roi=(3, 50, 60, 81))
        _check(s, ctx, fulls, 6, 0, roi=(3, 50, 60, 81), resize=TARGET, filt=BICUBIC)
        _check(s, ctx, fulls, 6, 3, fr.IMAGENET, resize=TARGET)
    s.pads = (0, 0, 0)
    s3 = _frame(jb, W, H, 2, 2, 3)
    f3 = _full(jb, s3, jb.ARITH_LIBJPEG)
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, orientation=8) as ctx:
        _check(s3, ctx, f3, 8, 0, resize=(32, 24), filt=BILINEAR, crops=[(0, 0, 70, 131), (61, 3, 9, 100), (5, 98, 40, 33)])


# ---- 6. files --------------------------------------------------------------------------------------------------------------
FILES = ["420_521x37_noise_q95", "gray_33x21", "420_45x35_progressive"]


@pytest.mark.parametrize("huff", ["0", "2"])
def test_decode_memory_takes_the_tag(jb, monkeypatch, huff):
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    kat = {name: data for name, data, _ in load_kat()}
    with jb.Context(0) as plain, jb.Context(0, orientation=jb.ORIENT_EXIF) as ctx:   # (the knob is read at creation)
        for name in FILES:
            full = plain.decode_memory(kat[name])
            assert np.array_equal(ctx.decode_memory(kat[name]), full)                 # no tag: as stored
            for o in (1, 3, 6, 8):
                tagged = ot.splice(kat[name], ot.exif_app1(o, big=(o == 6)))
                assert jb.exif_orientation(tagged) == o
                assert np.array_equal(plain.decode_memory(tagged), full)              # (a context never set ignores it)
                got = ctx.decode_memory(tagged)
                assert got.shape == ot.orient(full, o).shape and np.array_equal(got, ot.orient(full, o)), (name, o)
            tagged = ot.splice(kat[name], ot.exif_app1(6))
            oh, ow = ot.orient(full, 6).shape[:2]
            t = (max(ow // 2, 1), max(oh // 3, 1))
            assert np.array_equal(ctx.decode_memory(tagged, resize=t, filter=BICUBIC), pr.resize(ot.orient(full, 6), None, t, BICUBIC)), name
            spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
            roi = (0, oh // 2, ow, oh - oh // 2)
            assert fr.same_bits(ctx.decode_memory(tagged, fmt=spec, roi=roi), fr.to_format(_cut(ot.orient(full, 6), roi), 3, *fr.IMAGENET)), name
        # an explicit value overrides the tag
        ctx.set_orientation(2)
        name = FILES[0]
        assert np.array_equal(ctx.decode_memory(ot.splice(kat[name], ot.exif_app1(6))), ot.orient(plain.decode_memory(kat[name]), 2))


def test_decode_file_takes_the_tag(jb, tmp_path):
    data = {name: d for name, d, _ in load_kat()}[FILES[0]]
    p = tmp_path / "tagged.jpg"
    p.write_bytes(ot.splice(data, ot.exif_app1(8, big=True)))
    with jb.Context(0) as plain, jb.Context(0, orientation=jb.ORIENT_EXIF) as ctx:
        assert np.array_equal(ctx.decode_file(str(p)), ot.orient(plain.decode_file(str(p)), 8))


# ---- 7. the batch decoder --------------------------------------------------------------------------------------------------
ORDER = [1, 6, 6, 3, 1, 8, 8, 8]


@pytest.mark.parametrize("huff", ["0", "2"])
def test_batch_decoder_groups_by_orientation(jb, monkeypatch, tmp_path, huff):
    """Eight files of one geometry whose tags change in the middle of what would be one group."""
    import torch
    from jpeg_decoder_amd import synth
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    w, h = 70, 40
    paths, fulls = [], []
    with jb.Context(0) as plain:
        for i, o in enumerate(ORDER):
            coef, q = synth.synth_blocks(w, h, 2, 2, image_index=40 + i)
            data = synth.encode_jpeg(coef, w, h, 2, 2, q, (0, 1, 1), restart_interval=1)
            fulls.append(plain.decode_memory(data))
            paths.append(str(tmp_path / f"f{i}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(ot.splice(data, ot.exif_app1(o, big=bool(i & 1))))
    want = [ot.orient(f, o) for f, o in zip(fulls, ORDER)]
    with jb.BatchDecoder(2, 0, orientation=jb.ORIENT_EXIF) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * 8, (tm, st)
        for i in range(8):
            assert imgs[i].shape == want[i].shape and np.array_equal(imgs[i], want[i]), (i, ORDER[i])
        # rectangles of the oriented frames, one output size
        crops = [(3, 2, ot.size(w, h, o)[0] - 7, ot.size(w, h, o)[1] - 5) for o in ORDER]
        crops[2] = (0, 0, 40, 70)
        crops[5] = (39, 69, 1, 1)
        dec.set_resize((32, 32))
        wants = [area_resize(_cut(a, r), 32, 32) for a, r in zip(want, crops)]
        imgs, st, tm = dec.run(paths, crops=crops)
        assert tm["rc"] == 0 and st == [0] * 8, (tm, st)
        for i in range(8):
            assert np.array_equal(imgs[i], wants[i]), (i, ORDER[i])
        out = torch.full((8, 32, 32, 3), 7, dtype=torch.uint8, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, crops=crops)
        assert ret is out and st == [0] * 8, (st, tm)
        assert np.array_equal(out.cpu().numpy(), np.stack(wants))
        # a rectangle that only the stored frame holds: that file alone is refused
        crops[1] = (0, 0, 70, 40)
        imgs, st, tm = dec.run(paths, crops=crops)
        assert st == [0, -2, 0, 0, 0, 0, 0, 0], st
    with jb.BatchDecoder(2, 0, orientation=6) as dec:                 # an explicit value, whatever the files say
        imgs, st, tm = dec.run(paths[:4])
        assert st == [0] * 4 and all(np.array_equal(imgs[i], ot.orient(fulls[i], 6)) for i in range(4))


# ---- 7b. the host seam --------------------------------------------------------------------------------------------------
def test_host_seam_is_sized_for_the_oriented_frame(jb):
    """Context.blocks_to_rgb / submit / submit_batch on a landscape 100 x 50 frame: a transposing orientation gives 100
    rows of 50 pixels, and a buffer of the stored frame's shape is refused before anything is written."""
    from jpeg_decoder_amd import synth
    w, h = 100, 50
    desc = jb.make_desc(w, h, 2, 2)
    coef, q = synth.synth_blocks(w, h, 2, 2, image_index=5)
    g = jb.geometry_of(desc)
    with jb.Context(0, 2 * g.coef_bytes, 2 * g.rgb_bytes) as ctx:
        full = ctx.blocks_to_rgb(desc, coef, q)
        assert full.shape == (h, w, 3)
        for o in (6, 3, 5):
            ctx.set_orientation(o)
            want = ot.orient(full, o)
            got = ctx.blocks_to_rgb(desc, coef, q)
            assert got.shape == want.shape and np.array_equal(got, want), o
            ow, oh = ot.size(w, h, o)
            stride = 3 * ow + 6
            assert np.array_equal(ctx.blocks_to_rgb(desc, coef, q, stride=stride), want), o
            out = np.full((oh, stride), SENT, np.uint8)
            ctx.wait(ctx.submit(desc, coef, q, out, stride))
            assert np.array_equal(out[:, :3 * ow].reshape(oh, ow, 3), want) and np.all(out[:, 3 * ow:] == SENT), o
            both = np.full((2, oh, 3 * ow), SENT, np.uint8)
            ctx.wait(ctx.submit_batch(desc, np.stack([coef, coef]), np.stack([q, q]), both))
            assert np.array_equal(both[0].reshape(oh, ow, 3), want) and np.array_equal(both[1], both[0]), o
        ctx.set_orientation(6)
        small = np.full((h, 3 * w + 1), SENT, np.uint8)          # the stored frame's shape, a stride the C side accepts
        with pytest.raises(jb.JbError) as e:
            ctx.submit(desc, coef, q, small, 3 * w + 1)
        assert e.value.status == -2 and np.all(small == SENT)
        with pytest.raises(jb.JbError) as e:
            ctx.blocks_to_rgb(desc, coef, q, stride=3 * 50 - 1)
        assert e.value.status == -2
        with pytest.raises(jb.JbError) as e:
            ctx.submit_batch(desc, np.stack([coef, coef]), np.stack([q, q]), np.zeros((2, h, 3 * w - 3), np.uint8))
        assert e.value.status == -2
        ctx.set_orientation(jb.ORIENT_EXIF)
        for call in (lambda: ctx.blocks_to_rgb(desc, coef, q), lambda: ctx.submit(desc, coef, q, small),
                     lambda: ctx.submit_batch(desc, coef[None], q[None], small[None])):
            with pytest.raises(jb.JbError) as e:
                call()
            assert e.value.status == -7
        assert np.all(small == SENT)
        ctx.set_orientation(jb.ORIENT_STORED)
        assert np.array_equal(ctx.blocks_to_rgb(desc, coef, q), full)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(jb):
    s = _frame(jb, W, H, 2, 2)
    fulls = _full(jb, s)
    data = {name: d for name, d, _ in load_kat()}[FILES[0]]
    with jb.Context(0) as ctx:
        first = _check(s, ctx, fulls, 1, 0)[0]
        ctx.set_orientation(3)
        s.catch = True
        try:
            host, _ = s.run(ctx, 0, jb.scaled_size(W, H, 2), scale=2)
            assert s.error is not None and s.error.status == -9 and np.all(host == SENT)
            with pytest.raises(jb.JbError) as e:
                ctx.decode_memory(data, scale=2)
            assert e.value.status == -9
            ctx.set_orientation(jb.ORIENT_EXIF)
            host, _ = s.run(ctx, 0, (W, H))
            assert s.error is not None and s.error.status == -7 and np.all(host == SENT)
            host, _ = s.run(ctx, 3, TARGET, fr.IMAGENET, resize=TARGET)
            assert s.error is not None and s.error.status == -7 and np.all(host == SENT)
            host, _ = s.run(ctx, 0, jb.scaled_size(W, H, 2), scale=2)          # no file: -7, with a scale too
            assert s.error is not None and s.error.status == -7 and np.all(host == SENT)
        finally:
            s.catch = False
        for bad in (9, -1):
            with pytest.raises(jb.JbError) as e:
                ctx.set_orientation(bad)
            assert e.value.status == -2 and ctx.orientation == jb.ORIENT_EXIF
        ctx.set_orientation(jb.ORIENT_STORED)
        assert np.array_equal(_check(s, ctx, fulls, 1, 0)[0], first)
    for kw in (dict(scale=2, orientation=6), dict(scale=4, orientation=jb.ORIENT_EXIF)):
        with pytest.raises(jb.JbError) as e:
            jb.BatchDecoder(2, 0, **kw)
        assert e.value.status == -9
    with jb.BatchDecoder(2, 0, orientation=6) as dec:
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(2)
        assert e.value.status == -9
        with pytest.raises(jb.JbError) as e:
            dec.set_orientation(9)
        assert e.value.status == -2
        dec.set_orientation(jb.ORIENT_STORED)
        dec.set_scale(2)
