"""Fit on the GPU (-m gpu): letterbox (FIT_PAD) and centred crop (FIT_COVER) targets against tests/fit_ref.py, bit for bit.
`full` is the SAME context arithmetic's (and orientation's) full-size output -- itself held against the oracle, libjpeg and
Pillow by the other GPU tests -- or, for the libjpeg cases, Pillow's own decode from tests/golden/libjpeg_decode_kat.npz:
never something the code under test computed.  At the seam the whole sentinel-filled buffer is compared, odd lead and
pads included, so a fill that leaves its bands or an inner rectangle that is misplaced by one element is a failure."""
import numpy as np
import pytest

import fit_ref
import format_ref as fr
import libjpeg_ref
import orient_ref as ot
import pillow_resize_ref as pr
from resize_ref import area_resize
from seam_harness import NO_PARAMS, SENT, Seam

pytestmark = pytest.mark.gpu

AREA, BILINEAR, BICUBIC = pr.FILTER_AREA, pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
PAD, COVER = fit_ref.PAD, fit_ref.COVER
ANCHORS = (fit_ref.CENTER, fit_ref.START, fit_ref.END)
TARGETS = [(16, 16), (15, 16), (16, 13)]
FILL = (124, 116, 104)
KAT = libjpeg_ref.load_kat()
NAMES = [n for n, _, _ in KAT]


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


class FitSeam(Seam):
    """Seam whose launches also carry fit=, filter=, crops= and views= (attributes); catch: a refusal is kept in .error."""
    fit = None
    filter = 0
    crops = None
    views = None
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        seam = self

        class Through:
            def blocks_to_rgb_device(self, batch, **kw):
                try:
                    ctx.blocks_to_rgb_device(batch, fit=seam.fit, filter=seam.filter, crops=seam.crops, views=seam.views, **kw)
                except seam.jb.JbError as e:
                    if not seam.catch:
                        raise
                    seam.error = e

            def synchronize(self):
                ctx.synchronize()

        self.error = None
        return super().run(Through(), fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)


_frames, _fulls = {}, {}


def _frame(jb, w, h, hs, vs, n=3):
    """-> FitSeam over n noise images of w x h, each with quantisation tables of its own; made once"""
    from jpeg_decoder_amd import synth
    key = (w, h, hs, vs, n)
    if key not in _frames:
        coefs, qs = zip(*[synth.synth_blocks(w, h, hs, vs, image_index=w + 3 * h + 7 * i, qtabs=synth.annex_k_qtabs(90 - 15 * i)) for i in range(n)])
        _frames[key] = FitSeam(jb, w, h, hs, vs, list(coefs), list(qs))
        _frames[key].key = key
    return _frames[key]


def _full(jb, s, arithmetic=0):
    """-> the full-size images [n, H, W, 3] of `s` from a plain context: computed once, shared, not changed"""
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


def _pads(target):
    """an odd row stride in the uint8 formats, a gap behind every plane and image"""
    return (3 if target[0] % 2 == 0 else 2, 5, 7)


_refs = {}


def _ref_u8(full, roi, target, mode, anchor, fill, filt):
    """fit_ref's uint8 answer, computed once per request (the formats share it)"""
    key = (full.__array_interface__["data"][0], full.shape, roi, target, mode, anchor, fill, filt)
    if key not in _refs:
        _refs[key] = (full, fit_ref.fit_u8(full, roi, target, mode, anchor, fill, filt))    # (holds `full`: its address stays its own)
    return _refs[key][1]


def _check(jb, s, ctx, fulls, target, mode, anchor, filt, fmt, params=NO_PARAMS, roi=None, fill=FILL):
    wants = [fr.to_format(_ref_u8(f, roi, target, mode, anchor, fill, filt), fmt, *params) for f in fulls]
    s.pads = _pads(target)
    s.fit, s.filter = (jb.Fit.pad(fill, anchor) if mode == PAD else jb.Fit.cover(anchor)), filt
    try:
        return s.check(ctx, wants, fmt, params, roi=roi, resize=target, tag=("fit", mode, anchor, filt))
    finally:
        s.fit, s.filter, s.pads = None, 0, (0, 0, 0)


# ---- 1. the seam: both modes, three anchors, three filters, four formats ---------------------------------------------------
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
@pytest.mark.parametrize("w,h", [(37, 23), (23, 37)])
def test_seam_modes_anchors_filters_formats(jb, ctx, w, h, hs, vs):
    """A batch of three images with tables per image; the targets pad (and cut) on either axis: 37 x 23 letterboxed into
    16 x 16 has bands of 3 rows, into 16 x 13 bands of 2 and 1, 23 x 37 into 15 x 16 bands of 2 and 3 columns."""
    s = _frame(jb, w, h, hs, vs)
    fulls = _full(jb, s)
    seen = set()
    for target in TARGETS:
        for mode in (PAD, COVER):
            for anchor in ANCHORS:
                seen.add((mode,) + fit_ref.geometry((0, 0, w, h), target, mode, anchor)[1 if mode == PAD else 0])
                for filt in (AREA, BILINEAR, BICUBIC):
                    for fmt in range(4):
                        _check(jb, s, ctx, fulls, target, mode, anchor, filt, fmt, fr.IMAGENET if fmt >= 2 else NO_PARAMS)
    assert len(seen) >= 12      # (the anchors and targets really give different rectangles)


def test_every_parameter_set_converts_the_fill_as_the_store_stage(jb, ctx):
    """f32 and f16 under the three parameter sets: unit has inexact products, f16_ties fills that lie halfway between two
    binary16 values (fill 8: 8 * (1 + 2^-11))."""
    s = _frame(jb, 37, 23, 2, 2)
    fulls = _full(jb, s)
    for name, params in fr.PARAM_SETS.items():
        for fmt in (2, 3):
            for fill in ((8, 255, 0), FILL):
                _check(jb, s, ctx, fulls, (16, 16), PAD, fit_ref.CENTER, BILINEAR, fmt, params, fill=fill)


def test_no_border_when_the_aspect_is_the_targets(jb, ctx):
    """37 x 23 to 74 x 46: both modes are the stretch, bit for bit, and nothing is filled."""
    s = _frame(jb, 37, 23, 2, 2)
    fulls = _full(jb, s)
    for filt in (AREA, BICUBIC):
        stretch = area_resize(fulls[0], 74, 46) if filt == AREA else pr.resize(fulls[0], None, (74, 46), filt)
        for mode in (PAD, COVER):
            assert np.array_equal(fit_ref.fit_u8(fulls[0], None, (74, 46), mode, fit_ref.CENTER, FILL, filt), stretch)
            _check(jb, s, ctx, fulls, (74, 46), mode, fit_ref.CENTER, filt, 0)


# ---- 2. a rectangle as the source -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi", [(3, 2, 30, 17), (20, 1, 9, 22)])
def test_a_rectangle_is_the_source(jb, ctx, roi):
    s = _frame(jb, 37, 23, 2, 2)
    fulls = _full(jb, s)
    for mode in (PAD, COVER):
        for filt, fmt in ((AREA, 0), (BILINEAR, 3), (BICUBIC, 1)):
            for anchor in (fit_ref.CENTER, fit_ref.END):
                _check(jb, s, ctx, fulls, (16, 16), mode, anchor, filt, fmt, fr.IMAGENET if fmt >= 2 else NO_PARAMS, roi=roi)


# ---- 3. sub-batches ---------------------------------------------------------------------------------------------------------
def test_forced_sub_batches_give_the_same_buffer(jb, ctx, monkeypatch):
    """A scratch cap of 3,000 bytes holds one 37 x 23 intermediate (2,553 bytes; the filters' windows are no smaller) and not
    two, so the seam's `cap / tmp_image_bytes` is 1 and the three images go through three pixel and resample launches, with
    dst moved to each image's inner rectangle; the one fill launch of the call covers all three.  Every byte of the buffer
    is what the single sub-batch of the default cap gave, and what fit_ref says."""
    s = _frame(jb, 37, 23, 2, 2)
    fulls = _full(jb, s)
    first = {(mode, filt): _check(jb, s, ctx, fulls, (16, 13), mode, fit_ref.CENTER, filt, 3, fr.IMAGENET)[0]
             for mode in (PAD, COVER) for filt in (AREA, BICUBIC)}
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", "3000")     # one 37 x 23 image is 2,553 bytes
    with jb.Context(0) as small:                                 # (the knob is read when a context is created)
        for (mode, filt), host in first.items():
            assert np.array_equal(_check(jb, s, small, fulls, (16, 13), mode, fit_ref.CENTER, filt, 3, fr.IMAGENET)[0], host)


# ---- 4. orientation and arithmetic ------------------------------------------------------------------------------------------
def test_orientation_decides_the_aspect(jb):
    """o = 6 turns the 37 x 23 frame into 23 x 37: the bands of a 16 x 16 letterbox lie left and right, not above and below."""
    s = _frame(jb, 37, 23, 2, 2)
    fulls = [ot.orient(f, 6) for f in _full(jb, s)]
    assert fit_ref.geometry((0, 0, 23, 37), (16, 16), PAD)[1] == (3, 0, 10, 16)
    with jb.Context(0, orientation=6) as turned:
        for mode in (PAD, COVER):
            for filt, fmt in ((AREA, 0), (BICUBIC, 3)):
                _check(jb, s, turned, fulls, (16, 16), mode, fit_ref.CENTER, filt, fmt, fr.IMAGENET if fmt >= 2 else NO_PARAMS)
        _check(jb, s, turned, fulls, (15, 16), PAD, fit_ref.END, BILINEAR, 1, roi=(2, 3, 20, 30))


def _kat_seam(jb, name):
    _, jpeg, rgb = KAT[NAMES.index(name)]
    desc, q, coef = jb.entropy_decode(jpeg)
    s = FitSeam(jb, desc.width, desc.height, desc.hs, desc.vs, [np.ascontiguousarray(coef.reshape(-1, 64))], [q], qtab_id=tuple(desc.qtab_id))
    s.key = ("kat", name)
    return s, rgb


def test_libjpeg_arithmetic_on_a_kat_file_gives_pillows_bits(jb):
    s, rgb = _kat_seam(jb, "420_70x40_restart")
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as lj:
        for mode in (PAD, COVER):
            for filt, fmt in ((BILINEAR, 0), (BICUBIC, 3), (AREA, 2)):
                _check(jb, s, lj, [rgb], (16, 16), mode, fit_ref.CENTER, filt, fmt, fr.IMAGENET if fmt >= 2 else NO_PARAMS)


def test_libjpeg_arithmetic_equals_live_pillow_pad(jb):
    Image = pytest.importorskip("PIL.Image")
    import io
    from PIL import ImageOps
    _, jpeg, _ = KAT[NAMES.index("420_70x40_restart")]
    im = Image.open(io.BytesIO(jpeg)).convert("RGB")
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as lj:
        for method, filt in ((Image.BILINEAR, BILINEAR), (Image.BICUBIC, BICUBIC)):
            for anchor, centering in ((fit_ref.CENTER, (0.5, 0.5)), (fit_ref.START, (0, 0)), (fit_ref.END, (1, 1))):
                want = np.asarray(ImageOps.pad(im, (16, 13), method, color=FILL, centering=centering))
                assert np.array_equal(lj.decode_memory(jpeg, resize=(16, 13), filter=filt, fit=jb.Fit.pad(FILL, anchor)), want), (filt, anchor)


# ---- 5. files ---------------------------------------------------------------------------------------------------------------
FILES = ["420_70x40_restart", "420_3x5", "420_45x35_progressive", "444_521x19", "gray_33x21"]


def _write(tmp_path, names):
    paths = []
    for n in names:
        p = tmp_path / (n + ".jpg")
        p.write_bytes(KAT[NAMES.index(n)][1])
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("huff", ["2", "0"])
def test_decode_memory_and_file(jb, monkeypatch, tmp_path, huff):
    """The entropy stage on the device and on the host; *width and *height are the target's."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    paths = _write(tmp_path, FILES[:3])
    with jb.Context(0) as c:
        for name, path in zip(FILES[:3], paths):
            jpeg = KAT[NAMES.index(name)][1]
            full = c.decode_memory(jpeg)
            for mode, fit in ((PAD, jb.Fit.pad(FILL, jb.FIT_END)), (COVER, jb.Fit.cover(jb.FIT_START))):
                anchor = fit.anchor
                got = c.decode_memory(jpeg, resize=(16, 13), filter=BICUBIC, fit=fit)
                assert got.shape == (13, 16, 3) and np.array_equal(got, fit_ref.fit_u8(full, None, (16, 13), mode, anchor, FILL, BICUBIC)), (name, mode)
                got = c.decode_file(path, fmt=spec, resize=(15, 16), fit=fit, roi=None)
                assert fr.same_bits(got, fit_ref.fit(full, None, (15, 16), mode, anchor, FILL, AREA, 3, *sb)), (name, mode)
            assert np.array_equal(c.decode_memory(jpeg, resize=(16, 13), fit=jb.FIT_STRETCH), area_resize(full, 16, 13)), name


def test_batch_decoder_files_of_two_aspects_imagenet_f16(jb, tmp_path):
    """Files whose bands lie on different axes (70 x 40 and 521 x 19 above and below, 3 x 5 left and right) to
    ImageNet-normalised f16 with a grey border, through run, run_to_tensor and submit / collect; then set_fit(None) gives
    the stretch bits back."""
    import torch
    paths = _write(tmp_path, FILES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.Context(0) as c:
        fulls = [c.decode_memory(KAT[NAMES.index(n)][1]) for n in FILES]
    target = (16, 16)
    axes = {fit_ref.geometry((0, 0, f.shape[1], f.shape[0]), target, PAD)[1][2] < 16 for f in fulls}
    assert axes == {True, False}
    with jb.BatchDecoder(4, 0, fmt=spec, resize=target, filter=BILINEAR, fit=jb.Fit.pad(FILL)) as dec:
        wants = [fit_ref.fit(f, None, target, PAD, fit_ref.CENTER, FILL, BILINEAR, 3, *sb) for f in fulls]
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, want in enumerate(wants):
            assert fr.same_bits(imgs[i], want), FILES[i]
        out = torch.full((len(paths), 3, 16, 16), 7.0, dtype=torch.float16, device="cuda:0")
        out, st, tm = dec.run_to_tensor(paths, out)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        host = out.cpu().numpy()
        for i, want in enumerate(wants):
            assert fr.same_bits(host[i], want), FILES[i]
        # both sides of submit / collect have the fit: the letterbox first, its fill through the twin side too
        t, t2 = dec.submit(paths), dec.submit(paths)
        for ticket in (t, t2):
            imgs, st, tm = dec.collect(ticket)
            assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
            for i, want in enumerate(wants):
                assert fr.same_bits(imgs[i], want), FILES[i]
        dec.set_fit(jb.Fit.cover(jb.FIT_END))
        t, t2 = dec.submit(paths), dec.submit(paths)
        with pytest.raises(jb.JbError) as e:
            dec.set_fit(None)
        assert e.value.status == -7
        for ticket in (t, t2):
            imgs, st, tm = dec.collect(ticket)
            assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
            for i, f in enumerate(fulls):
                assert fr.same_bits(imgs[i], fit_ref.fit(f, None, target, COVER, fit_ref.END, FILL, BILINEAR, 3, *sb)), FILES[i]
        # stretch again
        dec.set_fit(None)
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, f in enumerate(fulls):
            assert fr.same_bits(imgs[i], pr.resize_to_format(f, None, target, BILINEAR, 3, *sb)), FILES[i]


# ---- 6. refusals and state ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(jb, ctx):
    s = _frame(jb, 37, 23, 2, 2)
    s.catch = True
    try:
        for kw, status in ((dict(crops=[(0, 0, 9, 9)] * 3), -9), (dict(views=[[(0, 0, 9, 9)]] * 3), -9)):
            for fit in (jb.Fit.pad(FILL), jb.Fit.cover()):
                s.fit, s.crops, s.views = fit, kw.get("crops"), kw.get("views")
                host, _ = s.run(ctx, 0, (16, 16), resize=(16, 16))
                assert s.error is not None and s.error.status == status, (kw, s.error)
                assert (host == SENT).all()
        s.crops = s.views = None
        # what only C sees: a mode that is none, an anchor that is none, a reserved field
        bad = jb.Fit.pad(FILL)
        bad.reserved8 = 1
        for fit in (jb.Fit(3, 0), jb.Fit(1, 5), bad):
            s.fit = fit
            host, _ = s.run(ctx, 0, (16, 16), resize=(16, 16))
            assert s.error is not None and s.error.status == -2, s.error
            assert (host == SENT).all()
    finally:
        s.catch, s.fit, s.filter, s.crops, s.views = False, None, 0, None, None


def test_the_tap_cap_is_that_of_the_pair_that_is_resampled(jb, ctx):
    """1033 x 11 to 8 x 8, bicubic: stretched and letterboxed the rows reduce 129-fold, more than the kernel's taps hold
    (JB_ERR_UNSUPPORTED, nothing written); the centred 11 x 11 square does not."""
    s, _ = _kat_seam(jb, "422_1033x11")
    full = _full(jb, s)
    s.catch, s.filter = True, BICUBIC
    try:
        for fit in (None, jb.Fit.pad(FILL)):
            s.fit = fit
            host, _ = s.run(ctx, 0, (8, 8), resize=(8, 8))
            assert s.error is not None and s.error.status == -9, (fit, s.error)
            assert (host == SENT).all()
    finally:
        s.catch, s.fit, s.filter = False, None, 0
    for fmt in (0, 3):
        _check(jb, s, ctx, full, (8, 8), COVER, fit_ref.CENTER, BICUBIC, fmt, fr.IMAGENET if fmt >= 2 else NO_PARAMS)


def test_batch_decoder_refuses_crops_and_views_while_a_mode_is_set(jb, tmp_path):
    paths = _write(tmp_path, FILES[:2])
    with jb.BatchDecoder(2, 0, resize=(16, 16), fit=jb.FIT_PAD) as dec:
        assert dec.run(paths, crops=[(0, 0, 2, 2)] * 2)[2]["rc"] == -9
        assert dec.run(paths, views=[[(0, 0, 2, 2)]] * 2)[2]["rc"] == -9
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, crops=[(0, 0, 2, 2)] * 2)
        assert e.value.status == -9
        for bad in (3, jb.Fit(1, 7)):
            with pytest.raises(jb.JbError) as e:
                dec.set_fit(bad)
            assert e.value.status == -2
        # the fit is kept while no target size is set: every file then answers JB_ERR_STATE
        dec.set_resize(None)
        imgs, st, tm = dec.run(paths)
        assert st == [-7, -7] and imgs == [None, None]
        dec.set_fit(jb.FIT_STRETCH)
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0, 0] and imgs[0].shape == (40, 70, 3)
        dec.set_resize((16, 16))
        imgs, st, tm = dec.run(paths, crops=[(0, 0, 2, 2)] * 2)
        assert tm["rc"] == 0 and st == [0, 0]


def test_set_fit_none_gives_the_stretch_bits_back(jb, ctx):
    """The seam: fit=None, FIT_STRETCH and a context that has just run a letterbox all give the stretch's buffer."""
    s = _frame(jb, 23, 37, 1, 1)
    fulls = _full(jb, s)
    s.pads, s.filter = (3, 5, 7), BICUBIC
    try:
        wants = [pr.resize_to_format(f, None, (16, 13), BICUBIC, 3, *fr.IMAGENET) for f in fulls]
        before = s.check(ctx, wants, 3, fr.IMAGENET, resize=(16, 13))[0]
        s.fit = jb.Fit.pad(FILL)
        s.check(ctx, [fit_ref.fit(f, None, (16, 13), PAD, 0, FILL, BICUBIC, 3, *fr.IMAGENET) for f in fulls], 3, fr.IMAGENET, resize=(16, 13))
        for fit in (None, jb.FIT_STRETCH, jb.Fit(0, 0)):
            s.fit = fit
            assert np.array_equal(s.check(ctx, wants, 3, fr.IMAGENET, resize=(16, 13))[0], before)
    finally:
        s.pads, s.filter, s.fit = (0, 0, 0), 0, None
