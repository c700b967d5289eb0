"""Decoder arithmetic JB_ARITH_LIBJPEG on the GPU (-m gpu): a context with ARITH_LIBJPEG decodes, bit for bit, what
libjpeg does -- Pillow's bits from tests/golden/libjpeg_decode_kat.npz where a file exists, tests/libjpeg_ref.py (held
against Pillow in test_libjpeg_cpu.py) for synthetic coefficients: never something the code under test computed -- and
every output option composes on top of that image unchanged.  At the seam the whole sentinel-filled buffer is compared,
odd lead and pads included."""
import os

import numpy as np
import pytest

import format_ref as fr
import libjpeg_ref
import pillow_resize_ref as pr
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, Seam, _oracle_full

pytestmark = pytest.mark.gpu

KAT = libjpeg_ref.load_kat()
BILINEAR, BICUBIC = pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
NAMES = [n for n, _, _ in KAT]
BIG = "420_521x37_noise_q95"
RECTS = [(16, 16, 16, 16),    # every edge on an MCU edge: all eight neighbouring MCUs' chroma, none of them launched for pixels
         (17, 15, 31, 7),
         (505, 30, 16, 7)]    # the frame's corner: the clamps


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def ctx(jb):
    c = jb.Context(0, arithmetic=jb.ARITH_LIBJPEG)
    assert c.arithmetic == jb.ARITH_LIBJPEG
    yield c
    c.close()


class LjSeam(Seam):
    """Seam whose launches also carry crops= and filter= (self.crops, self.filter); catch: a refusal is kept in .error."""
    crops = None
    filter = 0
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        seam = self

        class Through:
            def blocks_to_rgb_device(self, batch, **kw):
                try:
                    ctx.blocks_to_rgb_device(batch, crops=seam.crops, filter=seam.filter, **kw)
                except seam.jb.JbError as e:
                    if not seam.catch:
                        raise
                    seam.error = e

            def synchronize(self):
                ctx.synchronize()

        self.error = None
        return super().run(Through(), fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)


_cache = {}


def _kat_frame(jb, name):
    """-> (desc, qtabs, coef [n, 64], Pillow's image) of a KAT file, through the host front end; made once"""
    if name not in _cache:
        _, jpeg, rgb = KAT[NAMES.index(name)]
        desc, q, coef = jb.entropy_decode(jpeg)
        _cache[name] = desc, q, np.ascontiguousarray(coef.reshape(-1, 64)), rgb
    return _cache[name]


def _seam_of(jb, desc, coefs, qs, **pads):
    return LjSeam(jb, desc.width, desc.height, desc.hs, desc.vs, coefs, qs, qtab_id=tuple(desc.qtab_id), **pads)


def _synth_frame(jb, w, h, hs, vs, dense=False, index=0, n=1):
    """-> (LjSeam over n synthetic images, libjpeg_ref's images); made once and not changed"""
    from jpeg_decoder_amd import synth
    key = (w, h, hs, vs, dense, index, n)
    if key not in _cache:
        coefs, qs = zip(*[synth.synth_blocks(w, h, hs, vs, image_index=index + 11 * i, dense=dense) for i in range(n)])
        d = jb.make_desc(w, h, hs, vs)
        fulls = [libjpeg_ref.decode_blocks(d, q, c) for c, q in zip(coefs, qs)]
        _cache[key] = LjSeam(jb, w, h, hs, vs, list(coefs), list(qs), pad_row=3, pad_plane=5, pad_img=7), fulls
    return _cache[key]


def _big(jb, n=1):
    """the 521 x 37 4:2:0 KAT frame as image 0 of a seam of n images (the others synthetic, with tables of their own)
    -> (seam, full images)"""
    from jpeg_decoder_amd import synth
    key = ("big", n)
    if key not in _cache:
        desc, q, coef, rgb = _kat_frame(jb, BIG)
        assert (desc.hs, desc.vs) == (2, 2)
        coefs, qs, fulls = [coef], [q], [rgb]
        for i in range(1, n):
            c, qq = synth.synth_blocks(desc.width, desc.height, 2, 2, image_index=90 + i, qtabs=synth.annex_k_qtabs(60 + 10 * i))
            q4 = np.zeros_like(q)
            for comp in range(3):   # the tables where this file's descriptor looks for them
                q4[desc.qtab_id[comp]] = qq[(0, 1, 1)[comp]]
            coefs.append(c), qs.append(q4), fulls.append(libjpeg_ref.decode_blocks(desc, q4, c))
        _cache[key] = _seam_of(jb, desc, coefs, qs, pad_row=3, pad_plane=5, pad_img=7), fulls
    return _cache[key]


# ---- 1. the KAT's coefficients through the seam ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kat_coefficients_give_pillows_bits(jb, ctx, name):
    desc, q, coef, rgb = _kat_frame(jb, name)
    _seam_of(jb, desc, [coef], [q], pad_row=3, pad_img=7).check(ctx, [rgb], 0, tag=name)
    _seam_of(jb, desc, [coef], [q]).check(ctx, [rgb], 0, tag=(name, "tight"))


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_kat_every_format_every_parameter_set(jb, ctx, fmt):
    s, fulls = _big(jb)
    for name, (scale, bias) in list(fr.PARAM_SETS.items())[:3 if fmt >= 2 else 1]:
        s.check(ctx, [fr.to_format(fulls[0], fmt, scale, bias)], fmt, (scale, bias), tag=name)


def test_kat_batch_of_two_with_tables_per_image(jb, ctx):
    s, fulls = _big(jb, n=2)
    assert not np.array_equal(fulls[0], fulls[1])
    s.check(ctx, fulls, 0)
    s.check(ctx, [fr.to_format(f, 3, *fr.IMAGENET) for f in fulls], 3, fr.IMAGENET)


# ---- 2. synthetic coefficients, every layout ---------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_synthetic_blocks_every_layout(jb, ctx, hs, vs, dense):
    for w, h in ((8 * 64 + 5, 16 * 3 + 3), (7, 13)):
        s, fulls = _synth_frame(jb, w, h, hs, vs, dense, index=w + hs + 2 * vs)
        s.check(ctx, fulls, 0, tag=(hs, vs, dense, w, h))


# ---- 3. a rectangle is a crop of the full decode ---------------------------------------------------------------------
@pytest.mark.parametrize("hs,vs", [(2, 2), (2, 1), (1, 2)])
def test_roi_is_the_crop_of_the_full_image(jb, ctx, hs, vs):
    s, fulls = _big(jb) if (hs, vs) == (2, 2) else _synth_frame(jb, 521, 37, hs, vs, index=5)
    for k, (x, y, w, h) in enumerate(RECTS):
        for fmt in (0, 1 + k):
            sb = fr.IMAGENET if fmt >= 2 else NO_PARAMS
            s.check(ctx, [fr.to_format(fulls[0][y:y + h, x:x + w], fmt, *sb)], fmt, sb, roi=(x, y, w, h), tag=(hs, vs))


# ---- 4. composition ----------------------------------------------------------------------------------------------------
def test_resize_is_the_area_resize_of_the_full_image(jb, ctx):
    s, fulls = _big(jb)
    s.check(ctx, [area_resize(fulls[0], 20, 9)], 0, resize=(20, 9))
    x, y, w, h = RECTS[1]
    s.check(ctx, [fr.to_format(area_resize(fulls[0][y:y + h, x:x + w], 9, 4), 3, *fr.IMAGENET)], 3, fr.IMAGENET, roi=RECTS[1], resize=(9, 4))


@pytest.mark.parametrize("filt", [BILINEAR, BICUBIC])
def test_filters_are_pillows_resize_of_the_full_image(jb, ctx, filt):
    s, fulls = _big(jb)
    s.filter = filt
    try:
        for k, (rect, target) in enumerate(((RECTS[0], (24, 24)), ((100, 3, 300, 30), (56, 11)), (RECTS[2], (5, 9)), (None, (64, 8)))):
            for fmt in (0, 3):
                sb = fr.IMAGENET if fmt else NO_PARAMS
                s.check(ctx, [pr.resize_to_format(fulls[0], rect, target, filt, fmt, *sb)], fmt, sb, roi=rect, resize=target, tag=(filt, rect))
    finally:
        s.filter = 0


@pytest.mark.parametrize("filt", [0, BILINEAR, BICUBIC])
def test_crops_three_rectangles_over_a_batch_of_three(jb, ctx, filt):
    s, fulls = _big(jb, n=3)
    target = (12, 10)
    if filt == 0:
        wants = [fr.to_format(area_resize(f[y:y + h, x:x + w], *target), 3, *fr.IMAGENET) for f, (x, y, w, h) in zip(fulls, RECTS)]
    else:
        wants = [pr.resize_to_format(f, r, target, filt, 3, *fr.IMAGENET) for f, r in zip(fulls, RECTS)]
    s.crops, s.filter = RECTS, filt
    try:
        s.check(ctx, wants, 3, fr.IMAGENET, resize=target, tag=filt)
    finally:
        s.crops, s.filter = None, 0


def test_sub_batches_of_planes_give_the_same_buffer(jb, ctx, monkeypatch):
    """A scratch cap below two images' planes: three whole images run one by one; per-image rectangles on that context."""
    s, fulls = _big(jb, n=3)
    first = s.check(ctx, fulls, 0)[0]
    wants = [fr.to_format(area_resize(f[y:y + h, x:x + w], 12, 10), 3, *fr.IMAGENET) for f, (x, y, w, h) in zip(fulls, RECTS)]
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", "40000")    # one 521 x 37 4:2:0 image's planes are 38,016 bytes
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as small:  # (the knob is read when a context is created)
        assert np.array_equal(s.check(small, fulls, 0)[0], first)
        s.crops = RECTS
        try:
            s.check(small, wants, 3, fr.IMAGENET, resize=(12, 10))
        finally:
            s.crops = None


# ---- 5. files -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("huff", ["2", "0"])
def test_decode_memory_and_file_give_pillows_bits(jb, monkeypatch, tmp_path, huff):
    """Baseline, grayscale, progressive and restart-interval files; the entropy stage on the device and on the host."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as c:
        for name, jpeg, rgb in KAT:
            assert np.array_equal(c.decode_memory(jpeg), rgb), name
            path = tmp_path / (name + ".jpg")
            path.write_bytes(jpeg)
            assert np.array_equal(c.decode_file(str(path)), rgb), name


FILE_CASES = [(BIG, (101, 5, 300, 30), (56, 11)), ("444_521x19", (3, 2, 500, 16), (224, 7)), ("gray_33x21", None, (8, 8)),
              ("420_45x35_progressive", (16, 16, 16, 16), (24, 24))]


def test_decode_memory_filtered_is_pillows_resize_of_pillows_image(jb, ctx):
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    for name, roi, target in FILE_CASES:
        _, jpeg, rgb = KAT[NAMES.index(name)]
        assert np.array_equal(ctx.decode_memory(jpeg, roi=roi, resize=target, filter=BICUBIC), pr.resize(rgb, roi, target, BICUBIC)), name
        want = pr.resize_to_format(rgb, roi, target, BICUBIC, 3, list(spec.scale), list(spec.bias))
        assert fr.same_bits(ctx.decode_memory(jpeg, fmt=spec, roi=roi, resize=target, filter=BICUBIC), want), name


def test_decode_memory_filtered_equals_live_pillow(jb, ctx):
    Image = pytest.importorskip("PIL.Image")
    import io
    for name, roi, target in FILE_CASES:
        _, jpeg, _ = KAT[NAMES.index(name)]
        im = Image.open(io.BytesIO(jpeg)).convert("RGB")
        x, y, w, h = roi if roi is not None else (0, 0) + im.size
        want = np.asarray(im.resize(target, Image.BICUBIC, box=(x, y, x + w, y + h)))
        assert np.array_equal(ctx.decode_memory(jpeg, roi=roi, resize=target, filter=BICUBIC), want), name


MIXED = [BIG, "444_521x19", "422_1033x11", "440_515x37_synth", "420_3x5", "gray_33x21", "420_45x35_progressive", "420_70x40_restart", "422_5x3"]


def _write(tmp_path, names):
    paths = []
    for n in names:
        p = tmp_path / (n + ".jpg")
        p.write_bytes(KAT[NAMES.index(n)][1])
        paths.append(str(p))
    return paths, [KAT[NAMES.index(n)][2] for n in names]


def test_batch_decoder_mixed_files_resized_imagenet_f16(jb, tmp_path):
    paths, rgbs = _write(tmp_path, MIXED)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.BatchDecoder(4, 0, fmt=spec, resize=(32, 8), arithmetic=jb.ARITH_LIBJPEG) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, rgb in enumerate(rgbs):
            assert fr.same_bits(imgs[i], fr.to_format(area_resize(rgb, 32, 8), 3, *sb)), MIXED[i]
        dec.set_filter(BICUBIC)
        t = dec.submit(paths)         # the twin side has the arithmetic too
        t2 = dec.submit(paths)
        with pytest.raises(jb.JbError) as e:
            dec.set_arithmetic(jb.ARITH_REFERENCE)
        assert e.value.status == -7
        for ticket in (t, t2):
            imgs, st, tm = dec.collect(ticket)
            assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
            for i, rgb in enumerate(rgbs):
                assert fr.same_bits(imgs[i], pr.resize_to_format(rgb, None, (32, 8), BICUBIC, 3, *sb)), MIXED[i]


def test_batch_decoder_full_size_files(jb, tmp_path):
    paths, rgbs = _write(tmp_path, MIXED)
    with jb.BatchDecoder(2, 0, arithmetic=jb.ARITH_LIBJPEG) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, rgb in enumerate(rgbs):
            assert np.array_equal(imgs[i], rgb), MIXED[i]


def test_run_to_tensor_with_crops(jb, tmp_path):
    import torch
    names = [BIG, "440_515x37_synth", "420_70x40_restart"]
    crops = [RECTS[0], (490, 20, 25, 17), (3, 5, 60, 30)]
    paths, rgbs = _write(tmp_path, names)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.BatchDecoder(2, 0, fmt=spec, resize=(14, 9), filter=BILINEAR, arithmetic=jb.ARITH_LIBJPEG) as dec:
        out = torch.zeros((3, 3, 9, 14), dtype=torch.float16, device="cuda:0")
        out, st, tm = dec.run_to_tensor(paths, out, crops=crops)
        assert tm["rc"] == 0 and st == [0, 0, 0], (tm, st)
        host = out.cpu().numpy()
        for i in range(3):
            assert fr.same_bits(host[i], pr.resize_to_format(rgbs[i], crops[i], (14, 9), BILINEAR, 3, *sb)), names[i]


# ---- 6. refusals and state ---------------------------------------------------------------------------------------------
def test_scale_is_refused_and_nothing_is_written(jb, ctx):
    s, _ = _big(jb)
    s.catch = True
    try:
        host, _ = s.run(ctx, 0, jb.scaled_size(521, 37, 2), scale=2)
        assert s.error is not None and s.error.status == -9, s.error
        assert (host == SENT).all()
    finally:
        s.catch = False
    _, jpeg, _ = KAT[NAMES.index(BIG)]
    with pytest.raises(jb.JbError) as e:
        ctx.decode_memory(jpeg, scale=2)
    assert e.value.status == -9
    with pytest.raises(jb.JbError) as e:
        ctx.set_arithmetic(7)
    assert e.value.status == -2 and ctx.arithmetic == jb.ARITH_LIBJPEG


def test_the_switch_goes_both_ways(jb, oracle):
    """One context: the oracle's bits by default, libjpeg's after the setter, the oracle's again after setting back."""
    desc, q, coef, rgb = _kat_frame(jb, BIG)
    ref = _oracle_full(oracle, desc.width, desc.height, 2, 2, coef, q, tuple(desc.qtab_id))
    assert not np.array_equal(ref, rgb)
    s = _seam_of(jb, desc, [coef], [q], pad_row=3)
    with jb.Context.for_image(desc) as c:
        assert c.arithmetic == jb.ARITH_REFERENCE
        s.check(c, [ref], 0)
        c.set_arithmetic(jb.ARITH_LIBJPEG)
        s.check(c, [rgb], 0)
        assert np.array_equal(c.blocks_to_rgb(desc, coef, q), rgb)    # the host-buffer seam too
        c.set_arithmetic(jb.ARITH_REFERENCE)
        s.check(c, [ref], 0)
        assert np.array_equal(c.blocks_to_rgb(desc, coef, q), ref)


def test_decoder_scale_and_arithmetic_refuse_each_other(jb):
    with jb.BatchDecoder(1, 0, arithmetic=jb.ARITH_LIBJPEG) as dec:
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(2)
        assert e.value.status == -9
        dec.set_scale(1)
        with pytest.raises(jb.JbError) as e:
            dec.set_arithmetic(7)
        assert e.value.status == -2
    with jb.BatchDecoder(1, 0, scale=2) as dec:
        with pytest.raises(jb.JbError) as e:
            dec.set_arithmetic(jb.ARITH_LIBJPEG)
        assert e.value.status == -9
        dec.set_arithmetic(jb.ARITH_REFERENCE)
    with pytest.raises(jb.JbError) as e:
        jb.BatchDecoder(1, 0, scale=2, arithmetic=jb.ARITH_LIBJPEG)
    assert e.value.status == -9
