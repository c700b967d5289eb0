"""Draft decode on the GPU (-m gpu): a context with ARITH_LIBJPEG and draft K decodes, bit for bit, what libjpeg gives at
scale 1 / K -- Pillow's bits from tests/golden/libjpeg_draft_kat.npz where a file exists, tests/draft_ref.py (held
against Pillow in test_draft_cpu.py) for synthetic coefficients: never something the code under test computed -- and
every output option acts on that draft image as on a full-size decode of its size.  At the seam the whole
sentinel-filled buffer is compared, odd lead and pads included."""
import numpy as np
import pytest

import draft_ref
import fit_ref
import format_ref as fr
import libjpeg_ref
import pillow_resize_ref as pr
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, Seam

pytestmark = pytest.mark.gpu

KAT = draft_ref.load_kat()
NAMES = [n for n, _, _ in KAT]
FULL = {n: rgb for n, _, rgb in libjpeg_ref.load_kat()}
DENOMS = draft_ref.DENOMS
AREA, BILINEAR, BICUBIC = 0, pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
BIG = "420_521x37_noise_q95"          # 261 x 19 at draft 2: across the pixel kernel's 256-pixel tile
WIDE = "422_1033x11"                  # 517 and 259 columns at draft 2 and 4
BY_LAYOUT = {(1, 1): "draft_444_131x70", (2, 2): "draft_420_131x70", (2, 1): "draft_422_131x70", (1, 2): "draft_440_131x70_synth"}


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def ctxs(jb):
    """one context per draft, 1 included"""
    cs = {K: jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, draft=K) for K in (1,) + DENOMS}
    for K, c in cs.items():
        assert c.draft == K and c.arithmetic == jb.ARITH_LIBJPEG
    yield cs
    for c in cs.values():
        c.close()


class DraftSeam(Seam):
    """Seam whose launches also carry crops=, filter=, views= and fit= (attributes); with views the buffer holds
    k outputs per image.  catch: a refusal is kept in .error."""
    crops = None
    filter = 0
    views = None
    fit = None
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        seam, images = self, self.n

        class Through:
            def blocks_to_rgb_device(self, batch, **kw):
                batch.n_images = images
                try:
                    ctx.blocks_to_rgb_device(batch, crops=seam.crops, filter=seam.filter, views=seam.views, fit=seam.fit, **kw)
                except seam.jb.JbError as e:
                    if not seam.catch:
                        raise
                    seam.error = e

            def synchronize(self):
                ctx.synchronize()

        self.error = None
        if self.views is not None:
            self.n = images * len(self.views[0])   # (the harness lays out one "image" per output)
        try:
            return super().run(Through(), fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)
        finally:
            self.n = images

    def having(self, **attrs):
        """a context manager: the attributes for the launches inside it"""
        seam = self

        class Having:
            def __enter__(self):
                for k, v in attrs.items():
                    setattr(seam, k, v)

            def __exit__(self, *a):
                for k in attrs:
                    setattr(seam, k, getattr(DraftSeam, k))

        return Having()


_cache = {}


def _kat_frame(jb, name):
    """-> (desc, qtabs, coef [n, 64], {K: Pillow's draft image}) of a KAT file, through the host front end; made once"""
    if name not in _cache:
        _, jpeg, drafts = KAT[NAMES.index(name)]
        desc, q, coef = jb.entropy_decode(jpeg)
        _cache[name] = desc, q, np.ascontiguousarray(coef.reshape(-1, 64)), drafts
    return _cache[name]


def _ring_context(jb, desc, images=1, **settings):
    """a context whose staging ring holds `images` full-size images of desc (the host-buffer seam needs one)"""
    g = jb.geometry_of(desc)
    return jb.Context(0, images * g.coef_bytes, images * g.rgb_bytes, **settings)


def _seam_of(jb, desc, coefs, qs, **pads):
    return DraftSeam(jb, desc.width, desc.height, desc.hs, desc.vs, coefs, qs, qtab_id=tuple(desc.qtab_id), **pads)


def _three(jb, name):
    """the KAT frame `name` as image 0 of a seam of three (the others synthetic, with tables of their own), padded strides
    -> (seam, {K: [three draft images]})"""
    from jpeg_decoder_amd import synth
    key = ("three", name)
    if key not in _cache:
        desc, q, coef, drafts = _kat_frame(jb, name)
        coefs, qs = [coef], [q]
        for i in (1, 2):
            c, qq = synth.synth_blocks(desc.width, desc.height, desc.hs, desc.vs, image_index=90 + i, qtabs=synth.annex_k_qtabs(60 + 10 * i))
            q4 = np.zeros_like(q)
            for comp in range(3):   # the tables where this file's descriptor looks for them
                q4[desc.qtab_id[comp]] = qq[(0, 1, 1)[comp]]
            coefs.append(c), qs.append(q4)
        images = {K: [drafts[K]] + [draft_ref.decode_blocks(desc, qs[i], coefs[i], K) for i in (1, 2)] for K in DENOMS}
        _cache[key] = _seam_of(jb, desc, coefs, qs, pad_row=3, pad_plane=5, pad_img=7), images
    return _cache[key]


def _layout(jb, hs, vs):
    """the 131 x 70 KAT file of a layout -> (seam of one image, padded strides; {K: Pillow's draft image})"""
    key = ("layout", hs, vs)
    if key not in _cache:
        desc, q, coef, drafts = _kat_frame(jb, BY_LAYOUT[hs, vs])
        assert (desc.hs, desc.vs) == (hs, vs)
        _cache[key] = _seam_of(jb, desc, [coef], [q], pad_row=3, pad_plane=5, pad_img=7), drafts
    return _cache[key]


# ---- 1. every KAT file's coefficients through the seam, at every draft ---------------------------------------------------
@pytest.mark.parametrize("K", DENOMS)
def test_kat_coefficients_give_pillows_draft_bits(jb, ctxs, K):
    for name in NAMES:     # 1x1, 2x1, 17x1, the draft-8 replication of 4:2:2 and 4:4:0, 261 and 517 / 259 columns among them
        desc, q, coef, drafts = _kat_frame(jb, name)
        assert drafts[K].shape == (-(-desc.height // K), -(-desc.width // K), 3)
        _seam_of(jb, desc, [coef], [q], pad_row=3, pad_img=7).check(ctxs[K], [drafts[K]], 0, tag=(name, K))
        _seam_of(jb, desc, [coef], [q]).check(ctxs[K], [drafts[K]], 0, tag=(name, K, "tight"))


def test_the_named_shapes_are_among_the_cases():
    shape = lambda name, K: dict((n, d) for n, _, d in KAT)[name][K].shape[:2][::-1]
    assert shape(BIG, 2) == (261, 19) and shape(WIDE, 2) == (517, 6) and shape(WIDE, 4) == (259, 3)
    for name in ("420_1x1", "420_2x1", "420_17x1", "440_515x37_synth"):
        assert name in NAMES


@pytest.mark.parametrize("K", DENOMS)
@pytest.mark.parametrize("name", [BIG, WIDE])
def test_batch_of_three_with_tables_per_image_and_padded_strides(jb, ctxs, name, K):
    s, images = _three(jb, name)
    assert not np.array_equal(images[K][0], images[K][1])
    s.check(ctxs[K], images[K], 0, tag=(name, K))
    s.check(ctxs[K], [fr.to_format(f, 3, *fr.IMAGENET) for f in images[K]], 3, fr.IMAGENET, tag=(name, K))


# ---- 2. formats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_every_format_on_one_file_per_layout(jb, ctxs, hs, vs, fmt):
    s, drafts = _layout(jb, hs, vs)
    for K in DENOMS:
        sb = list(fr.PARAM_SETS.values())[(K + fmt) % 3] if fmt >= 2 else NO_PARAMS
        s.check(ctxs[K], [fr.to_format(drafts[K], fmt, *sb)], fmt, sb, tag=(hs, vs, K))


# ---- 3. a rectangle is a crop of the draft image -------------------------------------------------------------------------
def _rects(ow, oh, mw, mh):
    """six rectangles of an ow x oh draft frame whose MCUs are mw x mh of its pixels"""
    return [(mw, mh, mw, mh),                             # every edge on an MCU edge: the fancy neighbours lie in MCUs it does not touch
            (2 * mw, mh, 3 * mw, 2 * mh),
            (mw + 1, mh - 1, 2 * mw + 3, mh + 2),         # off the MCU grid
            (ow - 3, oh - 2, 3, 2),                       # the frame's corner: its last, partial MCU and the clamps
            (0, oh - 1, ow, 1),                           # the last row
            (ow // 2, 0, 1, oh)]                          # one column


@pytest.mark.parametrize("K", DENOMS)
@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_roi_is_the_crop_of_the_draft_image(jb, ctxs, hs, vs, K):
    s, drafts = _layout(jb, hs, vs)
    img = drafts[K]
    oh, ow = img.shape[:2]
    rects = _rects(ow, oh, hs * 8 // K, vs * 8 // K)
    assert ow % (hs * 8 // K) != 0 or K == 8     # (131 x 70: the last MCU column is partial at draft 2 and 4)
    for k, (x, y, w, h) in enumerate(rects):
        assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= ow and y + h <= oh
        fmt = k % 4
        sb = fr.IMAGENET if fmt >= 2 else NO_PARAMS
        s.check(ctxs[K], [fr.to_format(np.ascontiguousarray(img[y:y + h, x:x + w]), fmt, *sb)], fmt, sb, roi=(x, y, w, h), tag=(hs, vs, K))


def test_a_rectangle_outside_the_draft_frame_is_refused(jb, ctxs):
    s, drafts = _layout(jb, 2, 2)
    with s.having(catch=True):
        host, _ = s.run(ctxs[2], 0, (8, 8), roi=(60, 30, 8, 8))      # lies in 131 x 70, not in 66 x 35
        assert s.error is not None and s.error.status == -2 and (host == SENT).all()


# ---- 4. composition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", DENOMS)
def test_resize_is_the_resize_of_the_draft_image(jb, ctxs, K):
    s, images = _three(jb, BIG)
    fulls = images[K]
    oh, ow = fulls[0].shape[:2]
    rect = (ow // 4, 1, ow // 2, oh - 2)
    s.check(ctxs[K], [area_resize(f, 20, 3) for f in fulls], 0, resize=(20, 3), tag=K)
    x, y, w, h = rect
    s.check(ctxs[K], [fr.to_format(area_resize(f[y:y + h, x:x + w], 9, 2), 3, *fr.IMAGENET) for f in fulls], 3, fr.IMAGENET, roi=rect, resize=(9, 2), tag=K)
    for filt in (BILINEAR, BICUBIC):
        with s.having(filter=filt):
            for r, target in ((None, (24, 5)), (rect, (7, 9))):
                for fmt in (0, 3):
                    sb = fr.IMAGENET if fmt else NO_PARAMS
                    s.check(ctxs[K], [pr.resize_to_format(f, r, target, filt, fmt, *sb) for f in fulls], fmt, sb, roi=r, resize=target, tag=(K, filt, r))


@pytest.mark.parametrize("K", DENOMS)
@pytest.mark.parametrize("filt", [AREA, BICUBIC])
def test_crops_views_and_fit_act_on_the_draft_image(jb, ctxs, K, filt):
    s, images = _three(jb, BIG)
    fulls = images[K]
    oh, ow = fulls[0].shape[:2]
    target = (12, 4)
    crops = [(0, 0, ow, oh), (ow // 3, 1, ow // 3, oh - 1), (ow - 5, oh - 2, 5, 2)]

    def one(f, r):
        x, y, w, h = r
        return area_resize(f[y:y + h, x:x + w], *target) if filt == AREA else pr.resize(f, r, target, filt)

    with s.having(crops=crops, filter=filt):
        s.check(ctxs[K], [fr.to_format(one(f, r), 3, *fr.IMAGENET) for f, r in zip(fulls, crops)], 3, fr.IMAGENET, resize=target, tag=("crops", K))
    views = [[crops[(i + v) % 3] + (v == 1,) for v in range(2)] for i in range(3)]     # two views per image, the second mirrored
    wants = [np.ascontiguousarray(one(f, v[:4])[:, ::-1] if v[4] else one(f, v[:4])) for f, row in zip(fulls, views) for v in row]
    with s.having(views=views, filter=filt):
        s.check(ctxs[K], wants, 0, resize=target, tag=("views", K))
    fill = (124, 116, 104)
    for fit, mode in ((jb.Fit.pad(fill), fit_ref.PAD), (jb.Fit.cover(), fit_ref.COVER)):
        with s.having(fit=fit, filter=filt):
            s.check(ctxs[K], [fit_ref.fit(f, None, (16, 16), mode, fit_ref.CENTER, fill, filt, 3, *fr.IMAGENET) for f in fulls], 3, fr.IMAGENET,
                    resize=(16, 16), tag=("fit", mode, K))


def test_the_tap_cap_is_that_of_the_draft_frame(jb, ctxs):
    """bicubic 521 -> 8 columns is 65 x: refused at draft 1 (more than 160 taps), taken at draft 4 (131 -> 8)"""
    s, images = _three(jb, BIG)
    with s.having(filter=BICUBIC, catch=True):
        host, _ = s.run(ctxs[1], 0, (8, 8), resize=(8, 8))
        assert s.error is not None and s.error.status == -9 and (host == SENT).all()
    with s.having(filter=BICUBIC):
        s.check(ctxs[4], [pr.resize(f, None, (8, 8), BICUBIC) for f in images[4]], 0, resize=(8, 8))


def test_sub_batches_give_the_same_buffer(jb, ctxs, monkeypatch):
    """A scratch cap below two images' planes and intermediates: whole images, crops and views run one image at a time."""
    s, images = _three(jb, BIG)
    fulls = images[2]
    oh, ow = fulls[0].shape[:2]
    crops = [(0, 0, ow, oh), (ow // 3, 1, ow // 3, oh - 1), (ow - 5, oh - 2, 5, 2)]
    first = s.check(ctxs[2], fulls, 0)[0]
    wants = [pr.resize_to_format(f, r, (12, 4), BILINEAR, 3, *fr.IMAGENET) for f, r in zip(fulls, crops)]
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", "16000")    # one 261 x 19 draft: 14,877 bytes of pixels, 19,008 of planes
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, draft=2) as small:   # (the knob is read when a context is created)
        assert np.array_equal(s.check(small, fulls, 0)[0], first)
        with s.having(filter=BICUBIC):
            s.check(small, [pr.resize(f, None, (30, 7), BICUBIC) for f in fulls], 0, resize=(30, 7))
        with s.having(crops=crops, filter=BILINEAR):
            s.check(small, wants, 3, fr.IMAGENET, resize=(12, 4))


# ---- 5. files ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("huff", ["2", "0"])
def test_decode_memory_and_file_give_pillows_draft_bits(jb, monkeypatch, tmp_path, huff):
    """Baseline, grayscale, progressive and restart-interval files; the entropy stage on the device and on the host."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as c:
        for K in DENOMS:
            c.set_draft(K)
            for name, jpeg, drafts in KAT:
                got = c.decode_memory(jpeg)
                assert got.shape == drafts[K].shape and np.array_equal(got, drafts[K]), (name, K)
        c.set_draft(4)
        spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
        sb = (list(spec.scale), list(spec.bias))
        for name in (BIG, "420_45x35_progressive", "420_70x40_restart", "gray_33x21"):
            _, jpeg, drafts = KAT[NAMES.index(name)]
            path = tmp_path / (name + ".jpg")
            path.write_bytes(jpeg)
            assert np.array_equal(c.decode_file(str(path)), drafts[4]), name
            oh, ow = drafts[4].shape[:2]
            roi = (1, 1, ow - 2, oh - 2)
            want = pr.resize_to_format(drafts[4], roi, (9, 5), BICUBIC, 3, *sb)
            assert fr.same_bits(c.decode_memory(jpeg, fmt=spec, roi=roi, resize=(9, 5), filter=BICUBIC), want), name


def test_decode_memory_equals_live_pillow_draft_then_resize(jb):
    Image = pytest.importorskip("PIL.Image")
    import io
    _, jpeg, _ = KAT[NAMES.index("draft_420_131x70")]
    im = Image.open(io.BytesIO(jpeg))
    im.draft("RGB", (40, 20))             # Pillow picks scale 1/2: 66 x 35
    assert im.size == (66, 35)
    want = np.asarray(im.convert("RGB").resize((24, 12), Image.BICUBIC))
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, draft=2) as c:
        assert np.array_equal(c.decode_memory(jpeg, resize=(24, 12), filter=BICUBIC), want)


MIXED = [BIG, "444_521x19", WIDE, "440_515x37_synth", "420_3x5", "gray_33x21", "420_45x35_progressive", "420_70x40_restart", "422_5x3",
         "draft_420_131x70", "420_1x1"]


def _write(tmp_path, names, K):
    paths = []
    for n in names:
        p = tmp_path / (n + ".jpg")
        p.write_bytes(KAT[NAMES.index(n)][1])
        paths.append(str(p))
    return paths, [KAT[NAMES.index(n)][2][K] for n in names]


@pytest.mark.parametrize("K", DENOMS)
def test_batch_decoder_mixed_files(jb, tmp_path, K):
    """malloc'ed and arena output at the draft frame's size, device output resized; widths / heights are the draft's"""
    import torch
    paths, rgbs = _write(tmp_path, MIXED, K)
    with jb.BatchDecoder(4, 0, arithmetic=jb.ARITH_LIBJPEG, draft=K) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, rgb in enumerate(rgbs):
            assert imgs[i].shape == rgb.shape and np.array_equal(imgs[i], rgb), MIXED[i]
        sizes, st, tm = dec.run(paths, keep_pixels=False)
        assert st == [0] * len(paths) and sizes == [(r.shape[1], r.shape[0]) for r in rgbs]
    with jb.BatchDecoder(3, 0, arena_bytes=1 << 20, arithmetic=jb.ARITH_LIBJPEG, draft=K) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        for i, rgb in enumerate(rgbs):
            assert np.array_equal(imgs[i], rgb), MIXED[i]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.BatchDecoder(2, 0, fmt=spec, resize=(14, 9), filter=BILINEAR, arithmetic=jb.ARITH_LIBJPEG, draft=K) as dec:
        out = torch.zeros((len(paths), 3, 9, 14), dtype=torch.float16, device="cuda:0")
        out, st, tm = dec.run_to_tensor(paths, out)
        assert tm["rc"] == 0 and st == [0] * len(paths), (tm, st)
        host = out.cpu().numpy()
        for i, rgb in enumerate(rgbs):
            assert fr.same_bits(host[i], pr.resize_to_format(rgb, None, (14, 9), BILINEAR, 3, *sb)), MIXED[i]


def test_batch_decoder_submit_collect_and_crops(jb, tmp_path):
    names = [BIG, "440_515x37_synth", "draft_422_131x70"]
    paths, rgbs = _write(tmp_path, names, 2)
    crops = [(8, 4, 100, 12), (200, 3, 57, 16), (3, 5, 60, 30)]           # of 261 x 19, 258 x 19, 66 x 35
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    sb = (list(spec.scale), list(spec.bias))
    with jb.BatchDecoder(2, 0, fmt=spec, resize=(32, 8), filter=BICUBIC, arithmetic=jb.ARITH_LIBJPEG, draft=2) as dec:
        t = dec.submit(paths)             # the twin side has the draft too
        t2 = dec.submit(paths, crops=crops)
        with pytest.raises(jb.JbError) as e:
            dec.set_draft(4)
        assert e.value.status == -7
        imgs, st, tm = dec.collect(t)
        assert tm["rc"] == 0 and st == [0, 0, 0], (tm, st)
        for i, rgb in enumerate(rgbs):
            assert fr.same_bits(imgs[i], pr.resize_to_format(rgb, None, (32, 8), BICUBIC, 3, *sb)), names[i]
        imgs, st, tm = dec.collect(t2)
        assert tm["rc"] == 0 and st == [0, 0, 0], (tm, st)
        for i, rgb in enumerate(rgbs):
            assert fr.same_bits(imgs[i], pr.resize_to_format(rgb, crops[i], (32, 8), BICUBIC, 3, *sb)), names[i]
        # a rectangle that lies in the full frame alone: that file's status, the batch goes on
        imgs, st, tm = dec.run(paths, crops=[crops[0], (300, 3, 57, 16), crops[2]])
        assert st == [0, -2, 0] and imgs[1] is None


def test_context_submit_and_collect(jb):
    """jb_blocks_to_rgb, jb_submit and jb_submit_batch size and fill the draft frame"""
    desc, q, coef, drafts = _kat_frame(jb, BIG)
    with _ring_context(jb, desc, 2, arithmetic=jb.ARITH_LIBJPEG, draft=4) as c:
        want = drafts[4]
        assert np.array_equal(c.blocks_to_rgb(desc, coef, q), want)
        out = np.full((want.shape[0], 3 * want.shape[1] + 5), SENT, np.uint8)
        c.wait(c.submit(desc, coef, q, out, stride=out.shape[1]))
        assert np.array_equal(out[:, :3 * want.shape[1]].reshape(want.shape), want) and (out[:, 3 * want.shape[1]:] == SENT).all()
        outs = np.full((2,) + (want.shape[0], 3 * want.shape[1]), SENT, np.uint8)
        c.wait(c.submit_batch(desc, np.ascontiguousarray(np.stack([coef, coef])), np.ascontiguousarray(np.stack([q, q])), outs))
        assert np.array_equal(outs[0].reshape(want.shape), want) and np.array_equal(outs[1], outs[0])


# ---- 6. refusals and state -----------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_buffer_alone(jb):
    s, _ = _three(jb, BIG)
    _, jpeg, _ = KAT[NAMES.index(BIG)]
    with _ring_context(jb, _kat_frame(jb, BIG)[0]) as c:      # the reference arithmetic
        for bad in (0, 3, 16, -1):
            with pytest.raises(jb.JbError) as e:
                c.set_draft(bad)
            assert e.value.status == -2 and c.draft == 1
        c.set_draft(2)                                         # the setter takes it; every call then refuses
        with s.having(catch=True):
            host, _ = s.run(c, 0, (261, 19))
            assert s.error is not None and s.error.status == -9 and (host == SENT).all()
        desc, q, coef, _ = _kat_frame(jb, BIG)
        for call in (lambda: c.decode_memory(jpeg), lambda: c.blocks_to_rgb(desc, coef, q)):
            with pytest.raises(jb.JbError) as e:
                call()
            assert e.value.status == -9
        c.set_arithmetic(jb.ARITH_LIBJPEG)
        with s.having(catch=True):                             # a scale
            host, _ = s.run(c, 0, jb.scaled_size(261, 19, 2), scale=2)
            assert s.error is not None and s.error.status == -9 and (host == SENT).all()
        with pytest.raises(jb.JbError) as e:
            c.decode_memory(jpeg, scale=2)
        assert e.value.status == -9
        for orient in (jb.ORIENT_EXIF, 3, 6):                   # an orientation, the file's own included
            c.set_orientation(orient)
            with s.having(catch=True):
                host, _ = s.run(c, 0, (261, 19))
                assert s.error is not None and s.error.status == -9 and (host == SENT).all(), orient
            with pytest.raises(jb.JbError) as e:
                c.decode_memory(jpeg)
            assert e.value.status == -9, orient
        c.set_orientation(jb.ORIENT_STORED)
        s.check(c, _three(jb, BIG)[1][2], 0)                    # and the context is as good as before


def test_decoder_setters_refuse_each_other(jb):
    with jb.BatchDecoder(1, 0) as dec:
        with pytest.raises(jb.JbError) as e:
            dec.set_draft(2)                                    # the reference arithmetic
        assert e.value.status == -9
        with pytest.raises(jb.JbError) as e:
            dec.set_draft(3)
        assert e.value.status == -2
        dec.set_draft(1)
    with jb.BatchDecoder(1, 0, arithmetic=jb.ARITH_LIBJPEG, draft=2) as dec:
        for call in (lambda: dec.set_arithmetic(jb.ARITH_REFERENCE), lambda: dec.set_scale(2), lambda: dec.set_orientation(jb.ORIENT_EXIF),
                     lambda: dec.set_orientation(6)):
            with pytest.raises(jb.JbError) as e:
                call()
            assert e.value.status == -9
        dec.set_draft(1)
        dec.set_orientation(6)
        with pytest.raises(jb.JbError) as e:
            dec.set_draft(2)
        assert e.value.status == -9
    with pytest.raises(jb.JbError) as e:
        jb.BatchDecoder(1, 0, draft=2)                           # constructors set the arithmetic before the draft
    assert e.value.status == -9
    with pytest.raises(jb.JbError) as e:
        jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, draft=5)
    assert e.value.status == -2


def test_draft_back_to_one_gives_the_full_size_bits(jb):
    desc, q, coef, drafts = _kat_frame(jb, BIG)
    s = _seam_of(jb, desc, [coef], [q], pad_row=3)
    with _ring_context(jb, desc, arithmetic=jb.ARITH_LIBJPEG) as c:
        s.check(c, [FULL[BIG]], 0)
        for K in DENOMS:
            c.set_draft(K)
            s.check(c, [drafts[K]], 0)
            assert np.array_equal(c.blocks_to_rgb(desc, coef, q), drafts[K])
        c.set_draft(1)
        assert c.draft == 1
        s.check(c, [FULL[BIG]], 0)
        assert np.array_equal(c.blocks_to_rgb(desc, coef, q), FULL[BIG])
