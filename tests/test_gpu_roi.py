"""Region of interest on the GPU (-m gpu): a crop is the slice of the full decode.  With the rectangle (x, y, w, h) every
entry point that takes one returns format_ref.to_format(full[y:y+h, x:x+w], fmt, scale, bias) bit for bit, where `full`
is the oracle's pixels (seam), the reference's golden RGB (files) or the same decoder's output without a rectangle (batch
routes) -- never something the code under test computed.  At the seam the whole output buffer is compared, so a byte
written outside the rectangle (row, plane and image pads included) fails the test."""
import os

import numpy as np
import pytest

import format_ref as fr
from conftest import BASELINE_IMAGES, GOLD, load_golden
from seam_harness import LAYOUTS, Seam, _oracle_full

pytestmark = pytest.mark.gpu

SETS = list(fr.PARAM_SETS.items())


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def ctx(jb):
    c = jb.Context(0, 64 << 20, 64 << 20, 3)
    yield c
    c.close()


def _seam(jb, w, h, hs, vs, coefs, qs, qtab_id=(0, 1, 1), pad_row=3, pad_plane=5, pad_img=0):
    return Seam(jb, w, h, hs, vs, coefs, qs, qtab_id, pad_row=pad_row, pad_plane=pad_plane, pad_img=pad_img)


def _check(s, ctx, fulls, roi, fmt, scale=(1, 1, 1), bias=(0, 0, 0), tag=None):
    """The launch with `roi`: every image's output equals format_ref of the slice of its full-size pixels, and every
    other byte of the buffer still holds the sentinel.  -> the buffer."""
    x, y, w, h = roi
    return s.check(ctx, [fr.to_format(full[y:y + h, x:x + w], fmt, scale, bias) for full in fulls], fmt, (scale, bias), roi=roi, tag=tag)[0]


def _rotated(i, fmt):
    name, (scale, bias) = SETS[(i + fmt) % 3]
    return (scale, bias) if fmt >= 2 else ((1, 1, 1), (0, 0, 0))


W1, H1 = 1100, 45   # more than one 512- (4:2:2: 1024-) pixel tile per row in every layout, ragged in both directions
RECTS = [(0, 0, W1, H1), (0, 0, 1, 1), (1099, 44, 1, 1),
         (1, 0, 1099, 45), (2, 1, 1097, 43), (3, 0, 3, 45),
         (5, 3, 2, 2), (6, 4, 1, 9),                                      # left and right edge in one 4-pixel group
         (255, 0, 2, 45), (253, 7, 7, 1), (509, 11, 6, 5), (1021, 15, 8, 17), (1023, 16, 77, 29),   # segment / tile boundaries
         (513, 17, 224, 24),                                              # starts in the second tile
         (876, 0, 224, 45)]                                               # the right edge is the ragged image edge
RECTS += [(300, y, 224, h) for y, h in ((3, 1), (4, 1), (7, 2), (8, 8), (15, 2), (9, 36))]   # phase / MCU-row boundaries


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_chosen_rectangles_every_format(jb, ctx, oracle, hs, vs):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(W1, H1, hs, vs, image_index=W1 + H1)
    full = _oracle_full(oracle, W1, H1, hs, vs, coef, q)
    s = _seam(jb, W1, H1, hs, vs, [coef], [q])
    for fmt in (0, 1, 2, 3):
        for i, roi in enumerate(RECTS):
            scale, bias = _rotated(i, fmt)
            host = _check(s, ctx, [full], roi, fmt, scale, bias, tag=(hs, vs))
            if i == 0:   # the whole image through the ROI instantiation: the bytes of the entry point without a rectangle
                old, _ = s.run(ctx, fmt, (W1, H1), (scale, bias))
                assert np.array_equal(host, old), (hs, vs, fmt)


W2, H2 = 45, 37
ENUM_X = list(range(18))
ENUM_W = [1, 2, 3, 4, 5, None]                      # None: to the edge
ENUM_Y = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17]
ENUM_H = [1, 2, None]


@pytest.mark.parametrize("fmt", [0, 3])
@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2)])
def test_seam_enumerated_rectangles(jb, ctx, oracle, hs, vs, fmt):
    """On a 45 x 37 image: every x in 0..17 x w in {1, 2, 3, 4, 5, to the edge} x y in {0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17}
    x h in {1, 2, to the edge} -- the full set of the issue, nothing thinned: 3,564 rectangles per case, the coefficients
    uploaded once, one output buffer whose sentinel is refilled on the device."""
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(W2, H2, hs, vs, image_index=W2 + H2)
    full = _oracle_full(oracle, W2, H2, hs, vs, coef, q)
    s = _seam(jb, W2, H2, hs, vs, [coef], [q])
    k = 0
    for x in ENUM_X:
        for w in ENUM_W:
            for y in ENUM_Y:
                for h in ENUM_H:
                    roi = (x, y, W2 - x if w is None else w, H2 - y if h is None else h)
                    scale, bias = _rotated(k, fmt)
                    _check(s, ctx, [full], roi, fmt, scale, bias, tag=(hs, vs))
                    k += 1
    assert k == 18 * 6 * 11 * 3


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_batch_strides_dense_mixed_tables_and_parameter_sets(jb, ctx, oracle, hs, vs):
    """3 images of 333 x 203 as test_gpu_format.py builds them (full-range coefficients, a dense image, different Cb / Cr
    tables: the MIXQ instantiation of 4:2:0), padded row, plane and image strides, the rectangle (37, 18, 224, 160)."""
    from jpeg_decoder_amd import synth
    w, h = 333, 203
    qid = (0, 1, 2)
    g = jb.geometry_of(jb.make_desc(w, h, hs, vs))
    q = synth.annex_k_qtabs(50).copy()
    q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1, 1, 255)
    coefs = [synth.random_blocks(g.n_coded_blocks, 7 + i) for i in range(2)]
    coefs.append(synth.synth_blocks(w, h, hs, vs, image_index=9, qtabs=q, qtab_id=qid, dense=True)[0])
    fulls = [_oracle_full(oracle, w, h, hs, vs, c, q, qid) for c in coefs]
    s = _seam(jb, w, h, hs, vs, coefs, [q] * 3, qid, pad_row=13, pad_plane=7, pad_img=77)
    cases = [(fr.FMT_RGB_U8_HWC, ((1, 1, 1), (0, 0, 0))), (fr.FMT_RGB_U8_CHW, ((1, 1, 1), (0, 0, 0)))]
    cases += [(fmt, sb) for fmt in (fr.FMT_RGB_F32_CHW, fr.FMT_RGB_F16_CHW) for _, sb in SETS]
    for fmt, (scale, bias) in cases:
        _check(s, ctx, fulls, (37, 18, 224, 160), fmt, scale, bias, tag=(hs, vs))


def test_seam_refusals(jb, ctx):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(64, 48, 1, 1)
    s = _seam(jb, 64, 48, 1, 1, [coef], [q])
    for roi in ((0, 0, 65, 48), (0, 0, 64, 49), (-1, 0, 4, 4), (0, 0, 0, 4), (2 ** 31 - 1, 0, 2, 1), (60, 40, 5, 8)):
        with pytest.raises(jb.JbError) as e:
            s.run(ctx, 0, (roi[2], roi[3]), roi=roi)
        assert e.value.status == -2, roi
    with pytest.raises(jb.JbError) as e:
        ctx.blocks_to_rgb_device(jb.DeviceBatch(), scale=2, roi=(0, 0, 8, 8))
    assert e.value.status == -9
    ctx.synchronize()


def _roi_cases(w, h):
    return [(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)), (w - 1, h - 1, 1, 1)]


@pytest.mark.parametrize("huff", ["2", "0"])
@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_decode_file_and_memory_roi_golden(jb, monkeypatch, name, huff):
    """decode_file / decode_memory(roi=) == the slice of the reference's own RGB, entropy stage on the device (=2) and on
    the host (=0), format 0 and normalised f16; a rectangle one pixel too wide is JB_ERR_GEOMETRY and says both sizes."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    _, _, _, rgb = load_golden(name)
    h, w = rgb.shape[:2]
    path = os.path.join(GOLD, "images", name + ".jpg")
    data = open(path, "rb").read()
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.Context(0) as c:   # (the knob is read when the context is created)
        for roi in _roi_cases(w, h):
            x, y, rw, rh = roi
            for fmt, sp in ((0, None), (3, spec)):
                want = fr.to_format(rgb[y:y + rh, x:x + rw], fmt, list(spec.scale), list(spec.bias))
                assert fr.same_bits(c.decode_file(path, fmt=sp, roi=roi), want), (name, roi, fmt)
                assert fr.same_bits(c.decode_memory(data, fmt=sp, roi=roi), want), (name, roi, fmt)
        for call in (lambda r: c.decode_file(path, roi=r), lambda r: c.decode_memory(data, fmt=spec, roi=r)):
            for bad in ((0, 0, w + 1, h), (1, 0, w, h), (0, 0, w, h + 1)):
                with pytest.raises(jb.JbError) as e:
                    call(bad)
                assert e.value.status == -2
                assert f"{bad[2]} x {bad[3]}" in str(e.value) and f"{w} x {h}" in str(e.value), str(e.value)
        assert np.array_equal(c.decode_file(path), rgb)   # and the context still decodes whole images
        if huff == "0":
            assert c.device_entropy_images == 0


def test_decode_memory_roi_device_entropy_path_runs(jb, monkeypatch):
    """(the golden images may all be too small for the device entropy stage: a 1080p writer file is not)"""
    from jpeg_decoder_amd import synth
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "2")
    coef, q = synth.synth_blocks(1920, 1080, 2, 2, image_index=3)
    data = synth.encode_jpeg(coef, 1920, 1080, 2, 2, q, restart_interval=0)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.Context(0) as c:
        full = c.decode_memory(data)
        n0 = c.device_entropy_images
        assert n0 > 0
        k = 0
        for roi in _roi_cases(1920, 1080) + [(848, 428, 224, 224)]:
            x, y, rw, rh = roi
            for fmt, sp in ((0, None), (3, spec)):
                want = fr.to_format(full[y:y + rh, x:x + rw], fmt, list(spec.scale), list(spec.bias))
                assert fr.same_bits(c.decode_memory(data, fmt=sp, roi=roi), want), (roi, fmt)
                k += 1
        assert c.device_entropy_images == n0 + k


ROI_B = (20, 10, 224, 160)


@pytest.fixture(scope="module")
def sized_files(tmp_path_factory):
    """Writer files of five sizes and all four samplings; ROI_B fits every one but the 200 x 150 file (index 4)."""
    from jpeg_decoder_amd import synth
    d = tmp_path_factory.mktemp("roi")
    paths = []
    for j, (w, h, hs, vs, ri) in enumerate([(640, 360, 2, 2, 10), (333, 211, 1, 1, 0), (517, 300, 2, 1, 8), (250, 177, 1, 2, 0),
                                            (200, 150, 2, 2, 0), (1920, 1080, 1, 1, 240), (244, 170, 2, 2, 0)]):
        coef, q = synth.synth_blocks(w, h, hs, vs, image_index=90 + j)
        p = os.path.join(str(d), f"r{j}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri))
        paths.append(p)
    return paths


MISFIT = 4


def _check_batch(imgs, st, tm, fulls, roi, spec=None, order=None):
    x, y, w, h = roi
    order = list(range(len(fulls))) if order is None else order
    assert [s for i, s in zip(order, st) if i != MISFIT] == [0] * (len(fulls) - 1), (st, tm)
    for k, i in enumerate(order):
        if i == MISFIT:
            assert st[k] == -2 and imgs[k] is None, (st[k], tm)
            continue
        fmt, sc, bi = (0, (1, 1, 1), (0, 0, 0)) if spec is None else (spec.format, list(spec.scale), list(spec.bias))
        assert fr.same_bits(imgs[k], fr.to_format(fulls[i][y:y + h, x:x + w], fmt, sc, bi)), i


@pytest.mark.parametrize("huff", ["0", None])
def test_batch_decoder_roi_run_and_submit_collect(jb, monkeypatch, sized_files, huff):
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    with jb.BatchDecoder(4, 0) as dec:
        fulls, st, tm = dec.run(sized_files)                      # the same decoder's un-cropped output
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
    n = len(sized_files)
    with jb.BatchDecoder(4, 0, roi=ROI_B) as dec:
        imgs, st, tm = dec.run(sized_files)
        assert tm["rc"] == -2                                     # (the first failing status), and the batch went on:
        _check_batch(imgs, st, tm, fulls, ROI_B)
        spec = jb.OutputSpec.make(fr.FMT_RGB_F32_CHW, *fr.UNIT)
        dec.set_output_format(spec)                               # a rectangle with a format
        imgs, st, tm = dec.run(sized_files)
        _check_batch(imgs, st, tm, fulls, ROI_B, spec)
        dec.set_output_format(0)
        t0 = dec.submit(sized_files)
        t1 = dec.submit(sized_files[::-1])                        # two in flight: the twin side has the rectangle too
        with pytest.raises(jb.JbError) as e:
            dec.set_roi((0, 0, 8, 8))
        assert e.value.status == -7                               # JB_ERR_STATE
        imgs, st, tm = dec.collect(t0)
        _check_batch(imgs, st, tm, fulls, ROI_B)
        imgs, st, tm = dec.collect(t1)
        _check_batch(imgs, st, tm, fulls, ROI_B, order=list(range(n))[::-1])
        other = (3, 5, 100, 99)                                   # another rectangle reaches both sides; it fits every file
        dec.set_roi(other)
        for t in (dec.submit(sized_files), dec.submit(sized_files)):
            imgs, st, tm = dec.collect(t)
            assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
            for i in range(n):
                assert np.array_equal(imgs[i], fulls[i][5:104, 3:103]), i
        if huff is None:
            assert dec.device_entropy_images > 0
        # a rectangle and a scale exclude each other, whichever comes second
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(2)
        assert e.value.status == -9
        dec.set_roi(None)
        dec.set_scale(2)
        with pytest.raises(jb.JbError) as e:
            dec.set_roi(ROI_B)
        assert e.value.status == -9
        dec.set_scale(1)
        for bad in ((0, 0, 0, 1), (-1, 0, 5, 5), (0, 0, 65536, 1), (2 ** 31 - 1, 0, 2, 1)):   # no frame holds these
            with pytest.raises(jb.JbError) as e:
                dec.set_roi(bad)
            assert e.value.status == -2
        # whole images again, byte for byte
        imgs, st, tm = dec.run(sized_files)
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
        for i in range(n):
            assert np.array_equal(imgs[i], fulls[i]), i


def test_batch_decoder_roi_run_to_tensor_over_mixed_sizes(jb, sized_files):
    """One [N, 3, h, w] tensor from files of different sizes: the case run_to_tensor could not take without a rectangle."""
    import torch
    with jb.BatchDecoder(4, 0) as dec:
        fulls, st, tm = dec.run(sized_files)
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
        spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
        dec.set_output_format(spec)
        dec.set_roi(ROI_B)
        x, y, w, h = ROI_B
        n = len(sized_files)
        out = torch.full((n, 3, h, w), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(sized_files, out)
        assert ret is out
        assert st[MISFIT] == -2 and [s for i, s in enumerate(st) if i != MISFIT] == [0] * (n - 1), (st, tm)
        got = out.cpu().numpy()
        for i in range(n):
            if i == MISFIT:
                assert (got[i] == np.float16(7.0)).all()          # left as it was
            else:
                assert fr.same_bits(got[i], fr.to_format(fulls[i][y:y + h, x:x + w], 3, list(spec.scale), list(spec.bias))), i
