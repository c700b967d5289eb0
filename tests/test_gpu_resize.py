"""Fixed output size on the GPU (-m gpu): with resize=(ow, oh) every entry point returns
format_ref.to_format(resize_ref.area_resize(src, ow, oh), fmt, scale, bias) bit for bit, where `src` is the full-size
pixels -- the oracle's (seam), the reference's golden RGB (files, batch decoder) -- or the rectangle of them: never
something the code under test computed.  At the seam the whole output buffer is compared, so a byte written outside the
ow x oh elements (row, plane and image pads included) fails the test."""
import os

import numpy as np
import pytest

import format_ref as fr
from area_reduce import area_reduce
from conftest import GOLD, load_golden
from resize_ref import area_resize, area_sums
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
    c = jb.Context(0)
    yield c
    c.close()


def _params(i, fmt):
    return SETS[(i + fmt) % 3][1] if fmt >= 2 else ((1, 1, 1), (0, 0, 0))


def _seam(jb, w, h, hs, vs, coefs, qs, qtab_id=(0, 1, 1), pad_row=3, pad_plane=5, pad_img=7):
    return Seam(jb, w, h, hs, vs, coefs, qs, qtab_id, pad_row=pad_row, pad_plane=pad_plane, pad_img=pad_img)


def _check(s, ctx, srcs, resize, fmt, scale=(1, 1, 1), bias=(0, 0, 0), roi=None, tag=None):
    """The launch with `resize` (and `roi`): every image's output equals the reference of its source pixels `srcs[i]` (the
    full-size image, or its rectangle), and every other byte of the buffer still holds the sentinel."""
    wants = [fr.to_format(area_resize(src, *resize), fmt, scale, bias) for src in srcs]
    return s.check(ctx, wants, fmt, (scale, bias), roi=roi, resize=resize, tag=tag)


def _one(jb, oracle, w, h, hs, vs, seed=None):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=(w + h) if seed is None else seed)
    return _seam(jb, w, h, hs, vs, [coef], [q]), _oracle_full(oracle, w, h, hs, vs, coef, q), coef, q


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_identity_is_the_plain_decode(jb, ctx, oracle, hs, vs):
    s, full, _, _ = _one(jb, oracle, 16, 16, hs, vs)
    for fmt in (0, 1, 2, 3):
        scale, bias = _params(0, fmt)
        host, _ = _check(s, ctx, [full], (16, 16), fmt, scale, bias, tag=(hs, vs))
        old, _ = s.run(ctx, fmt, (16, 16), (scale, bias))     # the entry point without a target: the same bytes
        assert np.array_equal(host, old), (hs, vs, fmt)


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_divisible_sizes_equal_the_scaled_output(jb, ctx, oracle, hs, vs):
    from jpeg_decoder_amd import synth
    w, h = 64, 48
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=w + h)
    full = _oracle_full(oracle, w, h, hs, vs, coef, q)
    s = _seam(jb, w, h, hs, vs, [coef], [q])
    tight = Seam(jb, w, h, hs, vs, [coef], [q])
    for k in (2, 4, 8):
        host, idx = _check(s, ctx, [full], (w // k, h // k), 0, tag=(hs, vs))
        got, at = tight.check(ctx, [area_reduce(full, k)], 0, scale=k, tag=(hs, vs))   # the existing scale=k launch, bit for bit
        assert np.array_equal(host[idx[0]], got[at[0]]), (hs, vs, k)
        _check(s, ctx, [full], (w // k, h // k), 1 + k % 3, *_params(k, 1 + k % 3), tag=(hs, vs))


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_non_integer_ratio_every_layout_every_format(jb, ctx, oracle, hs, vs, fmt):
    """679 x 451 -> 224 x 224: non-integer ratios on both axes, ragged edge MCUs."""
    s, full, _, _ = _one(jb, oracle, 679, 451, hs, vs)
    _check(s, ctx, [full], (224, 224), fmt, *_params(hs + vs, fmt), tag=(hs, vs))


# (source size, targets): tiny with D not a power of two and one output pixel = the image mean; enlargement; enlargement
# on one axis and reduction on the other; more than one 4:4:4 tile per MCU row with a target wider than a wave
SMALL = [((33, 17), [(7, 5), (1, 1)]), ((9, 17), [(20, 31)]), ((1, 1), [(5, 3)]), ((40, 40), [(80, 10)]), ((520, 16), [(65, 3)])]


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_small_enlarging_and_mixed_cases(jb, ctx, oracle, hs, vs):
    k = hs + 2 * vs
    for (w, h), targets in SMALL:
        s, full, _, _ = _one(jb, oracle, w, h, hs, vs)
        for t in targets:
            for fmt in (0, 1 + k % 3):     # format 0 everywhere; the planar ones in turn
                _check(s, ctx, [full], t, fmt, *_params(k, 1 + k % 3), tag=(hs, vs, w, h))
                k += 1
    # one output pixel is the image mean, rounded half up
    s, full, _, _ = _one(jb, oracle, 33, 17, hs, vs)
    host, idx = _check(s, ctx, [full], (1, 1), 0, tag=(hs, vs))
    tot = full.astype(np.int64).sum(axis=(0, 1))
    assert np.array_equal(host[idx[0]].ravel(), (tot + (33 * 17) // 2) // (33 * 17))


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_rectangle_then_resize(jb, ctx, oracle, hs, vs):
    """100 x 80, roi (5, 3, 50, 40) -- not MCU-aligned -- resized to 13 x 11."""
    s, full, _, _ = _one(jb, oracle, 100, 80, hs, vs)
    x, y, w, h = roi = (5, 3, 50, 40)
    for fmt in (0, 1, 2, 3):
        _check(s, ctx, [full[y:y + h, x:x + w]], (13, 11), fmt, *_params(hs, fmt), roi=roi, tag=(hs, vs))


def test_seam_sums_beyond_32_bits(jb, ctx, oracle):
    """4608 x 4608 4:2:0, bright: the sums of a 1 x 1 and a 2 x 3 target do not fit 32 bits, so the 64-bit accumulation
    and the division are exercised."""
    from jpeg_decoder_amd import synth
    w = h = 4608
    q = synth.annex_k_qtabs(50)
    n = synth.geometry(w, h, 2, 2)[3]
    rng = np.random.default_rng(4608)
    coef = np.zeros((n, 64), np.int16)
    blk = np.arange(n) % 6
    # luma DC 52..60 (x 16 / 8 + 128 = 232..248), a little AC; chroma near zero
    coef[:, 0] = np.where(blk < 4, rng.integers(52, 61, n), rng.integers(-1, 2, n))
    coef[:, 1] = np.where(blk < 4, rng.integers(-2, 3, n), 0)
    full = _oracle_full(oracle, w, h, 2, 2, coef, q)
    s = _seam(jb, w, h, 2, 2, [coef], [q])
    for t in ((1, 1), (2, 3)):
        assert area_sums(full, *t).max() > 2 ** 32
        _check(s, ctx, [full], t, 0)
    _check(s, ctx, [full], (2, 3), 3, *fr.IMAGENET)


def test_seam_refusals(jb, ctx):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(64, 48, 1, 1)
    s = _seam(jb, 64, 48, 1, 1, [coef], [q])
    for bad in ((0, 8), (8, 0), (65536, 8), (-1, 8)):
        with pytest.raises(jb.JbError) as e:
            s.run(ctx, 0, (8, 8), resize=bad)
        assert e.value.status == -2, bad
    with pytest.raises(jb.JbError) as e:
        s.run(ctx, 0, (8, 8), roi=(60, 40, 5, 8), resize=(8, 8))     # the rectangle does not fit
    assert e.value.status == -2
    with pytest.raises(jb.JbError) as e:
        ctx.blocks_to_rgb_device(jb.DeviceBatch(), scale=2, resize=(8, 8))
    assert e.value.status == -9
    ctx.synchronize()


# ---- a batch, and the same batch in sub-batches ----------------------------------------------------
BW, BH = 333, 203


def _batch5(jb, oracle, hs=2, vs=2):
    from jpeg_decoder_amd import synth
    qid = (0, 1, 2)
    coefs, qs, fulls = [], [], []
    for i in range(5):
        q = synth.annex_k_qtabs(40 + 12 * i).copy()          # per-image quantisation tables
        q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1, 1, 255)
        c = synth.synth_blocks(BW, BH, hs, vs, image_index=20 + i, qtabs=q, qtab_id=qid, dense=(i == 4))[0]
        coefs.append(c), qs.append(q)
        fulls.append(_oracle_full(oracle, BW, BH, hs, vs, c, q, qid))
    return _seam(jb, BW, BH, hs, vs, coefs, qs, qid, pad_row=13, pad_plane=7, pad_img=77), fulls


def test_seam_batch_of_five_and_its_sub_batches(jb, ctx, oracle, monkeypatch):
    """n_images = 5 with per-image tables; then the same launches on contexts whose scratch holds fewer than two (one
    image per sub-batch) and fewer than three (2 + 2 + 1) intermediates: identical buffers.  (The knob belongs to the
    context: it is read when one is created, so a new context in this process has it.)"""
    s, fulls = _batch5(jb, oracle)
    cases = [((100, 60), 0, None), ((100, 60), 3, None), ((224, 224), 2, None), ((50, 41), 1, (37, 18, 224, 160))]
    first = []
    for k, (t, fmt, roi) in enumerate(cases):
        srcs = fulls if roi is None else [f[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]] for f in fulls]
        first.append(_check(s, ctx, srcs, t, fmt, *_params(k, fmt), roi=roi)[0])
    tmp = 3 * BW * BH
    for cap in (tmp * 3 // 2, tmp * 5 // 2):
        monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
        with jb.Context(0) as small:
            for k, (t, fmt, roi) in enumerate(cases):
                host, _ = s.run(small, fmt, t, _params(k, fmt), roi=roi, resize=t)
                assert np.array_equal(host, first[k]), (cap, t, fmt, roi)


# ---- files ---------------------------------------------------------------------------------------
def _gold(name):
    return os.path.join(GOLD, "images", name + ".jpg"), load_golden(name)[3]


@pytest.mark.parametrize("huff", ["2", "0"])
@pytest.mark.parametrize("name", ["img2", "img4"])
def test_decode_file_and_memory_resized_golden(jb, monkeypatch, name, huff):
    """decode_file / decode_memory(resize=) with and without roi == the reference of the reference decoder's own RGB,
    entropy stage on the device (=2) and on the host (=0), format 0 and normalised f16."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    path, rgb = _gold(name)
    h, w = rgb.shape[:2]
    data = open(path, "rb").read()
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.Context(0) as c:   # (the knob is read when the context is created)
        for roi, t in ((None, (224, 224)), (None, (w, h)), ((w // 4, h // 4, w // 2, h // 2), (33, 47)), ((w - 3, h - 2, 3, 2), (8, 8))):
            src = rgb if roi is None else rgb[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]
            for fmt, sp in ((0, None), (3, spec)):
                want = fr.to_format(area_resize(src, *t), fmt, list(spec.scale), list(spec.bias))
                assert fr.same_bits(c.decode_file(path, fmt=sp, roi=roi, resize=t), want), (name, roi, t, fmt)
                assert fr.same_bits(c.decode_memory(data, fmt=sp, roi=roi, resize=t), want), (name, roi, t, fmt)
        for call in (lambda **kw: c.decode_file(path, **kw), lambda **kw: c.decode_memory(data, fmt=spec, **kw)):
            for kw in (dict(resize=(0, 5)), dict(resize=(5, 65536)), dict(resize=(8, 8), roi=(1, 0, w, h))):
                with pytest.raises(jb.JbError) as e:
                    call(**kw)
                assert e.value.status == -2, kw
        assert np.array_equal(c.decode_file(path), rgb)   # and the context still decodes whole images


# ---- the batch decoder ---------------------------------------------------------------------------
NAMES = ["img2", "img4", "img6", "img", "img2"]     # 400x266 4:2:0, 800x400 4:4:4, 427x640 4:2:0, 679x451 4:2:0
T = (32, 32)


def _want(rgb, spec, roi=None, t=T):
    src = rgb if roi is None else rgb[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]
    return fr.to_format(area_resize(src, *t), spec.format, list(spec.scale), list(spec.bias))


@pytest.mark.parametrize("huff", ["0", None])
def test_batch_decoder_resize_every_route(jb, monkeypatch, huff):
    import torch
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    paths, n = list(paths), len(NAMES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(4, 0, resize=T, fmt=spec) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert fr.same_bits(imgs[i], _want(rgbs[i], spec)), i
        out = torch.full((n, 3, T[1], T[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out)
        assert ret is out and st == [0] * n, (st, tm)
        got = out.cpu().numpy()
        for i in range(n):
            assert fr.same_bits(got[i], _want(rgbs[i], spec)), i
        t0 = dec.submit(paths)
        t1 = dec.submit(paths[::-1])                       # two in flight: the twin side has the target too
        with pytest.raises(jb.JbError) as e:
            dec.set_resize((8, 8))
        assert e.value.status == -7                        # JB_ERR_STATE
        for t, order in ((t0, list(range(n))), (t1, list(range(n))[::-1])):
            imgs, st, tm = dec.collect(t)
            assert tm["rc"] == 0 and st == [0] * n, (tm, st)
            for k, i in enumerate(order):
                assert fr.same_bits(imgs[k], _want(rgbs[i], spec)), i
        # a rectangle that does not fit img2 (400 wide): -2 for those files only, the others are its resize
        roi = (0, 0, 410, 260)
        dec.set_roi(roi)
        imgs, st, tm = dec.run(paths)
        for i in range(n):
            if NAMES[i] == "img2":
                assert st[i] == -2 and imgs[i] is None, (i, st)
            else:
                assert st[i] == 0 and fr.same_bits(imgs[i], _want(rgbs[i], spec, roi)), (i, st)
        dec.set_roi(None)
        # uint8 interleaved, another target, host output
        dec.set_output_format(0)
        dec.set_resize((57, 40))
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert np.array_equal(imgs[i], area_resize(rgbs[i], 57, 40)), i
        # a target and a scale exclude each other, whichever comes second
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(2)
        assert e.value.status == -9
        dec.set_resize(None)
        dec.set_scale(2)
        with pytest.raises(jb.JbError) as e:
            dec.set_resize(T)
        assert e.value.status == -9
        dec.set_scale(1)
        for bad in ((0, 5), (5, 0), (65536, 1), (-1, 4)):
            with pytest.raises(jb.JbError) as e:
                dec.set_resize(bad)
            assert e.value.status == -2
        imgs, st, tm = dec.run(paths)                       # whole images again, byte for byte
        assert tm["rc"] == 0 and st == [0] * n, (tm, st)
        for i in range(n):
            assert np.array_equal(imgs[i], rgbs[i]), i
