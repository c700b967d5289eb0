"""Tensor-ready output on the GPU (-m gpu): every entry point that takes an output format equals tests/format_ref.py
applied to the full-size interleaved output it is defined by -- the oracle's pixels at the seam, the reference's golden
RGB for decode(path), the same decoder's format-0 output on the batch routes.  Every comparison is on the raw bits.
Format 0 through the new entry points is byte-identical to the old ones; a format with a scale is refused."""
import os

import numpy as np
import pytest

import format_ref as fr
from conftest import BASELINE_IMAGES, GOLD, load_golden
from seam_harness import LAYOUTS, SEAM_SIZES, Seam, _oracle_full

pytestmark = pytest.mark.gpu

NEW_FORMATS = (fr.FMT_RGB_U8_CHW, fr.FMT_RGB_F32_CHW, fr.FMT_RGB_F16_CHW)
SETS = list(fr.PARAM_SETS.items())
PROGRESSIVE = os.path.join(GOLD, "images", "prograssive-sample-2.jpg")


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


@pytest.mark.parametrize("hs,vs", LAYOUTS)
@pytest.mark.parametrize("w,h", SEAM_SIZES)
def test_seam_formats_equal_format_ref_of_oracle(jb, ctx, oracle, hs, vs, w, h):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=w + h)
    full = _oracle_full(oracle, w, h, hs, vs, coef, q)
    big = w * h > 4 << 20
    # padded rows / planes on everything but the largest size (tight: the spec's plane stride is 0, the seam derives it)
    s = Seam(jb, w, h, hs, vs, [coef], [q], **(dict(pad_row=0, pad_plane=0) if big else dict(pad_row=3, pad_plane=5)))
    for fmt in NEW_FORMATS:
        name, (scale, bias) = SETS[(w + h + fmt) % 3]
        s.check(ctx, [fr.to_format(full, fmt, scale, bias)], fmt, (scale, bias), tag=(w, h, hs, vs, name))


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_formats_batch_strides_dense_mixed_tables_and_parameter_sets(jb, ctx, oracle, hs, vs):
    """3 images with padded row, plane and image strides, full-range coefficients (outputs clamp at 0 and at 255, and
    every uint8 value occurs), different Cb / Cr tables (the MIXQ instantiation of 4:2:0); the float formats with all
    three parameter sets: ImageNet, 1/255 (separates round-to-nearest from round-toward-zero multiplies) and
    1 + 2**-11 (f16 ties)."""
    from jpeg_decoder_amd import synth
    w, h = 333, 203
    qid = (0, 1, 2)
    g = jb.geometry_of(jb.make_desc(w, h, hs, vs))
    q = synth.annex_k_qtabs(50).copy()
    q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1, 1, 255)
    coefs = [synth.random_blocks(g.n_coded_blocks, 7 + i) for i in range(2)]
    coefs.append(synth.synth_blocks(w, h, hs, vs, image_index=9, qtabs=q, qtab_id=qid, dense=True)[0])
    qs = [q] * 3
    fulls = [_oracle_full(oracle, w, h, hs, vs, c, q, qid) for c in coefs]
    assert any((f == 0).any() and (f == 255).any() for f in fulls)
    assert np.unique(np.concatenate([f.ravel() for f in fulls])).size == 256
    cases = [(fr.FMT_RGB_U8_CHW, "none", ((1, 1, 1), (0, 0, 0)))]
    cases += [(fmt, name, sb) for fmt in (fr.FMT_RGB_F32_CHW, fr.FMT_RGB_F16_CHW) for name, sb in SETS]
    s = Seam(jb, w, h, hs, vs, coefs, qs, qid, pad_row=13, pad_plane=7, pad_img=77)
    for fmt, name, (scale, bias) in cases:
        s.check(ctx, [fr.to_format(full, fmt, scale, bias) for full in fulls], fmt, (scale, bias), tag=(hs, vs, name))


def _device_batch(jb, w, h, hs, vs, es=1):
    import torch
    from jpeg_decoder_amd import synth
    desc = jb.make_desc(w, h, hs, vs)
    coef, q = synth.synth_blocks(w, h, hs, vs)
    keep = [torch.from_numpy(coef).to("cuda:0"), torch.from_numpy(jb.resolve_qtabs(desc, q)).to("cuda:0"),
            torch.zeros(3 * w * h * 4 + 64, dtype=torch.uint8, device="cuda:0")]
    b = jb.DeviceBatch()
    b.desc, b.n_images = desc, 1
    b.d_coef, b.coef_image_stride = keep[0].data_ptr(), coef.nbytes
    b.d_qtabs, b.d_rgb = keep[1].data_ptr(), keep[2].data_ptr()
    b.rgb_row_stride, b.rgb_image_stride = w * es, 3 * w * h * es
    return b, keep, (coef, q)


def test_seam_format_zero_is_the_old_seam_and_refusals(jb, ctx):
    import torch
    w, h = 679, 451
    for hs, vs in LAYOUTS:
        b, keep, (coef, q) = _device_batch(jb, w, h, hs, vs)
        b.rgb_row_stride, b.rgb_image_stride = 3 * w, 3 * w * h
        ctx.blocks_to_rgb_device(b, fmt=0)
        ctx.synchronize()
        via_fmt = keep[2][:3 * w * h].cpu().numpy().copy()
        keep[2].zero_()
        torch.cuda.synchronize()
        ctx.blocks_to_rgb_device(b)
        ctx.synchronize()
        assert np.array_equal(via_fmt, keep[2][:3 * w * h].cpu().numpy())
        assert np.array_equal(via_fmt.reshape(h, w, 3), ctx.blocks_to_rgb(jb.make_desc(w, h, hs, vs), coef, q))
    L = jb.lib()
    import ctypes

    def rc(b, spec, scale=1):
        if scale != 1:
            with pytest.raises(jb.JbError) as e:
                ctx.blocks_to_rgb_device(b, scale=scale, fmt=spec)
            return e.value.status
        return L.jb_blocks_to_rgb_device_fmt(ctx._h, ctypes.byref(b), ctypes.byref(spec), None)

    b, keep, _ = _device_batch(jb, 64, 64, 1, 1)
    assert rc(b, jb.OutputSpec.make(1)) == 0
    assert rc(b, jb.OutputSpec.make(4)) == -2 and rc(b, jb.OutputSpec.make(-1)) == -2        # unknown format
    for fmt in (0, 1):
        s = jb.OutputSpec.make(fmt)
        s.reserved = 7
        assert rc(b, s) == -2
    assert rc(b, jb.OutputSpec.make(1, plane_stride=64 * 64 - 1)) == -2                       # planes would overlap
    assert rc(b, jb.OutputSpec.make(2, [1, float("nan"), 1])) == -2
    assert rc(b, jb.OutputSpec.make(3, bias=[0, 0, float("inf")])) == -2
    b.rgb_row_stride = 63                                                                     # a row does not fit
    assert rc(b, jb.OutputSpec.make(1)) == -2
    for fmt, es in ((2, 4), (3, 2)):                                                          # float formats: element alignment
        b, keep, _ = _device_batch(jb, 64, 64, 1, 1, es)
        assert rc(b, jb.OutputSpec.make(fmt)) == 0
        b.d_rgb += 1
        assert rc(b, jb.OutputSpec.make(fmt)) == -2
        b.d_rgb -= 1
        b.rgb_row_stride += 1
        assert rc(b, jb.OutputSpec.make(fmt)) == -2
        b.rgb_row_stride -= 1
        assert rc(b, jb.OutputSpec.make(fmt, plane_stride=64 * 64 * es + 1)) == -2
    for fmt in NEW_FORMATS:                                                                   # a format with a scale
        for k in (2, 4, 8):
            assert rc(b, jb.OutputSpec.make(fmt), scale=k) == -9
    ctx.synchronize()


def _fresh_ctx(jb):
    return jb.Context(0)


@pytest.mark.parametrize("huff", ["2", "0"])
@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_decode_file_and_memory_formats_golden(jb, monkeypatch, name, huff):
    """decode_file / decode_memory(fmt=) == format_ref of the reference's own RGB, with the entropy stage on the device
    (JPEGBLK_GPU_HUFFMAN=2) and on the host (=0); format 0 == the old entry points; a format with a scale is refused."""
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    _, _, _, rgb = load_golden(name)
    path = os.path.join(GOLD, "images", name + ".jpg")
    data = open(path, "rb").read()
    with _fresh_ctx(jb) as c:   # (the knob is read when the context is created)
        assert np.array_equal(c.decode_file(path), rgb)
        assert fr.same_bits(c.decode_file(path, fmt=0), rgb) and fr.same_bits(c.decode_memory(data, fmt=0), rgb)
        for k, fmt in enumerate(NEW_FORMATS):
            sname, (scale, bias) = SETS[k % 3]
            spec = jb.OutputSpec.make(fmt, scale, bias)
            want = fr.to_format(rgb, fmt, scale, bias)
            assert fr.same_bits(c.decode_file(path, fmt=spec), want), (name, fmt, sname)
            assert fr.same_bits(c.decode_memory(data, fmt=spec), want), (name, fmt, sname)
            for scale_k in (2, 8):
                with pytest.raises(jb.JbError) as e:
                    c.decode_file(path, scale=scale_k, fmt=spec)
                assert e.value.status == -9
        n_dev = c.device_entropy_images
    if huff == "0":
        assert n_dev == 0


def test_decode_memory_formats_device_entropy_path_runs(jb, monkeypatch):
    """(the golden images may all be too small for the device entropy stage: a 1080p writer file is not)"""
    from jpeg_decoder_amd import synth
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "2")
    coef, q = synth.synth_blocks(1920, 1080, 2, 2, image_index=3)
    data = synth.encode_jpeg(coef, 1920, 1080, 2, 2, q, restart_interval=0)
    with _fresh_ctx(jb) as c:
        full = c.decode_memory(data)
        n0 = c.device_entropy_images
        assert n0 > 0
        for fmt in NEW_FORMATS:
            spec = jb.OutputSpec.imagenet(fmt)
            got = c.decode_memory(data, fmt=spec)
            assert fr.same_bits(got, fr.to_format(full, fmt, list(spec.scale), list(spec.bias))), fmt
        assert c.device_entropy_images == n0 + 3
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "0")
    with _fresh_ctx(jb) as c:
        for fmt in NEW_FORMATS:
            spec = jb.OutputSpec.imagenet(fmt)
            assert fr.same_bits(c.decode_memory(data, fmt=spec), fr.to_format(full, fmt, list(spec.scale), list(spec.bias))), fmt
        assert c.device_entropy_images == 0


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    """Writer files of several sizes and samplings, with and without restart intervals, the bundled baseline images and
    one progressive file (which the device entropy stage refuses: it takes the host path inside the batch)."""
    from jpeg_decoder_amd import synth
    d = tmp_path_factory.mktemp("formats")
    paths = []
    specs = [(640, 360, 2, 2, 10), (333, 211, 1, 1, 0), (1920, 1080, 1, 1, 240), (517, 300, 2, 1, 8), (250, 177, 1, 2, 0),
             (1, 1, 1, 1, 0), (7, 13, 2, 2, 0)]
    for j, (w, h, hs, vs, ri) in enumerate(specs):
        for r in range(2):
            coef, q = synth.synth_blocks(w, h, hs, vs, image_index=60 + 2 * j + r)
            p = os.path.join(str(d), f"m{j}_{r}.jpg")
            with open(p, "wb") as f:
                f.write(synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri))
            paths.append(p)
    paths += [os.path.join(GOLD, "images", n + ".jpg") for n in BASELINE_IMAGES]
    assert os.path.exists(PROGRESSIVE)
    paths.insert(3, PROGRESSIVE)
    return paths


def _refs(imgs0, spec):
    return [fr.to_format(f, spec.format, list(spec.scale), list(spec.bias)) for f in imgs0]


def _check(imgs, st, tm, refs):
    assert tm["rc"] == 0 and all(s == 0 for s in st), (tm["rc"], tm["error"], st)
    for i, (g, want) in enumerate(zip(imgs, refs)):
        assert g is not None and fr.same_bits(g, want), i


def _specs(jb):
    return [jb.OutputSpec.make(fr.FMT_RGB_U8_CHW), jb.OutputSpec.imagenet(fr.FMT_RGB_F32_CHW),
            jb.OutputSpec.make(fr.FMT_RGB_F16_CHW, *fr.F16_TIES), jb.OutputSpec.make(fr.FMT_RGB_F16_CHW, *fr.UNIT)]


@pytest.mark.parametrize("huff", ["0", None])
def test_batch_decoder_formats_malloc_and_arena(jb, monkeypatch, mixed_files, huff):
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    with jb.BatchDecoder(4, 0) as dec:
        imgs0, st, tm = dec.run(mixed_files)                     # the same decoder's format-0 output
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
        for spec in _specs(jb) + [jb.OutputSpec.make(0)]:        # the format changes between runs of one decoder
            dec.set_output_format(spec)
            imgs, st, tm = dec.run(mixed_files)
            _check(imgs, st, tm, _refs(imgs0, spec))
        if huff is None:
            assert dec.device_entropy_images > 0
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F32_CHW)
    need = sum((f.nbytes * 4 + 255) // 256 * 256 for f in imgs0)
    with jb.BatchDecoder(4, 0, arena_bytes=need + 4096, fmt=spec) as dec:
        imgs, st, tm = dec.run(mixed_files)
        _check(imgs, st, tm, _refs(imgs0, spec))


def test_batch_decoder_formats_device_regions_and_two_devices(jb, mixed_files):
    import torch
    with jb.BatchDecoder(4, 0) as dec:
        imgs0, st, tm = dec.run(mixed_files)
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
        region = torch.zeros(96 << 20, dtype=torch.uint8, device="cuda:0")
        dec.set_device_output(region.data_ptr(), region.numel())
        for spec in _specs(jb):
            dec.set_output_format(spec)
            es = np.dtype(spec.dtype).itemsize
            ptrs, dims, st, tm = dec.run_to_device(mixed_files)
            torch.cuda.synchronize()
            assert tm["rc"] == 0 and all(s == 0 for s in st), tm
            for i, want in enumerate(_refs(imgs0, spec)):
                w, h = dims[i]
                assert (3, h, w) == want.shape
                assert ptrs[i] % es == 0, "device-region pointers are element-aligned"
                off = ptrs[i] - region.data_ptr()
                got = region[off:off + want.nbytes].cpu().numpy().view(spec.dtype).reshape(3, h, w)
                assert fr.same_bits(got, want), (spec.format, i)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(4, devices=[0, 0], fmt=spec) as dec:
        imgs, st, tm = dec.run(mixed_files)
        _check(imgs, st, tm, _refs(imgs0, spec))
        r0 = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda:0")
        r1 = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda:0")
        dec.set_device_outputs([(r0.data_ptr(), r0.numel()), (r1.data_ptr(), r1.numel())])
        ptrs, dims, st, tm = dec.run_to_device(mixed_files)
        torch.cuda.synchronize()
        assert tm["rc"] == 0 and all(s == 0 for s in st), tm
        for i, want in enumerate(_refs(imgs0, spec)):
            r = (r0, r1)[i % 2]
            assert ptrs[i] % 2 == 0
            off = ptrs[i] - r.data_ptr()
            got = r[off:off + want.nbytes].cpu().numpy().view(np.float16).reshape(want.shape)
            assert fr.same_bits(got, want), i


def test_batch_decoder_formats_submit_collect_and_refusals(jb, mixed_files):
    with jb.BatchDecoder(4, 0) as dec:
        imgs0, st, tm = dec.run(mixed_files)
        assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
        spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
        dec.set_output_format(spec)
        t0 = dec.submit(mixed_files)
        t1 = dec.submit(mixed_files[::-1])      # two in flight: the twin side is built here, in the same format
        with pytest.raises(jb.JbError) as e:
            dec.set_output_format(jb.OutputSpec.make(1))
        assert e.value.status == -7              # JB_ERR_STATE
        refs = _refs(imgs0, spec)
        imgs, st, tm = dec.collect(t0)
        _check(imgs, st, tm, refs)
        imgs, st, tm = dec.collect(t1)
        _check(imgs, st, tm, refs[::-1])
        spec = jb.OutputSpec.make(fr.FMT_RGB_F32_CHW, *fr.UNIT)
        dec.set_output_format(spec)              # reaches the twin as well
        t2 = dec.submit(mixed_files)
        t3 = dec.submit(mixed_files)
        for t in (t2, t3):
            imgs, st, tm = dec.collect(t)
            _check(imgs, st, tm, _refs(imgs0, spec))
        # a format and a scale exclude each other, whichever comes second; bad specs are refused
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(2)
        assert e.value.status == -9
        dec.set_output_format(0)
        dec.set_scale(2)
        for fmt in NEW_FORMATS:
            with pytest.raises(jb.JbError) as e:
                dec.set_output_format(fmt)
            assert e.value.status == -9
        dec.set_scale(1)
        for bad in (jb.OutputSpec.make(9), jb.OutputSpec.make(2, [float("nan")] * 3), jb.OutputSpec.make(1, plane_stride=4096)):
            with pytest.raises(jb.JbError) as e:
                dec.set_output_format(bad)
            assert e.value.status == -2
        with pytest.raises(jb.JbError) as e:
            jb.BatchDecoder(2, 0, scale=4, fmt=1)
        assert e.value.status == -9


def test_run_to_tensor(jb, tmp_path):
    import torch
    from jpeg_decoder_amd import synth
    w, h, n = 333, 211, 6
    paths = []
    for i in range(n):
        hs, vs = LAYOUTS[i % 4]
        coef, q = synth.synth_blocks(w, h, hs, vs, image_index=80 + i)
        p = str(tmp_path / f"t{i}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=0))
        paths.append(p)
    coef, q = synth.synth_blocks(100, 37, 1, 1, image_index=5)
    odd = str(tmp_path / "odd.jpg")
    with open(odd, "wb") as f:
        f.write(synth.encode_jpeg(coef, 100, 37, 1, 1, q, restart_interval=0))
    with jb.BatchDecoder(4, 0) as dec:
        imgs0, st, tm = dec.run(paths)
        assert tm["rc"] == 0 and all(s == 0 for s in st)
        for spec, tdt in ((jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW), torch.float16), (jb.OutputSpec.imagenet(fr.FMT_RGB_F32_CHW), torch.float32),
                          (jb.OutputSpec.make(fr.FMT_RGB_U8_CHW), torch.uint8)):
            dec.set_output_format(spec)
            out = torch.zeros((n, 3, h, w), dtype=tdt, device="cuda:0")
            ret, st, tm = dec.run_to_tensor(paths, out)
            assert ret is out and all(s == 0 for s in st), (st, tm)
            want = np.stack(_refs(imgs0, spec))
            assert fr.same_bits(out.cpu().numpy(), want), spec.format
            with pytest.raises(ValueError):
                dec.run_to_tensor(paths, torch.zeros((n, 3, h, w), dtype=torch.float64, device="cuda:0"))
        # a file of another size: an error for that image, the others are delivered
        mixed = paths[:2] + [odd] + paths[2:5]
        out = torch.full((n, 3, h, w), 7, dtype=torch.uint8, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(mixed, out)
        assert st[2] != 0 and [s for i, s in enumerate(st) if i != 2] == [0] * 5
        got = out.cpu().numpy()
        assert (got[2] == 7).all()
        for i, j in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4)):
            assert fr.same_bits(got[i], fr.to_format(imgs0[j], 1)), i
        # the decoder is back on host output
        imgs, st, tm = dec.run(paths)
        _check(imgs, st, tm, _refs(imgs0, jb.OutputSpec.make(1)))
