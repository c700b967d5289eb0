"""Scaled output on the GPU (-m gpu): every scaled entry point equals the area reduction (tests/area_reduce.py)
of the full-size output it is defined by -- the oracle's pixels at the seam, the reference's golden RGB for
decode(path), the library's own full-size decode on every other route.  Scale 1 through the new entry points is
byte-identical to the old ones."""
import os

import numpy as np
import pytest

from area_reduce import area_reduce
from conftest import BASELINE_IMAGES, GOLD, load_golden
from seam_harness import LAYOUTS, SEAM_SIZES, Seam, _oracle_full

pytestmark = pytest.mark.gpu


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
def test_seam_scaled_equals_area_reduced_oracle(jb, ctx, oracle, hs, vs, w, h):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=w + h)
    full = _oracle_full(oracle, w, h, hs, vs, coef, q)
    s = Seam(jb, w, h, hs, vs, [coef], [q])
    for k in (2, 4, 8):
        s.check(ctx, [area_reduce(full, k)], 0, scale=k, tag=(w, h, hs, vs))


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_scaled_batch_strides_dense_and_mixed_tables(jb, ctx, oracle, hs, vs):
    """3 images with padded row and image strides, full-range coefficients (clamps at 0 and 255), and
    different Cb / Cr tables (the MIXQ instantiation of 4:2:0)."""
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
    s = Seam(jb, w, h, hs, vs, coefs, qs, qid, pad_row=13, pad_img=77)
    for k in (2, 4, 8):
        s.check(ctx, [area_reduce(full, k) for full in fulls], 0, scale=k, tag=(hs, vs))


def test_seam_scale_one_is_the_full_size_seam(jb, ctx):
    from jpeg_decoder_amd import synth
    for hs, vs in LAYOUTS:
        coef, q = synth.synth_blocks(679, 451, hs, vs, image_index=5)
        b = ctx.blocks_to_rgb(jb.make_desc(679, 451, hs, vs), coef, q)
        Seam(jb, 679, 451, hs, vs, [coef], [q], pad_row=3).check(ctx, [b], 0, scale=1, tag=(hs, vs))


def test_seam_scaled_refusals(jb, ctx):
    import torch
    from jpeg_decoder_amd import synth
    w, h = 64, 64
    desc = jb.make_desc(w, h, 1, 1)
    coef, q = synth.synth_blocks(w, h, 1, 1)
    coef_t = torch.from_numpy(coef).to("cuda:0")
    q_t = torch.from_numpy(jb.resolve_qtabs(desc, q)).to("cuda:0")
    out = torch.zeros(3 * w * h, dtype=torch.uint8, device="cuda:0")
    b = jb.DeviceBatch()
    b.desc, b.n_images = desc, 1
    b.d_coef, b.coef_image_stride = coef_t.data_ptr(), coef.nbytes
    b.d_qtabs, b.d_rgb = q_t.data_ptr(), out.data_ptr()
    b.rgb_row_stride, b.rgb_image_stride = 3 * 32 - 1, 3 * 32 * 32  # one byte short of a row at 1/2
    for k, status in ((2, -2), (3, -2), (0, -2), (16, -2)):
        with pytest.raises(jb.JbError) as e:
            ctx.blocks_to_rgb_device(b, scale=k)
        assert e.value.status == status
    b.rgb_row_stride = 3 * 32
    ctx.blocks_to_rgb_device(b, scale=2)
    ctx.synchronize()


@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_decode_file_scaled_golden(jb, ctx, name):
    """decode_file(path, scale=K) == the area reduction of the reference's own RGB."""
    _, _, _, rgb = load_golden(name)
    path = os.path.join(GOLD, "images", name + ".jpg")
    assert np.array_equal(ctx.decode_file(path, scale=1), rgb)
    for k in (2, 4, 8):
        assert np.array_equal(ctx.decode_file(path, scale=k), area_reduce(rgb, k)), k


@pytest.mark.parametrize("huff", ["0", "2"])
def test_decode_memory_scaled_routes(jb, monkeypatch, tmp_path, huff):
    """Host (JPEGBLK_GPU_HUFFMAN=0) and device (=2) entropy paths, a baseline file of each layout, the bundled
    progressive sample and a grayscale file: decode_memory(scale=K) == area_reduce(decode_memory())."""
    Image = pytest.importorskip("PIL.Image")
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:301, 0:457]
    img = np.clip(np.stack([xx * 0.4 + yy * 0.3, 220 - yy * 0.5, (xx + yy) * 0.3 + 20], -1)
                  + rng.normal(0, 9, (301, 457, 3)), 0, 255).astype(np.uint8)
    blobs = []
    for sub in (0, 1, 2):
        p = tmp_path / f"s{sub}.jpg"
        Image.fromarray(img).save(p, "JPEG", quality=92, subsampling=sub)
        blobs.append(p.read_bytes())
    p = tmp_path / "g.jpg"
    Image.fromarray(img).convert("L").save(p, "JPEG", quality=90)
    blobs.append(p.read_bytes())
    prog = os.path.join(GOLD, "images", "prograssive-sample-2.jpg")
    if os.path.exists(prog):
        blobs.append(open(prog, "rb").read())
    blobs.append(open(os.path.join(GOLD, "images", "img4.jpg"), "rb").read())  # restart intervals
    with jb.Context(0) as c:
        for i, data in enumerate(blobs):
            full = c.decode_memory(data)
            assert np.array_equal(c.decode_memory(data, scale=1), full)
            for k in (2, 4, 8):
                assert np.array_equal(c.decode_memory(data, scale=k), area_reduce(full, k)), (huff, i, k)
        n_dev = c.device_entropy_images
    assert (n_dev > 0) == (huff == "2")


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    """Writer files of several sizes and samplings, with and without restart intervals, plus the bundled images."""
    from jpeg_decoder_amd import synth
    d = tmp_path_factory.mktemp("scaled")
    paths = []
    specs = [(640, 360, 2, 2, 10), (333, 211, 1, 1, 0), (1920, 1080, 1, 1, 240), (517, 300, 2, 1, 8), (250, 177, 1, 2, 0),
             (1, 1, 1, 1, 0), (7, 13, 2, 2, 0)]
    for j, (w, h, hs, vs, ri) in enumerate(specs):
        for r in range(2):
            coef, q = synth.synth_blocks(w, h, hs, vs, image_index=40 + 2 * j + r)
            p = os.path.join(str(d), f"m{j}_{r}.jpg")
            with open(p, "wb") as f:
                f.write(synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri))
            paths.append(p)
    paths += [os.path.join(GOLD, "images", n + ".jpg") for n in BASELINE_IMAGES]
    return paths


def _full_decodes(jb, paths):
    with jb.BatchDecoder(4, 0) as dec:
        imgs, st, tm = dec.run(paths)
    assert tm["rc"] == 0 and all(s == 0 for s in st), (tm, st)
    return imgs


def _check_scaled(imgs, st, tm, fulls, k):
    assert tm["rc"] == 0 and all(s == 0 for s in st), (tm["rc"], tm["error"], st)
    for i, (g, f) in enumerate(zip(imgs, fulls)):
        assert g is not None and np.array_equal(g, area_reduce(f, k)), (i, k)


@pytest.mark.parametrize("huff", ["0", None])
def test_batch_decoder_scaled_malloc_arena_and_scale_changes(jb, monkeypatch, mixed_files, huff):
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    fulls = _full_decodes(jb, mixed_files)
    with jb.BatchDecoder(4, 0) as dec:
        for k in (2, 8, 1, 4):  # the scale changes between runs of one decoder
            dec.set_scale(k)
            imgs, st, tm = dec.run(mixed_files)
            _check_scaled(imgs, st, tm, fulls, k)
    # an arena that holds the scaled images (each rounded up to 256 bytes) but not the full-size ones
    for k in (2, 4):
        need = sum(((-(-f.shape[0] // k)) * (-(-f.shape[1] // k)) * 3 + 255) // 256 * 256 for f in fulls)
        assert need < sum(f.nbytes for f in fulls)
        with jb.BatchDecoder(4, 0, arena_bytes=need + 4096, scale=k) as dec:
            imgs, st, tm = dec.run(mixed_files)
            _check_scaled(imgs, st, tm, fulls, k)
    imgs, st, tm = jb.decode_batch(mixed_files, n_threads=4, scale=8)
    _check_scaled(imgs, st, tm, fulls, 8)


def test_batch_decoder_scaled_device_output_and_two_devices(jb, mixed_files):
    import torch
    fulls = _full_decodes(jb, mixed_files)
    k = 2
    with jb.BatchDecoder(4, 0, scale=k) as dec:
        region = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda:0")
        dec.set_device_output(region.data_ptr(), region.numel())
        ptrs, dims, st, tm = dec.run_to_device(mixed_files)
        torch.cuda.synchronize()
        assert tm["rc"] == 0 and all(s == 0 for s in st), tm
        for i, f in enumerate(fulls):
            want = area_reduce(f, k)
            w, h = dims[i]
            assert (h, w) == want.shape[:2]
            off = ptrs[i] - region.data_ptr()
            got = region[off:off + w * h * 3].cpu().numpy().reshape(h, w, 3)
            assert np.array_equal(got, want), i
    with jb.BatchDecoder(4, devices=[0, 0]) as dec:
        dec.set_scale(4)
        imgs, st, tm = dec.run(mixed_files)
        _check_scaled(imgs, st, tm, fulls, 4)


def test_batch_decoder_scaled_submit_collect(jb, mixed_files):
    fulls = _full_decodes(jb, mixed_files)
    with jb.BatchDecoder(4, 0) as dec:
        dec.set_scale(2)
        t0 = dec.submit(mixed_files)
        t1 = dec.submit(mixed_files[::-1])      # two in flight: the twin side is built here, at the same scale
        with pytest.raises(jb.JbError) as e:
            dec.set_scale(4)
        assert e.value.status == -7              # JB_ERR_STATE
        imgs, st, tm = dec.collect(t0)
        _check_scaled(imgs, st, tm, fulls, 2)
        imgs, st, tm = dec.collect(t1)
        _check_scaled(imgs, st, tm, fulls[::-1], 2)
        dec.set_scale(8)
        t2 = dec.submit(mixed_files)
        t3 = dec.submit(mixed_files)
        for t in (t2, t3):
            imgs, st, tm = dec.collect(t)
            _check_scaled(imgs, st, tm, fulls, 8)
        with pytest.raises(jb.JbError):
            dec.set_scale(3)
