"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (libjpegblk.so), against
the oracle and the committed golden vectors.  Parity bar: BIT-EXACT (integer/byte outputs);
the +-1 LSB allowance of BASELINE.json is not used."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import BASELINE_IMAGES, GOLD, load_golden, load_kat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def big_ctx(jb):
    # big enough for every host-buffer case in this file (1279x885 4:2:0 is the largest golden)
    ctx = jb.Context(0, 64 << 20, 64 << 20, 3)
    yield ctx
    ctx.close()


def _same_desc(jb, d):
    return jb.make_desc(d.width, d.height, d.hs, d.vs, list(d.qtab_id))


@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_golden_images_host_api(jb, big_ctx, manifest, name):
    desc, coef, qtabs, rgb = load_golden(name)
    got = big_ctx.blocks_to_rgb(_same_desc(jb, desc), coef, qtabs)
    assert np.array_equal(got, rgb)
    assert hashlib.sha256(got.tobytes()).hexdigest() == manifest["images"][name]["rgb_sha256"]


def test_golden_kat_vectors(jb, big_ctx):
    for name, (desc, coef, qtabs, rgb) in load_kat().items():
        got = big_ctx.blocks_to_rgb(_same_desc(jb, desc), coef, qtabs)
        assert np.array_equal(got, rgb), name


@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_decode_file_matches_reference(jb, big_ctx, name):
    """decode(path) -> RGB: host front end + device block pipeline == the reference's output."""
    _, _, _, rgb = load_golden(name)
    got = big_ctx.decode_file(os.path.join(GOLD, "images", name + ".jpg"))
    assert np.array_equal(got, rgb)


def test_decode_file_progressive_and_grayscale(jb, big_ctx, oracle, tmp_path):
    """Beyond the reference (it rejects both, jpeg.cpp:69-87): decode(path) of progressive and of
    grayscale files equals the oracle's pixel path on the decoded blocks; a progressive file gives
    exactly the pixels of the baseline file of the same image; the reference's own bundled
    progressive sample decodes and stays close to libjpeg's decode."""
    pytest.importorskip("PIL")
    from PIL import Image
    from oracle.pyoracle import make_desc as odesc
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:301, 0:457]
    img = np.clip(np.stack([xx * 0.4 + yy * 0.3, 220 - yy * 0.5, (xx + yy) * 0.3 + 20], -1)
                  + rng.normal(0, 5, (301, 457, 3)), 0, 255).astype(np.uint8)
    for sub in (0, 2):
        pb, pp = tmp_path / f"b{sub}.jpg", tmp_path / f"p{sub}.jpg"
        Image.fromarray(img).save(pb, "JPEG", quality=90, subsampling=sub)
        Image.fromarray(img).save(pp, "JPEG", quality=90, subsampling=sub, progressive=True)
        base, prog = big_ctx.decode_file(str(pb)), big_ctx.decode_file(str(pp))
        assert np.array_equal(base, prog)
        desc, q, coef = jb.entropy_decode(pp.read_bytes())
        assert np.array_equal(prog, oracle.blocks_to_rgb(odesc(457, 301, desc.hs, desc.vs, list(desc.qtab_id)), coef, q))
    pg = tmp_path / "g.jpg"
    Image.fromarray(img).convert("L").save(pg, "JPEG", quality=90)
    gray = big_ctx.decode_file(str(pg))
    assert np.array_equal(gray[..., 0], gray[..., 1]) and np.array_equal(gray[..., 0], gray[..., 2])
    assert np.abs(gray[..., 0].astype(int) - np.asarray(Image.open(pg)).astype(int)).max() <= 3
    path = os.path.join(GOLD, "images", "prograssive-sample-2.jpg")
    got = big_ctx.decode_file(path)
    ref = np.asarray(Image.open(path).convert("RGB")).astype(int)
    assert got.shape == ref.shape and np.abs(got.astype(int) - ref).mean() < 2.5


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_sixteen_bit_quant_entries_vs_oracle(jb, big_ctx, oracle, hs, vs):
    """Quantisation entries of 256..65535 (Pq = 1 tables) through the fused kernel's 24-bit multiply, every layout,
    Cb and Cr on different tables (the MIXQ instantiation) and on one: bit-exact against the oracle's int32
    multiply.  PARITY WITH THE REFERENCE IS UNPINNED HERE: it keeps only the low byte of such entries
    (jpeg.cpp:216), so there is no reference behaviour to match; the products are kept inside the range where its
    float -> int conversions are defined (|coefficient x entry| <= 65535 per term)."""
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    rng = np.random.default_rng(16)
    q = np.zeros((4, 64), np.uint16)
    q[0] = rng.integers(256, 4000, 64)
    q[1] = rng.integers(256, 65536, 64)
    q[2] = 65535
    q[3] = rng.integers(1, 65536, 64)
    q[:, 0] = (300, 65535, 256, 1000)
    for i, (w, h) in enumerate([(8, 8), (333, 211), (640, 360)]):
        for qid in [(0, 1, 2), (3, 3, 3), (1, 2, 2)]:
            n = oracle.geometry(odesc(w, h, hs, vs, qid)).n_coded_blocks
            coef = np.zeros((n, 64), np.int16)
            mask = rng.random((n, 64)) < 0.2
            coef[mask] = rng.integers(-8, 9, int(mask.sum()))
            big = q[list(qid)].max(0) > 8000                    # positions where a table in use has a large entry:
            coef[:, big] = np.clip(coef[:, big], -1, 1)         # every term stays below 2^16
            got = big_ctx.blocks_to_rgb(jb.make_desc(w, h, hs, vs, qid), coef, q)
            want = oracle.blocks_to_rgb(odesc(w, h, hs, vs, qid), coef, q, nthreads=4)
            assert np.array_equal(got, want), (w, h, hs, vs, qid)
            assert got.min() < 40 and got.max() > 215   # the large entries do reach the pixels


def test_grayscale_file_matches_the_oracle_on_its_blocks(jb, oracle, tmp_path):
    """A single-component frame (rejected by the reference, jpeg.cpp:83-87) through decode(path): the pixels equal
    the oracle's pixel path on the blocks the front end delivers (Y blocks of a 4:4:4 frame, Cb = Cr = 0), for
    baseline and progressive encodings, with the entropy stage on the host and on the device."""
    pytest.importorskip("PIL")
    from PIL import Image
    from oracle.pyoracle import make_desc as odesc
    rng = np.random.default_rng(3)
    g = np.clip(np.cumsum(rng.normal(0, 6, (431, 613)), axis=1) + 120, 0, 255).astype(np.uint8)
    for kw in ({}, {"progressive": True}, {"restart_marker_blocks": 9}):
        p = tmp_path / "g.jpg"
        Image.fromarray(g).save(p, "JPEG", quality=91, **kw)
        desc, q, coef = jb.entropy_decode(p.read_bytes())
        want = oracle.blocks_to_rgb(odesc(613, 431, desc.hs, desc.vs, list(desc.qtab_id)), coef, q)
        for knob in ("0", "2"):
            os.environ["JPEGBLK_GPU_HUFFMAN"] = knob     # (read when a context is created)
            try:
                with jb.Context(0) as c:
                    got = c.decode_file(str(p))
                    took = c.device_entropy_images
            finally:
                os.environ.pop("JPEGBLK_GPU_HUFFMAN", None)
            assert np.array_equal(got, want), (kw, knob)
            assert took == (1 if knob == "2" and "progressive" not in kw else 0), (kw, knob)


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_random_blocks_vs_oracle_ragged_sizes(jb, big_ctx, oracle, hs, vs):
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    q = synth.annex_k_qtabs(50)
    q[2] = 255
    q[3] = np.arange(64, 0, -1)
    sizes = [(1, 1), (8, 8), (9, 7), (100, 52), (511, 17), (513, 33), (1030, 19), (1537, 40), (777, 555)]
    for i, (w, h) in enumerate(sizes):
        for qid in [(0, 1, 2), (3, 3, 0)]:
            n = oracle.geometry(odesc(w, h, hs, vs, qid)).n_coded_blocks
            coef = synth.random_blocks(n, 100 + i) if i % 2 else synth.random_blocks(n, 200 + i, -700, 700)
            got = big_ctx.blocks_to_rgb(jb.make_desc(w, h, hs, vs, qid), coef, q)
            want = oracle.blocks_to_rgb(odesc(w, h, hs, vs, qid), coef, q, nthreads=4)
            assert np.array_equal(got, want), (w, h, hs, vs, qid)


def test_row_stride_and_untouched_padding(jb, big_ctx, oracle):
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    w, h = 301, 77
    coef, q = synth.synth_blocks(w, h, 2, 2, 5)
    stride = 3 * w + 29
    out = np.full((h, stride), 0xAB, np.uint8)
    t = big_ctx.submit(jb.make_desc(w, h, 2, 2), coef, q, out, stride)
    big_ctx.wait(t)
    want = oracle.blocks_to_rgb(odesc(w, h, 2, 2), coef, q)
    assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), want)
    assert (out[:, 3 * w:] == 0xAB).all()


def test_async_ring_many_images(jb, oracle):
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    w, h = 640, 360
    desc = jb.make_desc(w, h, 1, 1)
    with jb.Context.for_image(desc, 0, n_slots=3) as ctx:
        ins, outs, tickets = [], [], []
        for i in range(10):
            coef, q = synth.synth_blocks(w, h, 1, 1, i)
            out = np.zeros((h, 3 * w), np.uint8)
            ins.append((coef, q))
            outs.append(out)
            tickets.append(ctx.submit(desc, coef, q, out))
        # only the last n_slots tickets are still waitable; earlier ones completed when their
        # slot was recycled
        assert isinstance(ctx.poll(tickets[-1]), bool)      # non-blocking: pending or done
        for t in tickets[-3:]:
            ctx.wait(t)
            assert ctx.poll(t) is True
        with pytest.raises(jb.JbError) as e:
            ctx.wait(tickets[0])
        assert e.value.status == -7
        for (coef, q), out in zip(ins, outs):
            assert np.array_equal(out.reshape(h, w, 3), oracle.blocks_to_rgb(odesc(w, h, 1, 1), coef, q))


def test_device_batch_api_per_image_tables(jb, oracle):
    """The device-resident entry point bench.py uses: a batch in one launch, torch tensors as
    plumbing, per-image quantisation tables."""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    w, h, hs, vs, nimg = 1000, 200, 2, 2, 5
    desc = jb.make_desc(w, h, hs, vs, (0, 1, 2))
    g = jb.geometry_of(desc)
    coefs, q3s, qs = [], [], []
    for i in range(nimg):
        q = synth.annex_k_qtabs(40 + 10 * i)
        q[2] = q[1][::-1]
        coef, _ = synth.synth_blocks(w, h, hs, vs, i, qtabs=q, qtab_id=(0, 1, 2))
        coefs.append(coef)
        qs.append(q)
        q3s.append(jb.resolve_qtabs(desc, q))
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)  # an explicit stream: a NULL handle would mean the ctx's own stream
    stride = 3 * w + 4
    with torch.cuda.stream(ts), jb.Context(0) as ctx:
        coef_t = torch.from_numpy(np.stack(coefs)).to(dev)
        q_t = torch.from_numpy(np.stack(q3s)).to(dev)
        rgb_t = torch.zeros((nimg, h, stride), dtype=torch.uint8, device=dev)
        b = torch_batch(desc, nimg, coef_t, q_t, rgb_t, shared_qtabs=False)
        ctx.blocks_to_rgb_device(b, ts.cuda_stream)
        torch.cuda.synchronize()
    got = rgb_t.cpu().numpy()
    for i in range(nimg):
        want = oracle.blocks_to_rgb(odesc(w, h, hs, vs, (0, 1, 2)), coefs[i], qs[i], nthreads=4)
        assert np.array_equal(got[i, :, :3 * w].reshape(h, w, 3), want), i
    assert (got[:, :, 3 * w:] == 0).all()
    assert g.n_coded_blocks == coefs[0].shape[0]


@pytest.mark.parametrize("byte_store", [False, True])
@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_unaligned_output_both_store_paths(jb, oracle, monkeypatch, hs, vs, byte_store):
    """rgb pointer / stride not multiples of 4 (odd widths with tightly packed rows are the common
    case): the default path stores 12 bytes per lane at byte-aligned addresses, JPEGBLK_BYTE_STORE=1
    selects the byte-store path.  Both must be exact and must not touch a byte outside the rows.
    (The staged, line-aligned store stage -- a measured variant that only exists in -DJB_LAB builds of the kernels --
    went through this same test, 3 x 4 samplings green, before it was taken out of the product:
    profiles/r03/staged_store_parity.txt; profiles/r03/probe_staged.py compares its bytes with the product path's.)"""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    monkeypatch.setenv("JPEGBLK_SMALL_GRID", "0")      # (the 192-lane kernel's store paths are what this test is about)
    if byte_store is True:
        monkeypatch.setenv("JPEGBLK_BYTE_STORE", "1")
    else:
        monkeypatch.delenv("JPEGBLK_BYTE_STORE", raising=False)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)
    # (260 / 300 wide: a tile of 64 / 32 MCUs spans three MCU rows; 1024 wide with a 64-byte-aligned row: no byte runs at all)
    for (w, h, pad, off) in [(333, 41, 2, 1), (679, 451, 0, 3), (1921, 37, 1, 2), (515, 16, 0, 1), (260, 50, 0, 5), (300, 70, 61, 63),
                             (1040, 33, 16, 0)]:
        desc = jb.make_desc(w, h, hs, vs)
        coef, q = synth.synth_blocks(w, h, hs, vs, 9)
        stride = 3 * w + pad
        with torch.cuda.stream(ts), jb.Context(0) as ctx:
            coef_t = torch.from_numpy(coef).to(dev)
            q_t = torch.from_numpy(jb.resolve_qtabs(desc, q)).to(dev)
            raw = torch.full((h * stride + 80,), 0xC5, dtype=torch.uint8, device=dev)
            view = raw[off:off + h * stride].view(1, h, stride)
            b = torch_batch(desc, 1, coef_t.view(1, -1, 64), q_t, view)
            ctx.blocks_to_rgb_device(b, ts.cuda_stream)
            torch.cuda.synchronize()
        host = raw.cpu().numpy()
        rows = host[off:off + h * stride].reshape(h, stride)
        want = oracle.blocks_to_rgb(odesc(w, h, hs, vs), coef, q, nthreads=4)
        assert np.array_equal(rows[:, :3 * w].reshape(h, w, 3), want), (w, h, hs, vs, byte_store)
        assert (rows[:, 3 * w:] == 0xC5).all() and (host[:off] == 0xC5).all() and (host[off + h * stride:] == 0xC5).all()


@pytest.mark.parametrize("w,h,hs,vs", [(4096, 4096, 1, 1), (4096, 4096, 2, 2), (1920, 1080, 1, 1), (8192, 8192, 2, 2)])
def test_full_size_configs_vs_oracle_and_properties(jb, oracle, w, h, hs, vs):
    """BASELINE.json's single-GPU configurations at full size: bit-exact against the
    (multi-threaded) oracle, plus two size-independent properties of the path:
    MCU-permutation equivariance (blocks are independent) and idempotence of a
    repeated launch."""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    desc = jb.make_desc(w, h, hs, vs)
    g = jb.geometry_of(desc)
    coef, q = synth.synth_blocks(w, h, hs, vs, 1)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)
    with torch.cuda.stream(ts), jb.Context(0) as ctx:
        coef_t = torch.from_numpy(coef).to(dev).view(1, -1, 64)
        q_t = torch.from_numpy(jb.resolve_qtabs(desc, q)).to(dev)
        rgb_t = torch.zeros((1, h, 3 * w), dtype=torch.uint8, device=dev)
        s = ts.cuda_stream
        ctx.blocks_to_rgb_device(torch_batch(desc, 1, coef_t, q_t, rgb_t), s)
        torch.cuda.synchronize()
        got = rgb_t.cpu().numpy()[0].reshape(h, w, 3)
        want = oracle.blocks_to_rgb(odesc(w, h, hs, vs), coef, q, nthreads=16)
        assert np.array_equal(got, want)
        # idempotence: same launch again into the same buffer
        ctx.blocks_to_rgb_device(torch_batch(desc, 1, coef_t, q_t, rgb_t), s)
        torch.cuda.synchronize()
        assert np.array_equal(rgb_t.cpu().numpy()[0].reshape(h, w, 3), got)
        # equivariance: reverse the MCU order -> the image is the MCU-wise mirror
        bpm = g.blocks_per_mcu
        mc = coef_t.view(g.mcus_y, g.mcus_x, bpm, 64)
        flipped = torch.flip(mc, dims=(0, 1)).contiguous().view(1, -1, 64)
        rgb2 = torch.zeros_like(rgb_t)
        ctx.blocks_to_rgb_device(torch_batch(desc, 1, flipped, q_t, rgb2), s)
        torch.cuda.synchronize()
        mw, mh = 8 * hs, 8 * vs
        a = rgb_t.view(g.mcus_y, mh, g.mcus_x, mw, 3)
        b = torch.flip(rgb2.view(g.mcus_y, mh, g.mcus_x, mw, 3), dims=(0, 2))
        assert torch.equal(a, b)


def test_error_codes_no_exit(jb):
    """Every reference exit(1) path on this seam is a returned status here."""
    with jb.Context(0, 1 << 20, 1 << 20, 1) as ctx:
        coef = np.zeros((4, 64), np.int16)
        q = np.ones((4, 64), np.uint16)
        for desc, status in [(jb.make_desc(8, 8, 3, 1), -3), (jb.make_desc(8, 8, 1, 1, (0, 5, 1)), -4),
                             (jb.make_desc(0, 8, 1, 1), -2), (jb.make_desc(4096, 4096, 1, 1), -5)]:
            with pytest.raises(jb.JbError) as e:
                ctx.blocks_to_rgb(desc, coef, q)
            assert e.value.status == status
        assert jb.lib().jb_blocks_to_rgb(ctx._h, None, None, None, None, 0) == -1
    with pytest.raises(jb.JbError) as e:
        jb.Context(99)
    assert e.value.status == -6


def test_decode_batch_threads_and_failures(jb, tmp_path):
    """Multi-threaded decode(path) over a batch: host Huffman on several threads overlapped with
    the device stage; a rejected file in the middle is reported per file, the rest decode."""
    names = BASELINE_IMAGES * 3
    paths = [os.path.join(GOLD, "images", n + ".jpg") for n in names]
    # an unsupported frame in the middle: four components (patched Nf of a good file)
    good = bytearray(open(paths[0], "rb").read())
    good[good.index(b"\xff\xc0") + 9] = 4
    (tmp_path / "four.jpg").write_bytes(bytes(good))
    paths.insert(4, str(tmp_path / "four.jpg"))
    paths.insert(9, str(tmp_path / "missing.jpg"))
    imgs, statuses, times = jb.decode_batch(paths, n_threads=4)
    assert times["rc"] == -9 or times["rc"] == -8
    k = 0
    for i, p in enumerate(paths):
        if i == 4:
            assert statuses[i] == -9 and imgs[i] is None
        elif i == 9:
            assert statuses[i] == -8 and imgs[i] is None
        else:
            _, _, _, rgb = load_golden(names[k])
            assert statuses[i] == 0 and np.array_equal(imgs[i], rgb), p
            k += 1
    # single thread, clean batch
    imgs, statuses, times = jb.decode_batch(paths[:4], n_threads=1)
    assert times["rc"] == 0 and all(s == 0 for s in statuses)


def test_decode_pil_files_all_layouts_with_restarts(jb, big_ctx, oracle, tmp_path):
    """decode(path) on encoder-made files the reference has no fixtures for (4:2:2, 4:2:0 and
    4:4:4 with restart intervals): front end + device seam == oracle on the decoded blocks."""
    pytest.importorskip("PIL")
    from PIL import Image
    from oracle.pyoracle import make_desc as odesc
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:211, 0:333]
    img = np.clip(np.stack([xx * 0.6 + yy * 0.2, 200 - yy * 0.7, (xx + yy) * 0.35 + 30], -1)
                  + rng.normal(0, 2, (211, 333, 3)), 0, 255).astype(np.uint8)
    for sub in (0, 1, 2):
        for restart in (0, 7):
            p = tmp_path / f"s{sub}_r{restart}.jpg"
            kw = {"restart_marker_blocks": restart} if restart else {}
            Image.fromarray(img).save(p, "JPEG", quality=92, subsampling=sub, optimize=False, **kw)
            desc, q, coef = jb.entropy_decode(p.read_bytes())
            want = oracle.blocks_to_rgb(odesc(desc.width, desc.height, desc.hs, desc.vs, list(desc.qtab_id)), coef, q)
            got = big_ctx.decode_file(str(p))
            assert np.array_equal(got, want), (sub, restart)
            # sanity: the picture is recognisably the input (the reference's IDCT is not the
            # encoder's inverse to the last bit, so only a loose bound)
            assert np.abs(got.astype(int) - img.astype(int)).mean() < 8


def test_batch_of_1080p_images_one_launch(jb, oracle):
    """BASELINE config 4 shape (a GPU's share of a batch of 1920x1080 4:4:4 images) through the
    batched device entry point: every image of the launch against the oracle."""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    w, h, nimg = 1920, 1080, 6
    desc = jb.make_desc(w, h, 1, 1)
    coefs = [synth.synth_blocks(w, h, 1, 1, i)[0] for i in range(nimg)]
    q = synth.annex_k_qtabs(90)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)
    with torch.cuda.stream(ts), jb.Context(0) as ctx:
        coef_t = torch.from_numpy(np.stack(coefs)).to(dev)
        q_t = torch.from_numpy(jb.resolve_qtabs(desc, q)).to(dev)
        rgb_t = torch.zeros((nimg, h, 3 * w), dtype=torch.uint8, device=dev)
        ctx.blocks_to_rgb_device(torch_batch(desc, nimg, coef_t, q_t, rgb_t), ts.cuda_stream)
        torch.cuda.synchronize()
    got = rgb_t.cpu().numpy()
    for i in range(nimg):
        want = oracle.blocks_to_rgb(odesc(w, h, 1, 1), coefs[i], q, nthreads=16)
        assert np.array_equal(got[i].reshape(h, w, 3), want), i


@pytest.mark.parametrize("w,h,hs,vs,ri", [(1920, 1080, 1, 1, 0), (4096, 4096, 2, 2, 256), (8192, 8192, 2, 2, 0),
                                           (679, 451, 2, 2, 5), (1000, 700, 2, 1, 0), (1000, 700, 1, 2, 63)])
def test_stream_round_trip_full_sizes(jb, oracle, w, h, hs, vs, ri):
    """decode(bytes) at BASELINE's sizes (configs 2, 3, 5) with the build's own baseline writer:
    blocks -> JFIF stream -> jb_decode_memory (host Huffman + device seam) must equal the oracle
    on the blocks that were written -- the whole surface, no fixture size limit."""
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    coef, q = synth.synth_blocks(w, h, hs, vs, 77)
    data = synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri)
    desc = jb.make_desc(w, h, hs, vs)
    with jb.Context.for_image(desc, 0, n_slots=1) as ctx:
        got = ctx.decode_memory(data)
    want = oracle.blocks_to_rgb(odesc(w, h, hs, vs), coef, q, nthreads=16)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_batch_decoder_output_arena(jb, tmp_path):
    """jb_batch_decoder_set_arena: images land in the decoder's pinned arena (no per-image
    allocation or host copy); same pixels as the default malloc path; an arena that is too small
    fails the images that do not fit with JB_ERR_CAPACITY and decodes the rest."""
    import ctypes
    names = BASELINE_IMAGES * 2
    paths = [os.path.join(GOLD, "images", n + ".jpg") for n in names]
    want = [load_golden(n)[3] for n in names]
    total = sum((w.size + 255) // 256 * 256 for w in want)
    with jb.BatchDecoder(3, 0, arena_bytes=total) as dec:
        for _ in range(2):      # the arena is recycled by every run
            imgs, st, tm = dec.run(paths)
            assert tm["rc"] == 0 and all(x == 0 for x in st)
            for got, w in zip(imgs, want):
                assert np.array_equal(got, w)
    small = total - 256
    with jb.BatchDecoder(2, 0, arena_bytes=small) as dec:
        imgs, st, tm = dec.run(paths)
        assert tm["rc"] == -5 and sorted(set(st)) == [-5, 0] and st.count(-5) >= 1
        for got, w, x in zip(imgs, want, st):
            assert (got is None) if x else np.array_equal(got, w)
    imgs, st, tm = jb.decode_batch(paths, n_threads=3)      # default path, for comparison
    assert tm["rc"] == 0 and all(np.array_equal(g, w) for g, w in zip(imgs, want))


def test_randomised_soak_short():
    """tools/stress.py for a few seconds: random sizes, layouts, tables, coefficient statistics,
    batch sizes, output strides and byte offsets against the oracle, with guard bytes around
    every image (a 240-second run of the final kernels -- 13,473 launches, 10.6 Gpixels -- was clean)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(GOLD), "..", "tools", "stress.py"), "--seconds", "8", "--seed", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stress ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_cpp_image_mirror_cli(tmp_path):
    """include/jpegblk.hpp mirrors the reference's `Image` class (Image(path); readJPEG();
    saveToBMP()): tools/decode_cli.cpp is the reference's main() (jpeg.cpp:916-929) written against
    it.  Its PPM and BMP outputs must hold exactly the golden pixels; a rejected file exits 1
    with the reference's "-> ERROR" style message."""
    import subprocess
    pytest.importorskip("PIL")
    from PIL import Image
    root = os.path.dirname(os.path.dirname(GOLD))
    cli = os.path.join(root, "tools", "decode_cli")
    if not os.path.exists(cli):
        b = subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "tools", "decode_cli.cpp"),
                            "-L" + os.path.join(root, "jpeg_decoder_amd"), "-ljpegblk",
                            "-Wl,-rpath," + os.path.join(root, "jpeg_decoder_amd"), "-o", cli], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-2000:]
    src = os.path.join(GOLD, "images", "img.jpg")
    _, _, _, want = load_golden("img")
    for ext in ("ppm", "bmp"):
        out = tmp_path / f"o.{ext}"
        r = subprocess.run([cli, src, str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{want.shape[1]}x{want.shape[0]}" in r.stdout
        assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), want)
    bad = tmp_path / "bad.jpg"
    bad.write_bytes(b"not a jpeg")
    r = subprocess.run([cli, str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "ERROR" in r.stderr


@pytest.mark.parametrize("w,h,hs,vs", [(679, 451, 2, 2), (97, 61, 1, 1), (333, 100, 2, 1)])
def test_submit_batch_small_images(jb, oracle, w, h, hs, vs):
    """jb_submit_batch: several small images of one geometry, each with its own tables, in one
    upload + one launch + one download; every image against the oracle; capacity and count
    limits come back as statuses."""
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    n = 7
    qid = (0, 1, 2)
    desc = jb.make_desc(w, h, hs, vs, qid)
    g = jb.geometry_of(desc)
    coefs, qs = [], []
    for i in range(n):
        q = synth.annex_k_qtabs(35 + 9 * i)
        q[2] = q[1][::-1]
        coefs.append(synth.synth_blocks(w, h, hs, vs, i, qtabs=q, qtab_id=qid)[0])
        qs.append(q)
    coef, q = np.ascontiguousarray(np.stack(coefs)), np.ascontiguousarray(np.stack(qs))
    out = np.zeros((n, h, 3 * w), np.uint8)
    with jb.Context(0, n * g.coef_bytes, n * g.rgb_bytes, 2) as ctx:
        t = ctx.submit_batch(desc, coef, q, out)
        ctx.wait(t)
        for i in range(n):
            assert np.array_equal(out[i].reshape(h, w, 3), oracle.blocks_to_rgb(odesc(w, h, hs, vs, qid), coefs[i], qs[i])), i
        # one image more than the context was sized for
        big = np.ascontiguousarray(np.concatenate([coef, coef[:1]]))
        with pytest.raises(jb.JbError) as e:
            ctx.submit_batch(desc, big, np.ascontiguousarray(np.concatenate([q, q[:1]])), np.zeros((n + 1, h, 3 * w), np.uint8))
        assert e.value.status == -5


def test_huge_image_offsets_beyond_2_31(jb, oracle):
    """One 32768x24576 4:2:0 image: 2.4 GB of coefficients and 2.4 GB of pixels, so every byte
    offset inside the image passes 2^31 -- full output against the oracle."""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    w, h, hs, vs = 32768, 24576, 2, 2
    desc = jb.make_desc(w, h, hs, vs)
    g = jb.geometry_of(desc)
    assert g.coef_bytes > 2 ** 31 and g.rgb_bytes > 2 ** 31
    q = synth.annex_k_qtabs(80)
    pattern = synth.random_blocks(1_000_003, 12, -200, 200)      # a prime count: no alignment with MCU rows
    coef = np.resize(pattern, (g.n_coded_blocks, 64))
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)
    with torch.cuda.stream(ts), jb.Context(0) as ctx:
        coef_t = torch.from_numpy(coef).to(dev).view(1, -1, 64)
        q_t = torch.from_numpy(jb.resolve_qtabs(desc, q)).to(dev)
        rgb_t = torch.zeros((1, h, 3 * w), dtype=torch.uint8, device=dev)
        ctx.blocks_to_rgb_device(torch_batch(desc, 1, coef_t, q_t, rgb_t), ts.cuda_stream)
        torch.cuda.synchronize()
        got = rgb_t.cpu().numpy()[0].reshape(h, w, 3)
    del coef_t, rgb_t
    want = oracle.blocks_to_rgb(odesc(w, h, hs, vs), coef, q, nthreads=16)
    assert np.array_equal(got, want)


def test_contexts_on_concurrent_host_threads(jb, oracle):
    """SURVEY 8b threading contract: thread-safe per context handle -- four host threads, each
    with its own context (its own streams and staging ring) on the same GPU, decode different
    images concurrently; every result against the oracle."""
    import threading
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc as odesc
    shapes = [(640, 360, 1, 1), (679, 451, 2, 2), (1000, 300, 2, 1), (333, 777, 1, 2)]
    inputs = [synth.synth_blocks(w, h, hs, vs, 50 + i) for i, (w, h, hs, vs) in enumerate(shapes)]
    wants = [oracle.blocks_to_rgb(odesc(w, h, hs, vs), c, q, nthreads=4) for (w, h, hs, vs), (c, q) in zip(shapes, inputs)]
    errors = []

    def work(i):
        try:
            w, h, hs, vs = shapes[i]
            desc = jb.make_desc(w, h, hs, vs)
            coef, q = inputs[i]
            with jb.Context.for_image(desc, 0, n_slots=2) as ctx:
                for rep in range(25):
                    if rep % 2:
                        got = ctx.blocks_to_rgb(desc, coef, q)
                    else:
                        out = np.zeros((h, 3 * w), np.uint8)
                        ctx.wait(ctx.submit(desc, coef, q, out))
                        got = out.reshape(h, w, 3)
                    if not np.array_equal(got, wants[i]):
                        errors.append((i, rep))
                        return
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_reference_with_the_integration_patch(tmp_path, name):
    """The drop-in itself: the genuine reference (its own marker parser and Huffman decoder,
    compiled from where it lies by oracle/make_patched_ref.py) with the patch of INTEGRATION.md
    section 2 in place of dequantize(); inverseDCT(); YCbCrToRGB(); (jpeg.cpp:786-788) must
    produce the golden pixels through libjpegblk.so."""
    import subprocess
    root = os.path.dirname(os.path.dirname(GOLD))
    exe = os.path.join(root, "oracle", "_ref", "jpeg_patched")
    if not os.path.exists(exe):
        # loud, not a silent skip: a run without the genuine-reference build has NOT proven the drop-in
        pytest.xfail("oracle/_ref/jpeg_patched is absent (it is built from /root/reference by __graft_entry__.build(), "
                     "is git-ignored and travels with gpurun): the integration patch was NOT exercised in this run")
    pytest.importorskip("PIL")
    from PIL import Image
    out = tmp_path / "o.ppm"
    env = dict(os.environ, JB_DUMP=str(out))
    env.pop("DISPLAY", None)   # the reference's X11 sink fails headless and the program still exits 0
    r = subprocess.run([exe, os.path.join(GOLD, "images", name + ".jpg")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    _, _, _, want = load_golden(name)
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB")), want)


@pytest.mark.parametrize("byte_store", [False, True])
@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 2), (2, 1), (1, 2)])
def test_small_grid_kernels_vs_oracle(jb, oracle, monkeypatch, byte_store, hs, vs):
    """jb_small_kernel_444 / _420 / _16<2,1> / _16<1,2> (JPEGBLK_SMALL_GRID=1: one wave per 16 / 8 / 16 / 16 MCUs, four
    entry points of one body, jb_small_body<HS, VS>; the variants for launches that do not fill the device) against the oracle: sizes whose last tile of a row is ragged (1..15 MCUs), odd widths with tight rows and
    padded, misaligned rows, one pixel, a batch of images with per-image tables, 16-bit table entries, and the
    1080p frame of BASELINE.json's config 2 -- with guard bytes around every image, both store paths.  The same
    inputs through the default kernel must give the same bytes (JPEGBLK_SMALL_GRID=0)."""
    import torch
    from jpeg_decoder_amd import synth
    from jpeg_decoder_amd.api import torch_batch
    from oracle.pyoracle import make_desc as odesc
    if byte_store:
        monkeypatch.setenv("JPEGBLK_BYTE_STORE", "1")
    else:
        monkeypatch.delenv("JPEGBLK_BYTE_STORE", raising=False)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(dev)
    cases = [(1, 1, 0, 0, 1), (8, 8, 0, 1, 1), (127, 9, 2, 1, 3), (128, 16, 0, 0, 2), (129, 17, 1, 3, 1), (333, 41, 0, 1, 2),
             (679, 451, 0, 3, 1), (1921, 37, 5, 2, 1), (1920, 1080, 0, 0, 1), (2048, 24, 0, 0, 4), (1279, 853, 0, 1, 1), (16, 16, 0, 0, 1),
             (257, 17, 1, 1, 1)]   # 33 / 17 / 17 / 33 MCUs per row: the last workgroup of a row holds ONE MCU in every layout
    for (w, h, pad, off, n) in cases:
        desc = jb.make_desc(w, h, hs, vs)
        stride = 3 * w + pad
        per = h * stride + 32
        coefs, qs, wants = [], [], []
        for i in range(n):
            coef, q = synth.synth_blocks(w, h, hs, vs, 40 + i)
            if i == 1:
                q = (q.astype(np.int64) * 97 % 4000 + 1).astype(q.dtype)   # another table per image, entries above 255
            coefs.append(coef), qs.append(jb.resolve_qtabs(desc, q))
            wants.append(oracle.blocks_to_rgb(odesc(w, h, hs, vs), coef, q, nthreads=8))
        results = {}
        for knob in ("1", "0"):
            monkeypatch.setenv("JPEGBLK_SMALL_GRID", knob)
            with torch.cuda.stream(ts), jb.Context(0) as ctx:
                coef_t = torch.from_numpy(np.stack(coefs)).to(dev)
                q_t = torch.from_numpy(np.stack(qs)).to(dev)
                raw = torch.full((n * per + 16,), 0xC5, dtype=torch.uint8, device=dev)
                view = raw[off:off + n * per].view(n, per)[:, :h * stride].view(n, h, stride)
                b = torch_batch(desc, n, coef_t, q_t, view, shared_qtabs=False)
                ctx.blocks_to_rgb_device(b, ts.cuda_stream)
                torch.cuda.synchronize()
            results[knob] = raw.cpu().numpy()
        host = results["1"]
        assert np.array_equal(host, results["0"]), (w, h, "small-grid and default kernels differ")
        assert (host[:off] == 0xC5).all()
        for i in range(n):
            img = host[off + i * per: off + (i + 1) * per]
            rows = img[:h * stride].reshape(h, stride)
            assert np.array_equal(rows[:, :3 * w].reshape(h, w, 3), wants[i]), (w, h, i, byte_store)
            assert (rows[:, 3 * w:] == 0xC5).all() and (img[h * stride:] == 0xC5).all(), (w, h, i)
