"""The entropy stage on the device (-m gpu) on Huffman tables that are not Annex K's: the table shapes of
tests/huff_tables.py -- codes on both sides of the 10-bit first level, a second-level pool filled to its last table, the
27-bit DC symbol, flat and reversed tables on which lanes fall into step slowest -- decoded by jb_huff.hip on the MI355X,
where the bit-field instructions of the step (alignbit, ubfe, sbfe) are the hardware's and not the emulator's C.  Every
comparison is integer-exact: against the blocks the writer was given, against the host decoder, against the oracle's
pixels.  No family that fits the pool may be flagged: a "not in step" here is a finding, not a skip.  The same cases run
on the emulated kernels in tests/test_huff_tables_cpu.py."""
import io

import numpy as np
import pytest

import huff_tables as ht
from test_huff_emu import three_table_variant

pytestmark = pytest.mark.gpu

W, H = 200, 120
VARIANTS = [(n, False) for n in ht.TAKEN] + [(n, True) for n in ht.THREE_TABLES]
VARIANT_IDS = [n + ("-three" if t else "") for n, t in VARIANTS]


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(params=["128", "64"])
def dri_mode(request, monkeypatch):
    """Both chunk sizes of the device decoder (a context reads JPEGBLK_CHUNK_BYTES when it is created)."""
    monkeypatch.setenv("JPEGBLK_CHUNK_BYTES", request.param)
    return request.param


@pytest.fixture
def dctx(jb, dri_mode):
    c = jb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def content():
    """The two kinds of content per layout, made once: {(hs, vs): {"synth" | "full": (coef, qtabs)}}."""
    return {lay: ht.contents(W, H, *lay) for lay in ((1, 1), (2, 1), (1, 2), (2, 2))}


def encode(name, three, coef, w, h, hs, vs, q, ri=0):
    from jpeg_decoder_amd import synth
    data = synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri, huffman=ht.family(name))
    return three_table_variant(data) if three else data


# ---- a. direct device decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,three", VARIANTS, ids=VARIANT_IDS)
def test_device_decodes_every_taken_family(jb, dctx, content, name, three):
    """entropy_decode_device == the blocks written: 4:4:4 and 4:2:0, without restart intervals (the self-synchronising
    passes) and with intervals of 5 MCUs, ordinary and full-alphabet content."""
    for (hs, vs) in ((1, 1), (2, 2)):
        for ri in (0, 5):
            for kind, (coef, q) in content[(hs, vs)].items():
                d, _, c = dctx.entropy_decode_device(encode(name, three, coef, W, H, hs, vs, q, ri))
                assert (d.width, d.height, d.hs, d.vs) == (W, H, hs, vs)
                assert np.array_equal(c, coef), (hs, vs, ri, kind)


@pytest.mark.parametrize("name", ["flat", "all16"])
def test_device_decodes_a_large_full_alphabet_frame(jb, dctx, name):
    """640 x 480 4:4:4, full-alphabet content, no restart intervals: thousands of chunks in many workgroups, blocks longer
    than a chunk; under all16 nearly every symbol is 17 to 26 bits wide (a 16-bit code and its magnitude bits)."""
    from jpeg_decoder_amd import synth
    coef = ht.full_alphabet_blocks(640, 480, 1, 1, 31)
    data = encode(name, False, coef, 640, 480, 1, 1, synth.annex_k_qtabs(75))
    assert np.array_equal(dctx.entropy_decode_device(data)[2], coef)


def test_device_decodes_dense_content_without_any_block_end(jb, dctx):
    """Every coefficient +1 or -1: no EOB, and under `flat` every AC symbol is 9 bits -- nothing in the bits tells a lane
    where a block starts."""
    from jpeg_decoder_amd import synth
    coef = ht.dense_pm1_blocks(W, H, 1, 1, 3)
    for name in ("flat", "complete_allones", "all16"):
        data = encode(name, False, coef, W, H, 1, 1, synth.annex_k_qtabs(90))
        assert np.array_equal(dctx.entropy_decode_device(data)[2], coef), name


# ---- b. sets beyond the pool ------------------------------------------------------------------------------------------------
def test_sets_beyond_the_pool_go_to_the_host_decoder(jb, oracle, content, monkeypatch):
    """pool25 and pool_shared need 25 second-level tables: the device decoder refuses them with JB_ERR_UNSUPPORTED, and
    decode(bytes) with the device entropy stage forced (JPEGBLK_GPU_HUFFMAN=2) still gives the oracle's pixels for the
    blocks written -- through the host decoder, as its counter says; pool24 fits, and counts."""
    from oracle.pyoracle import make_desc as odesc
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "2")
    monkeypatch.delenv("JPEGBLK_CHUNK_BYTES", raising=False)
    with jb.Context(0) as c:
        for (hs, vs) in ((1, 1), (2, 2)):
            coef, q = content[(hs, vs)]["synth"]
            want = oracle.blocks_to_rgb(odesc(W, H, hs, vs), coef, q)
            for name in ht.REFUSED + ("pool24",):
                data = encode(name, False, coef, W, H, hs, vs, q)
                before = c.device_entropy_images
                if name in ht.REFUSED:
                    with pytest.raises(jb.JbError) as e:
                        c.entropy_decode_device(data)
                    assert e.value.status == -9, (name, e.value)
                else:
                    assert np.array_equal(c.entropy_decode_device(data)[2], coef)
                assert c.device_entropy_images == before
                assert np.array_equal(c.decode_memory(data), want), (name, hs, vs)
                assert c.device_entropy_images - before == (0 if name in ht.REFUSED else 1), (name, hs, vs)


# ---- c. several table sets in one launch -----------------------------------------------------------------------------------
def test_batch_with_several_table_sets_in_one_launch(jb, content, tmp_path, monkeypatch):
    """One BatchDecoder call, entropy stage on the device, over files of six families at mixed layouts (two, four and six
    first-level tables, 0 to 24 second-level tables), a grayscale libjpeg file and an Annex-K file: LDS is sized by the
    largest set of the launch and the second level starts elsewhere for every image.  Every image == the single-image
    decode with the entropy stage on the host, bit for bit; every file but the pool25 one is counted as device-decoded,
    and that one falls back alone."""
    pytest.importorskip("PIL")
    from PIL import Image
    from jpeg_decoder_amd import synth
    files = {}
    for (name, three, hs, vs, ri, kind) in [("flat", False, 1, 1, 0, "full"), ("pool24", False, 2, 2, 0, "synth"), ("all16", True, 2, 1, 5, "synth"),
                                            ("pool25", False, 1, 1, 0, "synth"), ("t1_split", False, 1, 2, 0, "full"),
                                            ("annexk_reversed", True, 2, 2, 0, "synth"), ("unary_dc_long", False, 1, 1, 5, "full")]:
        coef, q = content[(hs, vs)][kind]
        files[f"{name}_{hs}{vs}"] = encode(name, three, coef, W, H, hs, vs, q, ri)
    g = np.clip(np.cumsum(np.random.default_rng(4).normal(0, 5, (H, W)), axis=1) + 128, 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(g).save(b, "JPEG", quality=88)
    files["gray"] = b.getvalue()
    coef, q = content[(2, 1)]["synth"]
    files["annexk"] = synth.encode_jpeg(coef, W, H, 2, 1, q)
    order = ["flat_11", "gray", "pool24_22", "all16_21", "pool25_11", "annexk", "t1_split_12", "annexk_reversed_22", "unary_dc_long_11"]
    assert sorted(order) == sorted(files)
    paths = []
    for n in order:
        (tmp_path / (n + ".jpg")).write_bytes(files[n])
        paths.append(str(tmp_path / (n + ".jpg")))
    monkeypatch.delenv("JPEGBLK_CHUNK_BYTES", raising=False)
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "0")
    with jb.Context(0) as c:
        want = [c.decode_memory(files[n]) for n in order]
        assert c.device_entropy_images == 0
    monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", "2")   # (every eligible file, however few chunks it has)
    with jb.BatchDecoder(4, 0) as dec:
        for rep in range(2):
            imgs, st, tm = dec.run(paths)
            assert tm["rc"] == 0 and all(x == 0 for x in st), (tm, st)
            for n, got, w in zip(order, imgs, want):
                assert np.array_equal(got, w), (n, rep)
            assert dec.device_entropy_images == (rep + 1) * (len(paths) - 1)


# ---- d. hand-written streams --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    return ht.hand_streams()


def test_hand_written_streams_on_the_device(jb, dctx, hand):
    """Streams no writer makes (tests/huff_tables.py hand_streams): run-only symbols and runs that end exactly at position
    63 decode to the host decoder's coefficients; a run that leaves the block and symbols outside the baseline alphabet
    are JB_ERR_FORMAT -- an answer, never a crash."""
    for name in ht.HAND_ACCEPTED:
        data, want = hand[name]
        _, _, ch = jb.entropy_decode(data)
        assert np.array_equal(ch, want), name
        assert np.array_equal(dctx.entropy_decode_device(data)[2], ch), name
    for name in ht.HAND_REJECTED:
        with pytest.raises(jb.JbError) as e:
            dctx.entropy_decode_device(hand[name][0])
        assert e.value.status == -8, (name, e.value)
