"""CPU tests: pin the oracle (oracle/jpegblk_oracle.c) to the reference.

(1) against the committed golden vectors generated from the genuine reference build
    (oracle/gen_golden.py) -- runs everywhere;
(2) directly against oracle/_ref/libjpegref.so (the reference compiled in place) when that
    build is present, and always against the digests of its answers recorded in
    tests/golden/ref_results.json (oracle/gen_golden.py) -- which must agree with it where it is present.
Parity bar: bit-exact (the task's +-1 LSB allowance is not used)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import BASELINE_IMAGES, GOLD, load_golden, load_kat
from jpeg_decoder_amd import synth
from oracle.pyoracle import Ref, make_desc

# f32 bit patterns of reference include/types.hpp:5-19 and jpeg.cpp:521-523
EXPECTED_CONSTANTS = [0x3FEC835E, 0x3FB504F3, 0x3F8A8BD4, 0x3FB504F3, 0x40273D74, 0x3F43EF15,
                      0x3EB504F3, 0x3EFB14BE, 0x3EEC835E, 0x3ED4DB31, 0x3EB504F3, 0x3E8E39DA,
                      0x3E43EF15, 0x3DC7C5C2, 0x3FB374BC, 0x3EB020C5, 0x3F36C8B4, 0x3FE2D0E5]


def test_constants_match_reference(oracle, manifest):
    assert [int(x) for x in oracle.constants()] == EXPECTED_CONSTANTS
    assert manifest["constants_f32_bits"] == EXPECTED_CONSTANTS


@pytest.mark.parametrize("name", BASELINE_IMAGES)
def test_oracle_matches_golden_image(oracle, manifest, name):
    desc, coef, qtabs, rgb = load_golden(name)
    out = oracle.blocks_to_rgb(desc, coef, qtabs)
    assert out.shape == rgb.shape
    assert np.array_equal(out, rgb)
    assert hashlib.sha256(out.tobytes()).hexdigest() == manifest["images"][name]["rgb_sha256"]
    g = oracle.geometry(desc)
    m = manifest["images"][name]
    assert (g.mcu_w_real, g.mcu_h_real, g.n_coded_blocks) == (m["mcu_w_real"], m["mcu_h_real"], m["n_coded_blocks"])


def test_oracle_matches_golden_kat(oracle, manifest):
    kat = load_kat()
    assert len(kat) == len(manifest["kat"]) >= 50
    for name, (desc, coef, qtabs, rgb) in kat.items():
        out = oracle.blocks_to_rgb(desc, coef, qtabs)
        assert np.array_equal(out, rgb), name


def test_oracle_threads_agree(oracle):
    desc, coef, qtabs, rgb = load_golden("img")
    assert np.array_equal(oracle.blocks_to_rgb(desc, coef, qtabs, nthreads=3), rgb)


def test_oracle_row_stride(oracle):
    desc, coef, qtabs, rgb = load_golden("img2")
    out = oracle.blocks_to_rgb(desc, coef, qtabs, stride=3 * desc.width + 13)
    assert np.array_equal(out, rgb)


def test_oracle_rejects_bad_descriptors(oracle):
    from oracle.pyoracle import Geometry
    import ctypes
    for bad, rc in [(make_desc(0, 8, 1, 1), -2), (make_desc(8, 70000, 1, 1), -2),
                    (make_desc(8, 8, 3, 1), -3), (make_desc(8, 8, 1, 4), -3),
                    (make_desc(8, 8, 1, 1, (0, 4, 1)), -4)]:
        g = Geometry()
        assert oracle.lib.jbo_geometry_of(ctypes.byref(bad), ctypes.byref(g)) == rc


def test_dc_only_block_is_flat(oracle):
    # DC-only block: every 1-D pass sees one non-zero input -> a flat block.  800*s0 = 282.84
    # truncates to 282 after the column pass, 282*s0 = 99.70 truncates to 99 after the row
    # pass (an exact IDCT with rounding would give 100): the reference's two truncations.
    blk = np.zeros(64, np.int32)
    blk[0] = 800
    out = oracle.idct_block(blk)
    assert (out == out[0]).all() and out[0] == 99


@pytest.fixture(scope="module")
def ref_results():
    with open(os.path.join(GOLD, "ref_results.json")) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_ref_constants(oracle, manifest):
    """The oracle's constants == the reference build's, or, without it, those it gave for tests/golden/."""
    want = Ref().constants() if Ref.available() else np.array(manifest["constants_f32_bits"], np.uint32)
    assert np.array_equal(want, oracle.constants())


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_oracle_matches_reference_on_random_blocks(oracle, ref_results, hs, vs):
    ref = Ref() if Ref.available() else None
    q = synth.annex_k_qtabs(75)
    q[2] = 255
    q[3] = 1
    for (w, h, seed) in [(8, 8, 1), (100, 52, 2), (257, 131, 3)]:
        d = make_desc(w, h, hs, vs, (0, 1, 2))
        n = oracle.geometry(d).n_coded_blocks
        for kind, coef in (("full", synth.random_blocks(n, seed)), ("small", synth.random_blocks(n, seed + 10, -64, 64))):
            got = oracle.blocks_to_rgb(d, coef, q)
            if ref is not None:
                assert np.array_equal(got, ref.blocks_to_rgb(d, coef, q))
            assert _sha(got) == ref_results["random_blocks"][f"{hs}x{vs}/{w}x{h}/seed{seed}/{kind}"], (w, h, seed, kind)


@pytest.mark.parametrize("w,h,hs,vs,rows", [(679, 451, 2, 2, 0), (333, 211, 1, 1, 0), (100, 60, 2, 1, 0),
                                              (64, 80, 1, 2, 0), (640, 360, 1, 1, 2), (512, 256, 2, 2, 1)])
def test_writer_streams_through_the_reference_reader(oracle, ref_results, tmp_path, w, h, hs, vs, rows):
    """Pins the build's baseline writer (tools/jpegwriter) with the genuine reference: the
    reference's own marker parser + Huffman decoder (oracle/_ref) must read back exactly the
    blocks and tables that were written, and its RGB must equal the oracle's on them.  Restart
    intervals only as whole MCU rows -- the reference's restart test (jpeg.cpp:414,419) counts
    block rows, see INTEGRATION.md section 5.  Without the reference build: the writer must still
    produce the very stream whose reading by the reference tests/golden/ref_results.json records."""
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import Ref, make_desc
    coef, q = synth.synth_blocks(w, h, hs, vs, 21)
    ri = rows * synth.geometry(w, h, hs, vs)[0]
    data = synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri)
    rgb = oracle.blocks_to_rgb(make_desc(w, h, hs, vs), coef, q)
    if Ref.available():
        p = tmp_path / "w.jpg"
        p.write_bytes(data)
        info, rcoef, rq, rrgb = Ref().decode_file(str(p))
        assert (info.width, info.height, info.hs, info.vs) == (w, h, hs, vs)
        assert np.array_equal(rcoef, coef) and np.array_equal(rq[:2], q[:2])
        assert np.array_equal(rrgb, rgb)
    rec = ref_results["writer_streams"][f"{w}x{h}/{hs}x{vs}/rows{rows}"]
    assert _sha(np.frombuffer(data, np.uint8)) == rec["stream_sha256"], "the writer no longer makes the stream the reference read"
    assert rec["frame"] == [w, h, hs, vs]
    assert _sha(coef) == rec["coef_sha256"] and _sha(q[:2]) == rec["qtabs01_sha256"]
    assert _sha(rgb) == rec["rgb_sha256"]
