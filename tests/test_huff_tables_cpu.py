"""The device entropy decoder on Huffman tables that are not Annex K's, without a GPU (the same cases run on the MI355X in
tests/test_gpu_huff_tables.py).  tests/huff_tables.py makes the table shapes; here
  a. the lookup tables jb_huff_fill_table_ builds from them (dumped by tools/fuzz/huff_table_dump, a stand-alone program
     under ASan + UBSan) resolve EVERY 16-bit window to the symbol and length a canonical-code decoder written out below
     finds, or to "no code" -- and use exactly the second-level tables the codes' prefixes call for;
  b. the host decoder reads back exactly the blocks the writer coded with them (and so does the genuine reference, where
     oracle/_ref exists);
  c. the kernels of jb_huff.hip, emulated (tools/huff_emu), decode the same files with status 0 at both chunk sizes, with
     the default launches and with 8 -- or leave a set that does not fit the pool to the host decoder, with the reason;
  d. streams no writer makes (run-only symbols, runs that end exactly at or just beyond the block's last position, symbols
     outside the baseline alphabet) get the same coefficients, or the same verdict, from the host decoder and the kernels.
Every comparison is integer-exact."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import huff_tables as ht
from test_huff_emu import EMU, EMU_DIR, run, three_table_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ((1, 1), (2, 1), (1, 2), (2, 2))
INTERVALS = (0, 1, 5)
W, H = 200, 120
# a family as it is, and (some) with the Cr component on tables of its own: (family, three tables per kind)
VARIANTS = [(n, False) for n in ht.FAMILIES] + [(n, True) for n in ht.THREE_TABLES]
VARIANT_IDS = [n + ("-three" if t else "") for n, t in VARIANTS]


@pytest.fixture(scope="module")
def emu():
    import jpeg_decoder_amd as jb
    jb.lib()
    r = subprocess.run(["make", "-C", EMU_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EMU


@pytest.fixture(scope="module")
def dump_exe():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "huff_table_dump"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    return os.path.join(d, "huff_table_dump")


def encode(name, three, coef, w, h, hs, vs, q, ri):
    from jpeg_decoder_amd import synth
    data = synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=ri, huffman=ht.family(name))
    return three_table_variant(data) if three else data


REF_READS = {}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Every variant x layout x restart interval x content on 200 x 120, and one dense +-1 image per variant: written once,
    {(family, three): [(path, blocks written)]}; REF_READS[path]: the genuine reference can be asked about the file."""
    d = tmp_path_factory.mktemp("huff_tables")
    content = {lay: ht.contents(W, H, *lay) for lay in LAYOUTS}
    dense = ht.dense_pm1_blocks(W, H, 1, 1, 3)
    from jpeg_decoder_amd import synth
    out = {}
    for (name, three), vid in zip(VARIANTS, VARIANT_IDS):
        files = []
        for (hs, vs) in LAYOUTS:
            for ri in INTERVALS:
                for kind, (coef, q) in content[(hs, vs)].items():
                    p = d / f"{vid}_{hs}{vs}_{ri}_{kind}.jpg"
                    p.write_bytes(encode(name, three, coef, W, H, hs, vs, q, ri))
                    files.append((str(p), coef))
                    # (the reference's restart test, jpeg.cpp:414-419, counts MCUs right only while vs = 1)
                    REF_READS[str(p)] = ri == 0 or vs == 1
        p = d / f"{vid}_dense.jpg"
        p.write_bytes(encode(name, three, dense, W, H, 1, 1, synth.annex_k_qtabs(90), 0))
        files.append((str(p), dense))
        REF_READS[str(p)] = True
        out[(name, three)] = files
    return out


# ---- a. table construction ------------------------------------------------------------------------------------------------
def canonical_decode_all(bits, vals):
    """Every 16-bit window through a canonical-code decoder (T.81 F.2.2.3): take one more bit at a time, and at each length
    compare the bits so far with the running code of that length's first symbol.  -> (symbol or -1, length) per window."""
    w = np.arange(1 << 16, dtype=np.int64)
    sym = np.full(1 << 16, -1, np.int64)
    length = np.zeros(1 << 16, np.int64)
    vals = np.asarray(vals, np.int64)
    code, k = 0, 0
    for ln in range(1, 17):
        n = bits[ln - 1]
        c = w >> (16 - ln)
        hit = (length == 0) & (c >= code) & (c < code + n)
        sym[hit] = vals[k + c[hit] - code]
        length[hit] = ln
        k += n
        code = (code + n) << 1
    return sym, length


def expected_entries(is_ac, sym, length):
    """What a window's symbol means to the step (jb_huff.h): (total bits, magnitude bits, advance of k), all 0 for "no code"
    -- also for a symbol outside the baseline alphabet (DC size > 11, AC size > 10)."""
    if not is_ac:
        ok = (sym >= 0) & (sym <= 11)
        size, adv = sym, np.ones_like(sym)
    else:
        size, runlen = sym & 15, sym >> 4
        ok = (sym >= 0) & (size <= 10)
        adv = np.where(sym == 0, 82, np.where(sym == 0xf0, 17, runlen + 1))
    total = length + size
    return np.where(ok, total, 0), np.where(ok, size, 0), np.where(ok, adv, 0)


def dump_set(exe, tmp_path, tables):
    blob = bytes([len(tables)])
    for is_ac, (bits, vals) in tables:
        blob += bytes([int(is_ac)]) + bytes(bits) + bytes([len(vals)]) + bytes(vals)
    src, dst = tmp_path / "set.bin", tmp_path / "set.out"
    src.write_bytes(blob)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]   # (a sanitizer report ends the program with a failure)
    raw = dst.read_bytes()
    n, n_t2 = np.frombuffer(raw, np.uint32, 2)
    refused = int(np.frombuffer(raw, np.int32, 1, 8)[0])
    t1 = np.frombuffer(raw, np.uint16, int(n) * 1024, 12).reshape(int(n), 1024)
    t2 = np.frombuffer(raw, np.uint16, 24 * 64, 12 + int(n) * 2048).reshape(24, 64)
    return int(n_t2), refused, t1, t2


def check_set(exe, tmp_path, tables, refused_at=None):
    n_t2, refused, t1, t2 = dump_set(exe, tmp_path, tables)
    if refused_at is not None:
        # the pool fills up in this table: refused there, with all 24 tables given out and nothing written beyond them
        assert (refused, n_t2) == (refused_at, ht.POOL)
        return
    assert refused == -1
    assert n_t2 == ht.t2_tables([t for _, t in tables])
    w = np.arange(1 << 16)
    for tix, (is_ac, (bits, vals)) in enumerate(tables):
        e = t1[tix][w >> 6].astype(np.int64)
        second = (e >= 1) & (e <= 31)                      # (the step's test: e - 1 < 31)
        assert e[second].max(initial=0) <= n_t2
        e = np.where(second, t2[np.clip(e - 1, 0, 23), w & 63], e)
        sym, length = canonical_decode_all(bits, vals)
        total, size, adv = expected_entries(is_ac, sym, length)
        # a code of at most 10 bits must not need the second level, a longer one must (a window without a code may end in either)
        assert np.array_equal(second[length > 0], length[length > 0] > ht.T1_BITS), tix
        bad = (e & 31) != total
        bad |= ((e >> 5) & 15) != size
        bad |= (e >> 9) != adv
        assert not bad.any(), (tix, int(np.flatnonzero(bad)[0]), int(bad.sum()))


@pytest.mark.parametrize("name,three", VARIANTS, ids=VARIANT_IDS)
def test_lookup_tables_resolve_every_window(dump_exe, tmp_path, name, three):
    """65,536 windows x every table of the set (4, or 6 with three tables per kind) against the decoder above."""
    refused_at = {"pool25": 0, "pool_shared": 3}.get(name)
    check_set(dump_exe, tmp_path, ht.set_tables(name, three), refused_at)


def test_lookup_tables_of_the_hand_made_set(dump_exe, tmp_path):
    """The tables of the hand-written streams hold symbols outside the baseline alphabet (DC 12, AC 0x0B: no entry) and the
    run-only symbols 0x10..0xE0 (entries that advance k by the run and carry no magnitude bits)."""
    dc_l, ac_l, dc_c, ac_c = ht.hand_tables()
    tables = [(True, ac_l), (True, ac_c), (False, dc_l), (False, dc_c)]
    sym, _ = canonical_decode_all(*ac_l)
    total, size, adv = expected_entries(True, sym, np.zeros_like(sym))
    assert (total[sym == 0x0b] == 0).all() and (adv[sym == 0x30] == 4).all() and (size[sym == 0x30] == 0).all()
    check_set(dump_exe, tmp_path, tables)


# ---- b. the host decoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,three", VARIANTS, ids=VARIANT_IDS)
def test_host_decoder_reads_back_the_blocks_written(corpus, tmp_path, name, three):
    """jb_entropy_decode on every file of the variant == the blocks the writer was given; and, where the genuine reference
    has been built (oracle/_ref), its decodeHuffman() dump says the same for every file it can read (REF_READS) -- run in
    a child process, because it calls exit(1) on what it rejects."""
    import jpeg_decoder_amd as jb
    from oracle.pyoracle import Ref
    files = corpus[(name, three)]
    assert len(files) == len(LAYOUTS) * len(INTERVALS) * 2 + 1
    for path, coef in files:
        d, _, c = jb.entropy_decode(open(path, "rb").read())
        assert (d.width, d.height) == (W, H) and np.array_equal(c, coef), path
    asked = [(p, c) for p, c in files if REF_READS[p]]
    if Ref.available():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "huff_tables.py"), "--ref-dump"] + [p for p, _ in asked],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert len(asked) >= 17
        for path, coef in asked:
            assert np.array_equal(np.load(path + ".ref.npy"), coef), path


# ---- c. the emulated kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,three", [v for v in VARIANTS if v[0] in ht.TAKEN], ids=[i for v, i in zip(VARIANTS, VARIANT_IDS) if v[0] in ht.TAKEN])
def test_emulated_kernels_decode_every_taken_family(emu, corpus, name, three):
    """All files of the variant in one submission, --strict (status 0 and the host decoder's coefficients for every
    image), at both chunk sizes, with the default synchronisation launches and with 8."""
    paths = [p for p, _ in corpus[(name, three)]]
    for chunk in (128, 64):
        for launches in (None, 8):
            r = run(emu, paths, chunk, strict=True, launches=launches)
            assert r.returncode == 0 and "not taken" not in r.stdout, (chunk, launches, (r.stdout + r.stderr)[-3000:])


@pytest.mark.parametrize("name", ht.REFUSED)
def test_sets_beyond_the_pool_are_left_to_the_host_decoder(emu, corpus, name):
    """25 second-level tables -- in one table (pool25) or over the four of a set (pool_shared): jb_huff_prepare_ refuses
    every file of the family with JB_ERR_UNSUPPORTED and says why."""
    paths = [p for p, _ in corpus[(name, False)]]
    r = run(emu, paths, strict=True)
    lines = [ln for ln in r.stdout.splitlines() if "not taken by the device decoder" in ln]
    assert r.returncode == 0 and len(lines) == len(paths), (r.stdout + r.stderr)[-3000:]
    assert all("(-9: " in ln and "more long codes" in ln for ln in lines), lines[:3]


@pytest.mark.parametrize("name", ["flat", "all16"])
def test_emulated_kernels_on_a_large_full_alphabet_frame(emu, tmp_path, name):
    """640 x 480 4:4:4, full-alphabet content, no restart intervals: several workgroups, and a block is longer than a chunk
    (under all16 nearly every symbol is 17..26 bits; under flat no symbol is shorter than 8)."""
    from jpeg_decoder_amd import synth
    coef = ht.full_alphabet_blocks(640, 480, 1, 1, 31)
    p = tmp_path / f"{name}_640.jpg"
    p.write_bytes(encode(name, False, coef, 640, 480, 1, 1, synth.annex_k_qtabs(75), 0))
    r = run(emu, [str(p)], strict=True)
    assert r.returncode == 0 and "not taken" not in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_several_table_sets_in_one_submission(emu, corpus, tmp_path):
    """Files of six families (two, four and -- three tables per kind -- six first-level tables; 0 to 24 second-level
    tables), an Annex-K file and a grayscale file (one table of each kind) in ONE launch: LDS is sized by the largest
    set, and where the second level starts differs from image to image."""
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    from jpeg_decoder_amd import synth
    g = np.clip(np.cumsum(np.random.default_rng(4).normal(0, 5, (120, 200)), axis=1) + 128, 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(g).save(b, "JPEG", quality=88)
    (tmp_path / "gray.jpg").write_bytes(b.getvalue())
    coef, q = synth.synth_blocks(W, H, 2, 1, 9)
    (tmp_path / "annexk.jpg").write_bytes(synth.encode_jpeg(coef, W, H, 2, 1, q))
    pick = [("pool24", False, 3), ("flat", False, 0), ("all16", True, 23), ("t1_split", False, 12), ("unary_dc_long", False, 19),
            ("annexk_reversed", True, 6), ("complete_allones", False, 24)]
    paths = [str(tmp_path / "gray.jpg")]
    for name, three, i in pick:
        paths.append(corpus[(name, three)][i][0])
    paths.insert(4, str(tmp_path / "annexk.jpg"))
    for chunk in (128, 64):
        r = run(emu, paths, chunk, strict=True)
        assert r.returncode == 0 and "not taken" not in r.stdout, (chunk, (r.stdout + r.stderr)[-3000:])


def test_a_state_crosses_one_workgroup_boundary_per_launch(emu, corpus):
    """What the MI355X showed and the emulator's default order hides: the workgroups of a launch run side by side there, so
    a workgroup reads the exit state its left neighbour wrote in the launch BEFORE.  With --side-by-side (workgroups in
    descending order) the dense +-1 image under `flat` -- 9-bit AC symbols throughout, lanes never fall into step by
    themselves -- is flagged "not in step" (4) after the default launches, and decodes with one launch per workgroup (248
    own chunks each, kJbOwnChunks) and one more: the bound of jb_entropy_decode_device's last retry."""
    path = corpus[("flat", False)][-1][0]
    assert path.endswith("flat_dense.jpg")
    env = dict(os.environ, JPEGBLK_CHUNK_BYTES="64")
    r = subprocess.run([emu, "--side-by-side", path], capture_output=True, text=True, timeout=600, env=env)
    status, host_rc, line = _status_line(r.stdout, path)
    n_chunks = int(line.split(" chunks of")[0].split(", ")[-1])
    assert r.returncode == 0 and host_rc == 0 and status == 4 and n_chunks > 4 * 248, line
    enough = -(-n_chunks // 248) + 1
    r = subprocess.run([emu, "--side-by-side", "--strict", "--launches", str(enough), path], capture_output=True, text=True, timeout=600, env=env)
    status, host_rc, line = _status_line(r.stdout, path)
    assert r.returncode == 0 and (status, host_rc) == (0, 0) and " 0 coefficients differ" in line, line


# ---- d. hand-written streams -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    return ht.hand_streams()


def _status_line(stdout, path):
    line = [ln for ln in stdout.splitlines() if ln.startswith(path + ":")]
    assert len(line) == 1, stdout[-2000:]
    status = int(line[0].split("status ")[1].split(",")[0])
    host_rc = int(line[0].split("host rc ")[1].split(",")[0])
    return status, host_rc, line[0]


@pytest.mark.parametrize("name", ht.HAND_ACCEPTED)
def test_hand_written_streams_the_decoders_accept(emu, hand, tmp_path, name):
    """Run-only symbols and runs that end exactly at position 63: the host decoder gives the blocks the stream was written
    for, the emulated kernels give the host decoder's (--strict), the reference too where it has been built."""
    import jpeg_decoder_amd as jb
    from oracle.pyoracle import Ref
    data, want = hand[name]
    _, _, c = jb.entropy_decode(data)
    assert np.array_equal(c, want)
    p = tmp_path / (name + ".jpg")
    p.write_bytes(data)
    for chunk in (128, 64):
        r = subprocess.run([emu, "--strict", str(p)], capture_output=True, text=True, timeout=600, env=dict(os.environ, JPEGBLK_CHUNK_BYTES=str(chunk)))
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        status, host_rc, line = _status_line(r.stdout, str(p))
        assert (status, host_rc) == (0, 0) and " 0 coefficients differ" in line, line
        assert int(line.split(" chunks of")[0].split(", ")[-1]) >= 16, line
    if Ref.available():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "huff_tables.py"), "--ref-dump", str(p)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert np.array_equal(np.load(str(p) + ".ref.npy"), want)


@pytest.mark.parametrize("name", ht.HAND_REJECTED)
def test_hand_written_streams_the_decoders_reject(emu, hand, tmp_path, name):
    """A run that leaves the block (ZRL at k = 48, run/size with k + run = 64) and symbols outside the baseline alphabet:
    the host decoder rejects the stream with JB_ERR_FORMAT, the emulated kernels flag the image (never status 0)."""
    import jpeg_decoder_amd as jb
    data, want = hand[name]
    assert want is None
    from oracle.pyoracle import Ref
    with pytest.raises(jb.JbError) as e:
        jb.entropy_decode(data)
    assert e.value.status == -8
    p = tmp_path / (name + ".jpg")
    p.write_bytes(data)
    if Ref.available():  # (the reference's verdict is its exit(1))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "huff_tables.py"), "--ref-dump", str(p)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and not os.path.exists(str(p) + ".ref.npy"), (r.stdout + r.stderr)[-2000:]
    for chunk in (128, 64):
        for launches in (None, 8):
            cmd = [emu, "--strict"] + (["--launches", str(launches)] if launches else []) + [str(p)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, JPEGBLK_CHUNK_BYTES=str(chunk)))
            assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
            status, host_rc, line = _status_line(r.stdout, str(p))
            assert status != 0 and host_rc == -8, line
