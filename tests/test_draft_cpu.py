"""Draft decode without a GPU: the restatement tests/draft_ref.py against Pillow's own bits -- the known-answer file
tests/golden/libjpeg_draft_kat.npz (tools/gen_draft_kat.py), and live Pillow where it is installed -- jb_draft_geometry_of
against jdmaster.c's rule for every layout and draft, the setters' statuses that need no device, and the pure-host
checkers on a descriptor of the draft frame.  The host front end (entropy_decode) supplies the coefficients."""
import os

import numpy as np
import pytest

import draft_ref
import libjpeg_ref
from conftest import GOLD

KAT = draft_ref.load_kat()
LAYOUTS = [(1, 1), (2, 2), (2, 1), (1, 2)]
SIZES = [(1, 1), (2, 1), (3, 5), (4, 4), (5, 3), (7, 40), (40, 7), (9, 33), (33, 9), (16, 16), (17, 9), (37, 29), (64, 48), (131, 70), (521, 37)]
# (hs, vs, K) -> (S, Sc, eh, ev, fancy), worked out by hand from jdmaster.c's loop and jdsample.c's switch
BLOCKS = {(1, 1, 2): (4, 4, 1, 1, 1), (1, 1, 4): (2, 2, 1, 1, 1), (1, 1, 8): (1, 1, 1, 1, 0),
          (2, 2, 2): (4, 8, 1, 1, 1), (2, 2, 4): (2, 4, 1, 1, 1), (2, 2, 8): (1, 2, 1, 1, 0),
          (2, 1, 2): (4, 4, 2, 1, 1), (2, 1, 4): (2, 2, 2, 1, 1), (2, 1, 8): (1, 1, 2, 1, 0),
          (1, 2, 2): (4, 4, 1, 2, 1), (1, 2, 4): (2, 2, 1, 2, 1), (1, 2, 8): (1, 1, 1, 2, 0)}


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


def test_kat_holds_the_decode_kats_files_and_one_file_per_layout():
    names = [n for n, _, _ in KAT]
    for name, _, _ in libjpeg_ref.load_kat():
        assert name in names, name
    for want in ("draft_444_131x70", "draft_422_131x70", "draft_420_131x70", "draft_gray_131x70", "draft_440_131x70_synth"):
        assert want in names, want
    assert os.path.getsize(os.path.join(GOLD, "libjpeg_draft_kat.npz")) < 256 * 1024


@pytest.mark.parametrize("k", range(len(KAT)), ids=[n for n, _, _ in KAT])
def test_ref_equals_the_kats_pillow_bits(jb, k):
    name, jpeg, drafts = KAT[k]
    desc, q, coef = jb.entropy_decode(jpeg)
    for K in draft_ref.DENOMS:
        want = drafts[K]
        assert want.shape == (-(-desc.height // K), -(-desc.width // K), 3), (name, K)
        assert np.array_equal(draft_ref.decode_blocks(desc, q, coef.reshape(-1, 64), K), want), (name, K)


def test_draft_is_not_the_area_mean_of_the_full_decode():
    """What scale= would give under the reference arithmetic's definition (an area mean of the full-size image) is
    another image: a test that passes with one in the other's place shows nothing."""
    from resize_ref import area_resize
    full = {n: rgb for n, _, rgb in libjpeg_ref.load_kat()}
    name = "420_521x37_noise_q95"
    want = dict((n, d) for n, _, d in KAT)[name][2]
    assert not np.array_equal(area_resize(full[name], want.shape[1], want.shape[0]), want)


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_ref_equals_live_pillow(jb, hs, vs):
    pytest.importorskip("PIL.Image")
    from jpeg_decoder_amd import synth
    for i, (w, h) in enumerate(SIZES):
        coef, q = synth.synth_blocks(w, h, hs, vs, image_index=100 + i)
        jpeg = synth.encode_jpeg(coef, w, h, hs, vs, q)
        desc, q4, c = jb.entropy_decode(jpeg)
        for K in draft_ref.DENOMS:
            assert np.array_equal(draft_ref.decode_blocks(desc, q4, c.reshape(-1, 64), K), draft_ref.pillow_draft(jpeg, K)), (hs, vs, w, h, K)


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_draft_geometry_of_every_layout_and_draft(jb, hs, vs):
    for K in draft_ref.DENOMS:
        for w, h in SIZES + [(65535, 65535), (8, 8), (15, 17)]:
            g = jb.draft_geometry(jb.make_desc(w, h, hs, vs), K)
            assert (g.width, g.height) == (-(-w // K), -(-h // K)), (w, h, K)
            assert (g.luma_block, g.chroma_block, g.up_h, g.up_v, g.fancy) == BLOCKS[hs, vs, K], (hs, vs, K)
            assert g.reserved == 0
            assert (g.width, g.height, g.luma_block, g.chroma_block, g.up_h, g.up_v, g.fancy) == draft_ref.geometry(w, h, hs, vs, K)
    g = jb.draft_geometry(jb.make_desc(37, 29, hs, vs), 1)
    assert (g.width, g.height, g.luma_block, g.chroma_block, g.up_h, g.up_v, g.fancy) == (37, 29, 8, 8, hs, vs, 1)


def test_draft_geometry_statuses(jb):
    import ctypes
    L = jb.lib()
    d, g = jb.make_desc(16, 16, 2, 2), jb.DraftGeometry()
    assert L.jb_draft_geometry_of(None, 2, ctypes.byref(g)) == -1
    assert L.jb_draft_geometry_of(ctypes.byref(d), 2, None) == -1
    for bad in (0, 3, 5, 16, -2):
        assert L.jb_draft_geometry_of(ctypes.byref(d), bad, ctypes.byref(g)) == -2, bad
    assert L.jb_draft_geometry_of(ctypes.byref(jb.make_desc(0, 16, 2, 2)), 2, ctypes.byref(g)) == -2
    assert L.jb_draft_geometry_of(ctypes.byref(jb.make_desc(16, 16, 3, 1)), 2, ctypes.byref(g)) == -3
    assert L.jb_draft_geometry_of(ctypes.byref(jb.make_desc(16, 16, 1, 1, (0, 4, 1))), 2, ctypes.byref(g)) == -4


def test_setters_refuse_null_handles(jb):
    L = jb.lib()
    assert L.jb_ctx_set_draft(None, 2) == -1
    assert L.jb_batch_decoder_set_draft(None, 2) == -1
    assert L.jb_ctx_draft(None) == 1


def test_rectangles_are_checked_against_the_draft_frame(jb):
    """The pure-host checkers take draft coordinates through a descriptor of the draft frame: 521 x 37 at draft 4 is
    131 x 10, and what lies in the full frame alone is refused."""
    full = jb.make_desc(521, 37, 2, 2)
    g = jb.draft_geometry(full, 4)
    assert (g.width, g.height) == (131, 10)
    frame = jb.make_desc(g.width, g.height, 2, 2)
    inside, outside = (100, 2, 31, 8), (100, 2, 32, 8)

    def status(call, *a, **kw):
        try:
            call(*a, **kw)
        except jb.JbError as e:
            return e.status
        return 0

    assert status(jb.roi_check, full, outside) == 0 and status(jb.roi_check, frame, inside) == 0 and status(jb.roi_check, frame, outside) == -2
    assert status(jb.resize_check, frame, (8, 8), roi=inside) == 0 and status(jb.resize_check, frame, (8, 8), roi=outside) == -2
    assert status(jb.crops_check, frame, [inside, inside], (8, 8)) == 0 and status(jb.crops_check, frame, [inside, outside], (8, 8)) == -2
    assert status(jb.views_check, frame, [[inside, (0, 0, 131, 10)]], (8, 8)) == 0 and status(jb.views_check, frame, [[inside, outside]], (8, 8)) == -2
    # the tap cap is that of the draft frame: bicubic 521 -> 8 is refused (65 x: beyond 160 taps), 131 -> 8 is taken
    assert status(jb.filter_check, full, (8, 8), jb.FILTER_BICUBIC) == -9
    assert status(jb.filter_check, frame, (8, 8), jb.FILTER_BICUBIC) == 0
    win = jb.filter_window(frame, (10, 3), jb.FILTER_BICUBIC, roi=(60, 2, 40, 6))
    assert win[0] >= 0 and win[1] >= 0 and win[0] + win[2] <= 131 and win[1] + win[3] <= 10
    src, inner = jb.fit_geometry(g.width, g.height, (8, 8), jb.Fit.cover())
    assert src[0] + src[2] <= 131 and src[1] + src[3] <= 10 and inner == (0, 0, 8, 8)


def test_kernels_and_launchers_under_sanitizers(tmp_path):
    """tools/fuzz/lj_kernel_check: the block and pixel kernels of csrc/jb_libjpeg.hip and their two launchers on the CPU --
    every file of both known-answer sets at draft 1, 2, 4, 8, the whole frame, rectangles through the ROI launch and
    all of them in one crops launch, exactly-sized coefficients, planes and outputs -- under ASan + UBSan, against
    Pillow's bits."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "lj_kernel_check"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    cases = str(tmp_path / "lj_cases.bin")
    w = subprocess.run([sys.executable, os.path.join(d, "lj_kernel_cases.py"), cases], capture_output=True, text=True, timeout=120)
    assert w.returncode == 0, (w.stdout + w.stderr)[-3000:]
    r = subprocess.run([os.path.join(d, "lj_kernel_check"), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) >= 4 * len(libjpeg_ref.load_kat()) * 4, r.stdout     # (at least four launches per frame of the decode KAT)
