"""The flat front end of the 4:4:4 tile kernel on the GPU (-m gpu): a launch whose every tile is full and whose images lie
densely takes the entry that issues its coefficient loads from base + blockIdx * 24576 before anything else; every other
launch takes the general prologue.  Both must write the same bytes.  Small images through tests/seam_harness.py
(JPEGBLK_SMALL_GRID=0: the 192-lane kernel, not the one-wave kernels), sentinel-filled buffers, bit-exact against the
oracle, three images with a table set each; which front end ran is read back from the context (Context.last_front)."""
import numpy as np
import pytest

import format_ref as fr
from seam_harness import Seam, _oracle_full

pytestmark = pytest.mark.gpu

QID = (0, 1, 2)
N = 3
GENERAL, FLAT = 1, 2
SB = ((0.5, 0.25, 2.0), (-1.0, 0.5, 3.0))


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


def _context(jb, flat_knob=None):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("JPEGBLK_SMALL_GRID", "0")
        for k in ("JPEGBLK_BYTE_STORE", "JPEGBLK_ROW_TILING", "JPEGBLK_FLAT_FRONT"):
            mp.delenv(k, raising=False)
        if flat_knob is not None:
            mp.setenv("JPEGBLK_FLAT_FRONT", flat_knob)
        return jb.Context(0, 64 << 20, 64 << 20, 3)


@pytest.fixture(scope="module")
def ctx(jb):
    c = _context(jb)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off(jb):
    c = _context(jb, "0")
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(jb, oracle):
    """(w, h) -> (coefficients, tables, the oracle's images) of N images of that size: computed once, shared, not written to"""
    from jpeg_decoder_amd import synth
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            g = jb.geometry_of(jb.make_desc(w, h, 1, 1))
            qs = []
            for i in range(N):
                q = synth.annex_k_qtabs(90 - 17 * i).copy()
                q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1 + i, 1, 255)
                qs.append(q)
            coefs = [synth.random_blocks(g.n_coded_blocks, 211 + i) for i in range(N)]   # full-range int16
            wants = [_oracle_full(oracle, w, h, 1, 1, coefs[i], qs[i], QID) for i in range(N)]
            assert all(not np.array_equal(wants[i], wants[j]) for i in range(N) for j in range(i))
            for a in coefs + wants:
                a.setflags(write=False)
            cache[(w, h)] = (coefs, qs, wants)
        return cache[(w, h)]
    return get


def _seam(jb, w, h, coefs, qs, pad_coef=False, **pads):
    """the harness's batch; pad_coef: the images' coefficients 128 bytes further apart than they are long"""
    import torch
    s = Seam(jb, w, h, 1, 1, coefs, qs, QID, **pads)
    if pad_coef:
        n_blocks = coefs[0].shape[0]
        wide = torch.full((len(coefs), n_blocks + 1, 64), 0x7fff, dtype=torch.int16, device="cuda:0")
        wide[:, :n_blocks] = s.coef_t
        s.coef_t = wide[:, :n_blocks]
        assert s.coef_t.stride(0) * 2 == n_blocks * 128 + 128
    return s


def _run(jb, ctx, case, w, h, front, linear, pad_coef=False, fmt=0, **pads):
    coefs, qs, wants = case(w, h)
    if fmt:
        wants = [fr.to_format(x, fmt, *SB) for x in wants]
    host, _ = _seam(jb, w, h, coefs, qs, pad_coef, **pads).check(ctx, wants, fmt, SB if fmt else ((1, 1, 1), (0, 0, 0)),
                                                                 tag=(w, h, pad_coef, fmt, pads))
    assert ctx.last_front() == (front, linear), (w, h, pad_coef, fmt, pads)
    return host


@pytest.mark.parametrize("h", [8, 16])
def test_exact_fit_is_flat_and_a_padded_stride_is_not(jb, ctx, case, h):
    """512 x 8 and 512 x 16: one and two full tiles an image, row-bound; dense -> flat, 128 bytes between the images ->
    the general prologue, the same pixels"""
    a = _run(jb, ctx, case, 512, h, FLAT, 0, pad_row=13, pad_img=77)
    b = _run(jb, ctx, case, 512, h, GENERAL, 0, pad_coef=True, pad_row=13, pad_img=77)
    assert np.array_equal(a, b)


def test_ragged_row_is_general(jb, ctx, case):
    """520 x 8: 65 MCUs a row -- the linear tiling, its second tile one MCU long"""
    _run(jb, ctx, case, 520, 8, GENERAL, 1, pad_row=13, pad_img=77)


def test_linear_tiling_flat_and_not(jb, ctx, case):
    """768 pixels = 96 MCUs a row, no multiple of 64: the linear tiling.  16 rows: 192 MCUs = three full tiles, the second
    across the row's end -> flat; 24 rows: 288 MCUs, the last tile half full -> general"""
    _run(jb, ctx, case, 768, 16, FLAT, 1, pad_row=13, pad_img=77)
    _run(jb, ctx, case, 768, 16, GENERAL, 1, pad_coef=True, pad_row=13, pad_img=77)
    _run(jb, ctx, case, 768, 24, GENERAL, 1, pad_row=13, pad_img=77)


def test_the_output_plays_no_part(jb, ctx, case):
    """flat says where the coefficients lie, nothing about the pixels: a padded pitch, an odd image stride, and a width
    whose last MCU is cut (509: 64 MCUs, the tile still full) are all flat"""
    _run(jb, ctx, case, 512, 8, FLAT, 0, pad_row=64)
    _run(jb, ctx, case, 512, 8, FLAT, 0, pad_img=1)
    _run(jb, ctx, case, 509, 8, FLAT, 0, pad_row=13, pad_img=77)
    _run(jb, ctx, case, 509, 8, FLAT, 0)


def test_knob_off_takes_the_general_path_same_bytes(jb, ctx, ctx_off, case):
    for (w, h, linear) in ((512, 8, 0), (768, 16, 1)):
        a = _run(jb, ctx, case, w, h, FLAT, linear, pad_row=13, pad_img=77)
        b = _run(jb, ctx_off, case, w, h, GENERAL, linear, pad_row=13, pad_img=77)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_planar_formats(jb, ctx, case, fmt):
    a = _run(jb, ctx, case, 512, 8, FLAT, 0, fmt=fmt, pad_row=3, pad_plane=5, pad_img=7)
    b = _run(jb, ctx, case, 512, 8, GENERAL, 0, pad_coef=True, fmt=fmt, pad_row=3, pad_plane=5, pad_img=7)
    assert np.array_equal(a, b)
