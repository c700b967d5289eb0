"""The 192 / 256-lane tile kernel's front end on the GPU (-m gpu): the prologue that finds a workgroup's tile without a
division (csrc/jb_divmagic.h), the full-tile and the ragged load path of the 4:4:4 LDS-DMA branch, and the quantisation
table fetched ahead of the coefficients' arrival.  Small images, JPEGBLK_SMALL_GRID=0 so that they go through that kernel
and not the one-wave kernels; sentinel-filled buffers with padded strides (tests/seam_harness.py); bit-exact against the
oracle.  Every case has several images, three MCU rows and a divisor that is no power of two, and a table per image (and,
in 4:4:4, per component), so that a tile taken for another, or a table fetched from another image's or another
component's place, changes bytes."""
import numpy as np
import pytest

from seam_harness import Seam, _oracle_full

pytestmark = pytest.mark.gpu

QID = (0, 1, 2)


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


def _context(jb, row_tiling):
    """A context that never takes the small-grid kernels (the knobs are read when it is created); row_tiling: the
    row-bound tiling even where it leaves a ragged tile per MCU row (otherwise such a width gets the linear tiling)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("JPEGBLK_SMALL_GRID", "0")
        mp.delenv("JPEGBLK_BYTE_STORE", raising=False)
        if row_tiling:
            mp.setenv("JPEGBLK_ROW_TILING", "1")
        else:
            mp.delenv("JPEGBLK_ROW_TILING", raising=False)
        return jb.Context(0, 64 << 20, 64 << 20, 3)


@pytest.fixture(scope="module")
def ctx_default(jb):
    c = _context(jb, False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_row(jb):
    c = _context(jb, True)
    yield c
    c.close()


def _tables(n):
    """n table sets, each with three different tables (luma, Cb, Cr), no two sets alike"""
    from jpeg_decoder_amd import synth
    out = []
    for i in range(n):
        q = synth.annex_k_qtabs(90 - 17 * i).copy()
        q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1 + i, 1, 255)
        assert not np.array_equal(q[0], q[1]) and not np.array_equal(q[1], q[2]) and not np.array_equal(q[0], q[2])
        out.append(q)
    assert all(not np.array_equal(out[i], out[j]) for i in range(n) for j in range(i))
    return out


def _check(jb, ctx, oracle, w, h, hs, vs, n, kind, tag, qid=QID):
    from jpeg_decoder_amd import synth
    qs = _tables(n)
    g = jb.geometry_of(jb.make_desc(w, h, hs, vs))
    if kind == "synth":
        coefs = [synth.synth_blocks(w, h, hs, vs, image_index=31 + i, qtabs=qs[i], qtab_id=qid)[0] for i in range(n)]
    else:
        coefs = [synth.random_blocks(g.n_coded_blocks, 101 + i) for i in range(n)]  # full-range int16
    wants = [_oracle_full(oracle, w, h, hs, vs, coefs[i], qs[i], qid) for i in range(n)]
    assert all(not np.array_equal(wants[i], wants[j]) for i in range(n) for j in range(i))
    Seam(jb, w, h, hs, vs, coefs, qs, qid, pad_row=13, pad_img=77).check(ctx, wants, 0, tag=tag)
    return g


@pytest.mark.parametrize("kind", ["synth", "random"])
def test_444_full_tiles_two_per_row_three_rows_three_images(jb, ctx_default, oracle, kind):
    """1024 x 24: 128 MCUs a row = two full tiles, three MCU rows, six tiles an image, 18 workgroups: every one takes the
    full-tile load path; tiles_per_image = 6 is no power of two and three images put workgroups behind multiples of it."""
    g = _check(jb, ctx_default, oracle, 1024, 24, 1, 1, 3, kind, "444 1024x24")
    assert (g.mcus_x, g.mcus_y) == (128, 3)


def test_444_full_and_ragged_tiles_in_one_launch_row_bound(jb, ctx_row, oracle):
    """1032 x 24, row-bound: 129 MCUs a row = tiles of 64, 64 and 1 MCUs (tiles_per_row = 3, tiles_per_image = 9), two
    images: both load paths in one launch, the last tile of the last image among the ragged ones."""
    g = _check(jb, ctx_row, oracle, 1032, 24, 1, 1, 2, "random", "444 1032x24 row-bound")
    assert (g.mcus_x, g.mcus_y) == (129, 3)


def test_444_full_and_ragged_tiles_in_one_launch_linear(jb, ctx_default, oracle):
    """The same image in the tiling it gets by default, the linear one: 387 MCUs = six full tiles and one of 3 MCUs."""
    _check(jb, ctx_default, oracle, 1032, 24, 1, 1, 2, "random", "444 1032x24 linear")


def test_444_linear_tiling_divides_by_mcus_x(jb, ctx_default, oracle):
    """1000 x 24: 125 MCUs a row, 375 an image = tiles that start at MCUs 0, 64, 128 (row 1, column 3), 192, 256 (row 2,
    column 6), 320 -- m0 / mcus_x with a divisor that is no power of two -- the last one 55 MCUs long."""
    g = _check(jb, ctx_default, oracle, 1000, 24, 1, 1, 2, "synth", "444 1000x24 linear")
    assert (g.mcus_x, g.mcus_y) == (125, 3)


# The direct-load layouts, which change through the prologue alone: a width of two full tiles and one MCU (tiles_per_row =
# 3 row-bound; linear: mcus_x = 65 or 129), three MCU rows, two images.  Cb and Cr share a table, the usual case, but for
# the last case: the MIXQ instantiation of 4:2:0.
@pytest.mark.parametrize("row_tiling", [True, False])
@pytest.mark.parametrize("w,h,hs,vs,qid", [(1040, 48, 2, 2, (0, 1, 1)), (2064, 24, 2, 1, (0, 1, 1)), (1032, 48, 1, 2, (0, 1, 1)),
                                           (1040, 48, 2, 2, (0, 1, 2))])
def test_direct_load_layouts_two_full_tiles_and_one_mcu(jb, ctx_default, ctx_row, oracle, w, h, hs, vs, qid, row_tiling):
    g = _check(jb, ctx_row if row_tiling else ctx_default, oracle, w, h, hs, vs, 2, "synth", (w, h, hs, vs, qid, row_tiling), qid)
    assert g.mcus_x == 2 * (32 if (hs, vs) == (2, 2) else 64) + 1 and g.mcus_y == 3
