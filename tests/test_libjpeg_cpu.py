"""Decoder arithmetic JB_ARITH_LIBJPEG without a GPU: the restatement tests/libjpeg_ref.py against Pillow's own bits --
the known-answer file tests/golden/libjpeg_decode_kat.npz (tools/gen_libjpeg_kat.py), and live Pillow where it is
installed -- its domain check, and the setters' NULL handling.  The host front end (entropy_decode) supplies the
coefficients."""
import io
import os

import numpy as np
import pytest

import libjpeg_ref
from conftest import GOLD

KAT = libjpeg_ref.load_kat()


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


def test_kat_holds_the_cases_the_contract_names():
    names = [n for n, _, _ in KAT]
    for want in ("420_521x37_noise_q95", "444_521x19", "422_1033x11", "440_515x37_synth", "420_1x1", "420_2x1", "420_3x5", "420_4x4",
                 "420_5x3", "420_17x1", "422_3x5", "422_5x3", "420_40x24_binary_q100", "420_40x24_binary_q30", "gray_33x21",
                 "420_45x35_progressive", "420_70x40_restart"):
        assert want in names, want
    assert os.path.getsize(os.path.join(GOLD, "libjpeg_decode_kat.npz")) < 256 * 1024


@pytest.mark.parametrize("k", range(len(KAT)), ids=[n for n, _, _ in KAT])
def test_ref_equals_the_kats_pillow_bits(jb, k):
    name, jpeg, rgb = KAT[k]
    desc, q, coef = jb.entropy_decode(jpeg)
    assert (desc.height, desc.width, 3) == rgb.shape
    assert np.array_equal(libjpeg_ref.decode_blocks(desc, q, coef.reshape(-1, 64)), rgb), name


def test_binary_cases_reach_both_clamps():
    for name, _, rgb in KAT:
        if "binary" in name:
            assert rgb.min() == 0 and rgb.max() == 255, name


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_ref_equals_live_pillow(jb, sub):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(77 + sub)
    for w, h in ((1, 2), (6, 2), (9, 9), (31, 17), (64, 48), (233, 131)):
        quality = (30, 95, 100)[(w + h + sub) % 3]
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        f = io.BytesIO()
        Image.fromarray(px).save(f, "JPEG", quality=quality, subsampling=sub)
        want = np.asarray(Image.open(io.BytesIO(f.getvalue())).convert("RGB"))
        desc, q, coef = jb.entropy_decode(f.getvalue())
        assert np.array_equal(libjpeg_ref.decode_blocks(desc, q, coef.reshape(-1, 64)), want), (w, h, sub, quality)


def test_roi_needs_the_neighbours_outside_it(jb):
    """The first rectangle's edge pixels differ from an upsampling that clamps at the rectangle's MCUs: test_gpu_libjpeg.py's
    rectangle test cannot pass without the halo."""
    _, jpeg, rgb = KAT[0]
    desc, q, coef = jb.entropy_decode(jpeg)
    coef = coef.reshape(-1, 64)
    y, cb, cr = libjpeg_ref.planes_of(desc, q, coef)
    x0, y0, w, h = 16, 16, 16, 16
    sub = lambda c: libjpeg_ref.upsample(c[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], w, h, 2, 2)
    alone = libjpeg_ref.colour(y[y0:y0 + h, x0:x0 + w].astype(np.int64), sub(cb), sub(cr))
    assert not np.array_equal(alone, rgb[y0:y0 + h, x0:x0 + w])


def test_domain_check_raises_on_full_range_blocks(jb):
    from jpeg_decoder_amd import synth
    w, h = 16, 16
    n = synth.geometry(w, h, 2, 2)[3]
    coef = synth.random_blocks(n, 5)
    with pytest.raises(libjpeg_ref.OutOfDomain):
        libjpeg_ref.decode_blocks(jb.make_desc(w, h, 2, 2), synth.annex_k_qtabs(90), coef)


def test_setters_refuse_null_handles(jb):
    L = jb.lib()
    assert L.jb_ctx_set_arithmetic(None, 1) == -1
    assert L.jb_batch_decoder_set_arithmetic(None, 1) == -1
    assert L.jb_ctx_arithmetic(None) == jb.ARITH_REFERENCE == 0 and jb.ARITH_LIBJPEG == 1
