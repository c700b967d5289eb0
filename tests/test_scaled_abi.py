"""Scaled output (include/jpegblk.h "scaled output"), the parts that need no GPU: jb_scaled_size, the
refusal of denominators outside {1, 2, 4, 8}, and the area reduction the GPU tests hold the library to."""
import numpy as np
import pytest

from area_reduce import area_reduce


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


SIZES = [(1, 1), (7, 13), (8, 8), (9, 17), (679, 451), (1920, 1080), (4096, 4096), (65535, 65535), (65535, 1)]


@pytest.mark.parametrize("w,h", SIZES)
def test_scaled_size_table(jb, w, h):
    for k in (1, 2, 4, 8):
        assert jb.scaled_size(w, h, k) == (-(-w // k), -(-h // k)), (w, h, k)


@pytest.mark.parametrize("k", [0, 3, 16, -1, 5, 7])
def test_scaled_size_refuses_other_denominators(jb, k):
    with pytest.raises(jb.JbError) as e:
        jb.scaled_size(640, 480, k)
    assert e.value.status == -2  # JB_ERR_GEOMETRY


def test_scaled_size_refuses_bad_images(jb):
    for w, h in [(0, 1), (1, 0), (65536, 1), (-5, 5)]:
        with pytest.raises(jb.JbError):
            jb.scaled_size(w, h, 2)


def test_area_reduce_definition():
    """The rounding rule, by hand: floor((S + n/2) / n) over the pixels inside the image only."""
    a = np.zeros((3, 5, 3), np.uint8)
    a[..., 0] = [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]]
    r = area_reduce(a, 2)
    assert r.shape == (2, 3, 3)
    # boxes: (1+2+6+7)=16/4 -> 4; (3+4+8+9)=24/4 -> 6; (5+10)=15/2 -> floor(8.5) = 8
    #        (11+12)=23/2 -> 12; (13+14)=27/2 -> 14; 15/1 -> 15
    assert r[..., 0].tolist() == [[4, 6, 8], [12, 14, 15]]
    assert np.array_equal(area_reduce(a, 1), a)
    b = np.full((13, 7, 3), 255, np.uint8)
    for k in (2, 4, 8):
        assert (area_reduce(b, k) == 255).all()


@pytest.mark.parametrize("w,h", [(64, 48), (67, 45), (679, 451)])
def test_area_reduce_matches_pil_reduce_on_full_boxes(w, h):
    """Inside the image the reduction is PIL's Image.reduce(K); PIL may differ by 1 on clipped edge
    boxes whose pixel count is not a power of two (it divides with a fixed-point reciprocal)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    for k in (2, 4, 8):
        ours = area_reduce(img, k)
        pil = np.asarray(Image.fromarray(img).reduce(k))
        assert ours.shape == pil.shape
        fw, fh = w // k, h // k  # whole boxes
        assert np.array_equal(ours[:fh, :fw], pil[:fh, :fw]), k
        assert np.abs(ours.astype(int) - pil.astype(int)).max() <= 1, k
