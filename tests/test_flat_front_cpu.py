"""The flat front end of the 4:4:4 tile kernel, host side (no GPU): jb_flat_front_geometry -- the predicate the pixel
launch asks before it takes the entry whose first loads read at base + blockIdx * 24576 -- against brute force.  A launch
may be flat exactly when, for EVERY workgroup, that address is the one the general prologue computes (img * stride +
(my * mcus_x + mx0) * 384) and the tile is full (64 MCUs): the test walks all tiles of every shape and compares."""
import numpy as np
import pytest

TILE_MCUS, MCU_BYTES = 64, 384        # 4:4:4: 64 MCUs of three 128-byte blocks a tile
TILE_BYTES = TILE_MCUS * MCU_BYTES    # 24576


@pytest.fixture(scope="module")
def flat():
    import jpeg_decoder_amd as jb
    return jb.flat_front_geometry


def brute(mcus_x, mcus_y, linear, n_images, stride):
    """(every workgroup's flat address is its general address and its tile is full, the last tile's flat offset)"""
    if linear:
        tpi = -(-mcus_x * mcus_y // TILE_MCUS)
    else:
        tpr = -(-mcus_x // TILE_MCUS)
        tpi = tpr * mcus_y
    t = np.arange(n_images * tpi, dtype=np.int64)
    img, rem = t // tpi, t % tpi
    if linear:
        m0 = rem * TILE_MCUS
        my, mx0 = m0 // mcus_x, m0 % mcus_x
        nvalid = np.minimum(TILE_MCUS, mcus_x * mcus_y - m0)
    else:
        my, mx0 = rem // tpr, (rem % tpr) * TILE_MCUS
        nvalid = np.minimum(TILE_MCUS, mcus_x - mx0)
    general = img * stride + (my * mcus_x + mx0) * MCU_BYTES
    return bool(np.array_equal(general, t * TILE_BYTES) and (nvalid == TILE_MCUS).all()), int(t[-1]) * TILE_BYTES


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("h", [8, 16, 24])
def test_predicate_is_brute_force(flat, h, linear):
    n_flat = 0
    for w in range(8, 1101, 8):
        mcus_x, mcus_y = w // 8, h // 8
        dense = mcus_x * mcus_y * MCU_BYTES
        for stride in (dense, dense + 128):
            for n in (1, 3):
                want, _ = brute(mcus_x, mcus_y, linear, n, stride)
                assert flat(1, 1, linear, mcus_x, mcus_y, n, stride) == want, (w, h, linear, n, stride)
                n_flat += want
    assert n_flat > 0   # (both answers occur: 512- and 1024-pixel rows are flat in either tiling)


def test_one_image_has_no_stride(flat):
    """img is 0 for every workgroup of a one-image launch: the stride is multiplied by nothing"""
    assert flat(1, 1, 0, 64, 2, 1, 0) and flat(1, 1, 0, 64, 2, 1, 64 * 2 * MCU_BYTES + 128)
    assert not flat(1, 1, 0, 64, 2, 2, 64 * 2 * MCU_BYTES + 128)


def test_last_tile_beyond_32_bits(flat):
    """64 images of 4096 x 4096: 262144 tiles, the last at byte 6.4e9 of the batch -- geometry only, nothing is allocated"""
    mcus = 512
    want, last = brute(mcus, mcus, 0, 64, mcus * mcus * MCU_BYTES)
    assert want and last > 1 << 32
    assert flat(1, 1, 0, mcus, mcus, 64, mcus * mcus * MCU_BYTES)
    assert not flat(1, 1, 0, mcus, mcus, 64, mcus * mcus * MCU_BYTES + 16)


def test_other_layouts_and_arguments(flat):
    """the subsampled layouts have no flat entry; nonsense geometry is refused, not divided by"""
    for hs, vs in ((2, 2), (2, 1), (1, 2)):
        assert not flat(hs, vs, 0, 64, 2, 1, 0)
    assert not flat(1, 1, 0, 0, 2, 1, 0) and not flat(1, 1, 0, 64, 0, 1, 0) and not flat(1, 1, 0, 64, 2, 0, 0)
