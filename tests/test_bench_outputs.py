"""CPU tests of bench.py --dump-outputs: what dump_outputs() writes from a batch of images, checked against
numpy on the same bytes (a host tensor stands in for the device buffer)."""
import os
import sys
import types

import numpy as np
import torch

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _batch(nimg, w, h, pitch, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, size=(nimg, h, pitch), dtype=np.uint8)
    res = types.SimpleNamespace(w=w, h=h, nimg=nimg, pitch=pitch)
    return res, rgb


def test_dump_outputs_row_sums_and_sample(tmp_path):
    """Row sums cover every pixel byte and no pitch padding; the sample holds the bytes at its seeded positions;
    everything is float32 / float64 and within the 64 MB budget."""
    bench = _bench()
    res, rgb = _batch(3, 37, 11, 128, seed=1)            # 3 * 37 = 111 pixel bytes per row, 17 bytes of padding
    bench.dump_outputs(str(tmp_path), np, torch, res, torch.from_numpy(rgb))
    sums = np.load(tmp_path / "rgb_row_sums.npy")
    sample = np.load(tmp_path / "rgb_sample.npy")
    assert sums.dtype == np.float64 and sample.dtype == np.float32
    assert np.array_equal(sums, rgb[:, :, :111].sum(axis=2, dtype=np.int64).astype(np.float64))
    pix = rgb[:, :, :111].reshape(-1)
    assert sample.size == pix.size                       # smaller than DUMP_SAMPLE_BYTES: one draw per byte
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, pix.size, size=pix.size, dtype=np.int64))
    assert np.array_equal(sample, pix[pos].astype(np.float32))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_BUDGET_BYTES + 1024


def test_dump_outputs_is_deterministic_and_bounded(tmp_path):
    """The same images give the same files; a large batch is sampled, not dumped whole."""
    bench = _bench()
    res, rgb = _batch(2, 1500, 1000, 4500, seed=2)       # 9 MB of pixel bytes > DUMP_SAMPLE_BYTES
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), np, torch, res, torch.from_numpy(rgb))
    for f in ("rgb_row_sums.npy", "rgb_sample.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    sample = np.load(tmp_path / "a" / "rgb_sample.npy")
    assert sample.size == bench.DUMP_SAMPLE_BYTES
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET_BYTES + 1024
