"""bench.py on the GPU (-m gpu): a plain run measures the headline alone, and --dump-outputs writes what
its last timed step computed -- checked here against the oracle on the same seeded images."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_what_the_last_step_computed(tmp_path, oracle):
    out = tmp_path / "out"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--precondition", "2", "--workload", "679x451-420", "--images-per-step", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"configs", "end_to_end", "cpu_baseline"} & set(d)          # those take --full
    # the batch of bench.Resident: image i is the seeded image rotated by (i * 7919 mod MCUs) MCUs
    import jpeg_decoder_amd as jb
    from jpeg_decoder_amd import synth
    from oracle.pyoracle import make_desc
    w, h, hs, vs = 679, 451, 2, 2
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=0)
    g = jb.geometry_of(jb.make_desc(w, h, hs, vs))
    want = np.stack([oracle.blocks_to_rgb(make_desc(w, h, hs, vs), np.roll(coef, (i * 7919 % (g.mcus_x * g.mcus_y)) * g.blocks_per_mcu, axis=0),
                                          q, nthreads=4).reshape(h, 3 * w) for i in range(2)])
    sums = np.load(out / "rgb_row_sums.npy")
    assert sums.dtype == np.float64 and np.array_equal(sums, want.sum(axis=2, dtype=np.int64).astype(np.float64))
    sys.path.insert(0, ROOT)
    import bench
    pix = want.reshape(-1)
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, pix.size, size=pix.size, dtype=np.int64))
    sample = np.load(out / "rgb_sample.npy")
    assert sample.dtype == np.float32 and np.array_equal(sample, pix[pos].astype(np.float32))
