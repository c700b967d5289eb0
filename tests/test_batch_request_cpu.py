"""The batch decoder's request rules without a GPU: tools/fuzz/batch_request_check, a stand-alone program over
jpeg_decoder_amd/csrc/jb_batch_request.h under sanitizers, against the table recorded on a device."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


def test_request_rules_equal_the_recorded_refusals():
    """tools/fuzz/batch_request_check walks OutputRequest::verdict over every request of tests/batch_refusal_cases.py that can
    be had and every setter argument that passes the setter's own check, and PerFile's builders and PerFile::check over every
    entry point's per-file arguments on the five decoder states with nothing in flight -- under ASan + UBSan -- and every row it
    prints equals the row of that name in tests/golden/batch_refusals.json, code and text; it prints every such row of the
    table.  The decoder-level rows (a batch in flight, the setters' own argument checks, NULL decoders and outputs, the arena
    and the device regions, tickets) need a decoder and stay with tests/test_gpu_batch_refusals.py."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import batch_refusal_cases
    import record_batch_refusals
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, "batch_request_check"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "batch_request_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = [line.split("\t") for line in r.stdout.split("\n") if line]
    golden = {name: (rc, text) for name, rc, text in record_batch_refusals.load()}
    assert sorted(g[0] for g in got) == sorted(batch_refusal_cases.pure_names()) and len(got) > 2500
    for name, rc, text in got:
        assert (int(rc), text) == golden[name], name
