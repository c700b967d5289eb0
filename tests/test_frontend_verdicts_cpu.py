"""The host front end's verdict on malformed and on valid files without a GPU: tools/fuzz/frontend_verdicts, a stand-alone
program over jpeg_decoder_amd/csrc/jb_frontend*.cpp under sanitizers with the device half stubbed, over the files of
tests/frontend_cases.py, against the table recorded from the commit before the front end was rewritten
(tests/golden/frontend_verdicts.json, its "header" says which)."""
import os
import shutil
import sys

import pytest

from conftest import ROOT

# Message texts of the recorded sources that no recorded row holds, each with the reason; at most 6.
UNREACHED = {
    "scan too large for 32-bit bit offsets: host decoder": "needs more than 255 MB of scan",
    "scan too large for the device decoder: host decoder": "needs more than 2^30 chunks, 64 GB of scan",
    "restart intervals out of order": "unstuff() gives ascending interval starts: a guard for the kernels, not a verdict on bytes",
    "bad frame geometry": "the frame rules refuse every descriptor jb_geometry_of refuses before it is asked",
}


@pytest.fixture(scope="module")
def tables():
    """-> (the recorded table, the table of this tree's sources)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_frontend_verdicts as rec
    exe, err = rec.build()
    if exe is None and ("cannot find -lasan" in err or "cannot find -lubsan" in err or "libasan" in err):
        pytest.skip("toolchain without sanitizer runtimes")
    assert exe is not None, err[-2000:]
    return rec.load(), rec.table_of(*rec.rows_of(exe))


def test_verdicts_equal_the_recorded_ones(tables):
    """Every structured case and every row of the twelve jb_decode_memory* / jb_decode_file* entry points equals the
    recorded row, field by field: status, jb_last_error text, the descriptor, the digests of tables, coefficients and
    device job, the route taken.  Every sweep (per seed: all prefixes up to 8 bytes past the first SOS; every header byte
    set to 0x00, 0xFF, byte ^ 0x01) has the recorded number of rows, SHA-256 over them and number of distinct outcomes."""
    golden, got = tables
    fields = got["fields"]
    for key in ("cases", "entries"):
        assert list(got[key]) == list(golden[key]), key
        for name, row in got[key].items():
            assert [fields[i] for i in row] == golden[key][name], name
    assert got["sweeps"] == golden["sweeps"]
    assert len(golden["cases"]) > 400 and len(golden["entries"]) > 500 and sum(s["rows"] for s in golden["sweeps"].values()) > 40000


def test_every_message_text_is_in_a_recorded_row(tables):
    """The condition on the case list: every text that the recorded sources pass to set_err(...) or done(...) occurs in a
    recorded row of a structured case or of an entry point, but for the UNREACHED ones above."""
    golden, _ = tables
    assert len(UNREACHED) <= 6 and set(UNREACHED) <= set(golden["texts"]) and len(golden["texts"]) > 50
    seen = {f.split("|")[1] for rows in (golden["cases"], golden["entries"]) for row in rows.values() for f in row if "|" in f}
    missing = [t for t in golden["texts"] if t not in seen and t not in UNREACHED]
    assert not missing, missing
    assert not [t for t in UNREACHED if t in seen]
