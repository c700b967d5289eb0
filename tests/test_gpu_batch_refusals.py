"""The refusals of the batch decoder, all of them, against the table recorded before the decoder was taken apart
(tests/batch_refusal_cases.py has the cases, tools/record_batch_refusals.py wrote tests/golden/batch_refusals.json)."""
import os
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_batch_refusals_equal_the_recorded_table(tmp_path):
    """every setter on every request that can be had, idle and with a batch in flight; the twelve entry points on seven
    decoder states with every bad argument; arena and device regions on a single and a two-part decoder; ticket errors:
    return code and jb_last_error text, row by row"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import batch_refusal_cases
    import jpeg_decoder_amd as jb
    import record_batch_refusals
    golden = record_batch_refusals.load()
    got = batch_refusal_cases.cases(jb, batch_refusal_cases.tiny_files(tmp_path))
    assert [g[0] for g in got] == [g[0] for g in golden]
    wrong = [(a, b) for a, b in zip(got, golden) if a != b]
    assert not wrong, (len(wrong), wrong[:5])
