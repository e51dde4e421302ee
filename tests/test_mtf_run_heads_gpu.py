"""mtf_win's run-head walk against the reference bzip2, byte for byte: the rows
of tests/bz2_mtf_run_cases.py (head counts of 1, 63, 64, 65 and 128 per
segment, runs over and up to the load and segment seams, the ring at its
fullest, loads of 47 and 48 heads (below and at the count from which a load
is a window of its own) with and without heads pending, a window gathered
from ten loads, dense next to sparse segments,
short last segments that end in a run, a pixel-like row), whose premises
tests/test_mtf_run_heads_cpu.py proves on the reference's own streams.  Every
row must come back with flags == 0: a row handed to the host library would
hide a wrong kernel."""
import pytest

import bz2_encode_cases as C
import bz2_mtf_run_cases as R
from test_bzip2_seams_gpu import expected, run_batch, run_cases

pytestmark = pytest.mark.gpu


def test_run_head_cases(lfmlib, oracle, gpu):
    """Every case, in batches of equal length (the rows of 36 864 bytes in one
    call, the three short last segments a call each)."""
    failed, _ = run_cases(lfmlib, gpu, oracle, [(cid, raw) for cid, raw, _ in R.cases()])
    assert not failed, failed


def test_run_head_cases_in_one_mixed_batch(lfmlib, oracle, gpu):
    """One-head, 63 to 128 head, dense / sparse and pixel-like rows side by
    side, twice over: more streams than one workgroup row, and neighbours of
    either kind for each."""
    rows = R.mixed_batch()
    rows = rows + rows[::-1]
    got, flags, _ = run_batch(lfmlib, gpu, oracle, [raw for _, raw in rows], C.LEVEL, False)
    failed = [cid for (cid, raw), g, f in zip(rows, got, flags) if f != 0 or g != expected(oracle, raw, C.LEVEL)]
    assert not failed, failed
