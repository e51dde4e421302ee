"""The tied list of the placing chunk sorts (bwt_chunk_sort<.., PLACE>: blocked
load, sa stored at tied slots only, the slots appended per workgroup for
tie_runs_direct and bwt_place_tied) and the second pass of the sorts without
PLACE when a run is left, on the calls of tests/bwt_tied_list_cases.py, whose
premises tests/test_bwt_tied_list_cpu.py proves.  For every call, by the
comparison of test_bwt_place_path_gpu.py (run_call of
test_bwt_sort_seams_gpu.py):

  - no stream is flagged for the host library;
  - every stream is byte-identical to the reference bzip2;
  - lfm_hip_bzip2_last_bwt_stats equals the model field by field;
  - lfm.bzip2_last_place_path() is the path those stats imply."""
import pytest

import bwt_tied_list_cases as C
import bz2_place_cases as P
import bz2_sort_cases as S
from test_bwt_sort_seams_gpu import run_call

pytestmark = pytest.mark.gpu


def check(lfmlib, torch, oracle, cid, rows, m):
    bad = run_call(lfmlib, torch, oracle, cid, rows, C.LEVEL, m)
    got, want = lfmlib.bzip2_last_place_path(), P.place_path(m["stats"])
    print("%s: placement path %d, model %d" % (cid, got, want))
    if got != want:
        bad.append((cid, "place path %d, model %d" % (got, want)))
    return bad


@pytest.mark.parametrize("cid", [c[0] for c in C.CASES])
def test_case(lfmlib, oracle, gpu, cid):
    m = C.model_of(cid)
    assert not any(m["host"])
    bad = check(lfmlib, gpu, oracle, cid, C.rows_of(cid), m)
    assert not bad, bad


def test_control_restart(lfmlib, oracle, gpu):
    """A restart case of bz2_sort_cases (it_full), unchanged."""
    (c,) = [c for c in S.all_cases() if c[0] == C.CONTROL]
    bad = check(lfmlib, gpu, oracle, c[0], c[1], S.model_of(c[0]))
    assert not bad, bad
