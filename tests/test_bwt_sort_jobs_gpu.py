"""The sort jobs of the GPU bzip2 encoder's BWT (bwt_bucket's job lists, the
128 x 4, 256 x 4, 512 x 4 and 512 x 8 shapes of bwt_chunk_sort over them, with
and without PLACE) on the calls of tests/bz2_sort_jobs.py, whose premises
tests/test_bwt_sort_jobs_cpu.py proves.  For every call, by run_call of
test_bwt_sort_seams_gpu.py and one more comparison:

  - no stream is flagged, and every stream is byte-identical to the reference
    bzip2;
  - lfm_hip_bzip2_last_bwt_stats equals the model of bz2_sort_cases field by
    field (the chunk classes are what they were);
  - lfm.bzip2_last_sort_jobs() equals the job rule's counts."""
import pytest

import bwt_tied_list_cases as C
import bz2_sort_cases as S
import bz2_sort_jobs as J
from test_bwt_sort_seams_gpu import run_call

pytestmark = pytest.mark.gpu


def check(lfmlib, torch, oracle, cid, rows, level, m):
    bad = run_call(lfmlib, torch, oracle, cid, rows, level, m)
    got, want = lfmlib.bzip2_last_sort_jobs(), J.job_counts(m["rounds"])
    print("%s: sort jobs %s, model %s" % (cid, got, want))
    if got != want:
        bad.append((cid, "sort jobs %s, model %s" % (got, want)))
    return bad


@pytest.mark.parametrize("call", [c[0] for c in J.CALLS])
def test_call(lfmlib, oracle, gpu, call):
    m = J.model_of(call)
    assert not any(m["host"])
    bad = check(lfmlib, gpu, oracle, call, J.rows_of(call), J.LEVEL, m)
    assert not bad, bad


@pytest.mark.parametrize("cid", ["A-multi-2047", "A-bucket-4096", "A-classes-x9"])
def test_job_counts_on_the_chunk_class_list(lfmlib, oracle, gpu, cid):
    """Cases of bz2_sort_cases' list A: a chunk split at 1 023 | 1 024, the big
    sorter's single buckets and the segmented sort's (no job), nine streams."""
    (c,) = [c for c in S.a_cases() if c[0] == cid]
    bad = check(lfmlib, gpu, oracle, cid, c[1], c[2], S.model_of(cid))
    assert not bad, bad


def test_job_counts_with_runs_in_three_sorters(lfmlib, oracle, gpu):
    """A call of bwt_tied_list_cases: tied runs in chunks of every class, 36 buckets of a few hundred."""
    cid = "L-s20"
    bad = check(lfmlib, gpu, oracle, cid, C.rows_of(cid), C.LEVEL, C.model_of(cid))
    assert not bad, bad
