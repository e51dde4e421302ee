"""How the GPU bzip2 encoder places its sorted rotations -- in the chunk sorts
(bwt_chunk_sort<.., PLACE>, then bwt_place_tied and bwt_pend_live), by
bwt_place_sorted over the whole batch, or not at all -- on the calls of
tests/bz2_place_cases.py, whose premises tests/test_bwt_place_path_cpu.py
proves.  For every call, as in test_bwt_sort_seams_gpu.py:

  - flags are non-zero exactly for the streams the model hands to the host;
  - every stream with flags == 0 is byte-identical to the reference bzip2;
  - lfm_hip_bzip2_last_bwt_stats equals the model;

and lfm.bzip2_last_place_path() is the path those stats imply
(bz2_place_cases.place_path): a case that silently leaves the fused path, or
takes it when it must not, fails.

The existing lists hold no call with a kModeFull stream beside typed ones that
stays on the fused path (test_bwt_induce_compact_gpu's mixed batch restarts: 60
times 0xFB in its text); P-full-beside-ordinary is that batch with the lists'
own 0xFB lead.  List H restarts too (path 0); P-two-parts-direct is the multi
entry on the fused path."""
import pytest

import bz2_place_cases as P
from test_bwt_sort_seams_gpu import run_call

pytestmark = pytest.mark.gpu


def run(lfmlib, torch, oracle, cids):
    bad = []
    for cid in cids:
        _, rows, level, multi = P.case(cid)
        m = P.model_of(cid)
        bad += run_call(lfmlib, torch, oracle, cid, rows, level, m, multi=multi)
        got, want = lfmlib.bzip2_last_place_path(), P.place_path(m["stats"])
        print("%s: placement path %d, model %d" % (cid, got, want))
        if got != want:
            bad.append((cid, "place path %d, model %d" % (got, want)))
    return bad


def test_fused_with_ties(lfmlib, oracle, gpu):
    """Runs of 2, 31 and 32 and typed runs settled directly, and a tied pair
    (in the text in the order opposite to the sorted one) at the first two
    slots, the last two slots and across a thread's blocked boundary of the
    256 x 4, 512 x 4 and 512 x 8 sorters."""
    bad = run(lfmlib, gpu, oracle, ["D-run-2", "D-run-31", "D-run-32", "D-agree-40-typed"] + [p[0] for p in P.PAIRS])
    assert not bad, bad


def test_chunk_fill(lfmlib, oracle, gpu):
    """Chunks of exactly 1, 1 024, 1 025, 2 048, 2 049 and 4 096 rotations on
    the fused path; 4 097 (segmented sort) on the whole-batch kernel."""
    bad = run(lfmlib, gpu, oracle, ["P-chunk-1", "A-multi-1024", "A-bucket-1025", "A-multi-1025", "A-bucket-2048",
                                    "A-multi-2048", "A-bucket-2049", "A-bucket-4096", "A-bucket-4097"])
    assert not bad, bad
    assert P.place_path(P.model_of("A-bucket-4097")["stats"]) == P.WHOLE


def test_text_wrap(lfmlib, oracle, gpu):
    """kModeSortA and kModeSortB: rotations 0 .. 3 and n - 8 .. n - 1 sorted
    (the keys over the wrap, rotation 0's origPtr), and each of rotations
    0 .. 3 sorted at the head of a chain of placed ones, which take
    T[i-2 .. i-4] -- bytes from over the wrap -- out of its entry."""
    bad = run(lfmlib, gpu, oracle, ["P-wrap-sort-a", "P-wrap-sort-b"])
    assert not bad, bad


def test_streams(lfmlib, oracle, gpu):
    """Two and nine streams of different text lengths and alphabets; a
    host-flagged stream (cut overflow) between two ordinary ones; a kModeFull
    stream beside typed ones."""
    bad = run(lfmlib, gpu, oracle, ["P-two-streams", "P-nine-streams", "P-flagged-between", "P-full-beside-ordinary"])
    assert not bad, bad


def test_live_slots(lfmlib, oracle, gpu):
    """No live slot at all; nearly every placed rotation live, in both scan
    directions (bwt_pend_live writes a range per bucket)."""
    bad = run(lfmlib, gpu, oracle, ["P-no-live-slot", "P-live-rising", "P-live-falling"])
    assert not bad, bad


def test_off_the_fused_path(lfmlib, oracle, gpu):
    """A text round and the segmented sort (path 2), the restart (path 0)."""
    bad = run(lfmlib, gpu, oracle, ["E-agree-12", "A-bucket-4097", "D-agree-72"])
    assert not bad, bad
    assert [P.place_path(P.model_of(c)["stats"]) for c in ("E-agree-12", "A-bucket-4097", "D-agree-72")] == \
        [P.WHOLE, P.WHOLE, P.NONE]


def test_parts(lfmlib, oracle, gpu):
    """Two parts at level 1 through the multi entry: list H (restart) and
    its stream without the run of 33 (fused)."""
    bad = run(lfmlib, gpu, oracle, ["H-two-parts", "P-two-parts-direct"])
    assert not bad, bad
    assert P.place_path(P.model_of("P-two-parts-direct")["stats"]) == P.FUSED
