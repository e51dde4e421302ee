"""The sort stage of the GPU bzip2 encoder's BWT (bwt_bucket's cuts and chunk
classes, bwt_chunk_sort in its three shapes, the segmented sort with
bwt_chunk_keys / bwt_chunk_flags, tie_offsets, tie_compact, tie_runs_direct,
the text rounds, the restart, rank_rebuild in both forms, the doubling rounds,
bwt_flag_periodic) on the case lists of tests/bz2_sort_cases.py, whose
premises tests/test_bwt_sort_cases_cpu.py proves.  For every call:

  - flags are non-zero exactly for the streams the model hands to the host
    library (periodic ones, and list B's cut overflow);
  - every stream with flags == 0 is byte-identical to the reference bzip2 at
    the same level;
  - lfm_hip_bzip2_last_bwt_stats equals the model field by field, so a case
    that silently takes another path fails.

Every case is a call of its own: the rounds are decided per call (N = slots x
cap), and the statistics are the call's.

List B, the cut overflow: a stream that needs kMaxCuts cut entries or more
comes back with a host flag, which the model predicts -- not with exact bytes.
Before bwt_bucket flagged it, its tail chunk of many buckets went through the
segmented sort of the low 50 key bits (see test_b_cut_overflow)."""
import numpy as np
import pytest

import bz2_sort_cases as S
from test_bwt_induce_compact_gpu import ref_bz2

pytestmark = pytest.mark.gpu


def run_call(lfmlib, torch, oracle, cid, rows, level, m=None, multi=False):
    """One call; the list of what differs from the reference and the model."""
    n = len(rows[0])
    assert all(len(r) == n for r in rows)
    if m is None:
        m = S.model_of(cid)
    d = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy()).cuda()
    got, flags = lfmlib.bzip2_device(d, [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], 1, level=level, multi=multi)
    stats = lfmlib.bzip2_last_bwt_stats()
    print("%s: %d x %d bytes, stats %s, flagged %s" % (cid, len(rows), n, stats, [i for i, f in enumerate(flags) if f]))
    bad = []
    if stats != m["stats"]:
        bad.append((cid, "stats", {k: (stats[k], m["stats"][k]) for k in stats if stats[k] != m["stats"][k]}))
    want_host = m["stream_host"] if "stream_host" in m else m["host"]
    for i, (raw, g, f) in enumerate(zip(rows, got, flags)):
        if bool(f) != bool(want_host[i]):
            bad.append((cid, i, "flags %d, model %s" % (f, want_host[i])))
        elif f == 0 and g != ref_bz2(oracle, raw, level):
            bad.append((cid, i, "bytes differ"))
    return bad


def run_list(lfmlib, torch, oracle, cases):
    bad = []
    for cid, rows, level, _ in cases:
        bad += run_call(lfmlib, torch, oracle, cid, rows, level)
    return bad


def test_a_chunk_classes(lfmlib, oracle, gpu):
    """List A: single buckets of 1 024 .. 4 097 rotations, multi-bucket chunks of
    1 023 .. 2 048, a big bucket at slot 0, two back to back, one chunk, and 1,
    7, 8, 9 chunks per class (the XCD-order launch)."""
    bad = run_list(lfmlib, gpu, oracle, S.a_cases())
    assert not bad, bad


def test_b_cut_overflow(lfmlib, oracle, gpu):
    """List B: the 890 kB text whose 729 buckets above kChunk need 1 457 cut
    entries, and its siblings with 1 022, 1 023 (exact bytes, 1 024 chunks: the
    last lane) and 1 024 entries.  From kMaxCuts entries on the stream comes
    back flagged for the host library, as the model predicts; below, exact.
    (Unflagged, the overflow stream's last chunk ran from the last kept cut to
    nsub over 220 buckets and was sorted by the low 50 key bits only: wrong
    bytes with flags == 0.)"""
    bad = run_list(lfmlib, gpu, oracle, S.b_cases())
    assert not bad, bad


def test_c_keys_at_the_wrap(lfmlib, oracle, gpu):
    bad = run_list(lfmlib, gpu, oracle, S.c_cases())
    assert not bad, bad


def test_d_direct_runs(lfmlib, oracle, gpu):
    bad = run_list(lfmlib, gpu, oracle, S.d_cases())
    assert not bad, bad


def test_e_text_rounds(lfmlib, oracle, gpu):
    bad = run_list(lfmlib, gpu, oracle, S.e_cases())
    assert not bad, bad


def test_f_restart_ranks_doubling(lfmlib, oracle, gpu):
    bad = run_list(lfmlib, gpu, oracle, S.f_cases())
    assert not bad, bad


def test_g_list_plumbing(lfmlib, oracle, gpu):
    bad = run_list(lfmlib, gpu, oracle, S.g_cases())
    assert not bad, bad


def test_g_same_shape_twice_with_roles_swapped(lfmlib, oracle, gpu):
    """Two calls of one shape, one after the other (the second takes the
    first one's workspace back from the allocator): the tied and the untied
    streams swapped, so stale uflag / done of the first call would show."""
    first, second = S.g_swap_pair()
    bad = []
    for name, rows in (("G-swap-first", first), ("G-swap-second", second)):
        m = S.model([S.text_of(r) for r in rows], S.call_cap(rows, 2))
        bad += run_call(lfmlib, gpu, oracle, name, rows, 2, m)
    assert not bad, bad


def test_h_parts(lfmlib, oracle, gpu):
    """One stream of two bzip2 blocks through lfm_hip_bzip2_blocks_multi at
    level 1: the slots are the parts, N = 2 x the part cap."""
    raw, m = S.h_model()
    bad = run_call(lfmlib, gpu, oracle, "H-two-parts", [raw], S.H_LEVEL, m, multi=True)
    assert not bad, bad
