"""The sort-job rule of tests/bz2_sort_jobs.py, without a GPU: on every first
round of every case of bz2_sort_cases, bwt_tied_list_cases and bz2_place_cases,
and on the crafted streams of bz2_sort_jobs,

  - the jobs of a chunk partition it at bucket boundaries;
  - no job exceeds its capacity, and a job of several buckets fits the
    half-size sorter;
  - a chunk of several buckets and more than 512 rotations gives exactly two
    jobs, the second its last bucket -- unless cuts_of did not close it after
    that bucket (the stream's last chunk, a chunk in front of a bucket above
    kChunk), which is then at most kChunk long and one job; every other chunk
    gives one job;
  - no tie group spans two jobs;

and each crafted stream holds the chunk it is named for, split as listed."""
import os
import re

import numpy as np
import pytest

import bwt_tied_list_cases as C
import bz2_place_cases as P
import bz2_sort_cases as S
import bz2_sort_jobs as J
from conftest import PKG

KCHUNK = S.K["kChunk"]


def test_rule_constants_are_the_kernels():
    src = open(os.path.join(PKG, "csrc", "lfm_bzip2.hip")).read()
    assert re.search(r"\bkMiniCap = %d;" % J.MINI, src)
    assert J.CAPS == (J.MINI, S.K["kTinyCap"], S.SMALL_CAP, S.BIG_CAP)
    assert re.search(r"mid = last < m && m > kMiniCap \? ce - last : ce;", src), "the split rule"
    import lfm
    assert lfm.SORT_JOB_CAPS == J.CAPS


def check_round(fr, where):
    """The properties above on one stream's first round; the number of chunks split."""
    if fr["overflow"]:
        assert not fr["chunks"]
        return 0
    edges = set(np.concatenate([[0], np.cumsum(fr["hist"][fr["hist"] > 0])]).tolist())
    closing = J.closing_buckets(fr["hist"])
    jobs = J.jobs_of(fr)
    assert len(jobs) == len(fr["chunks"])
    split = 0
    flat = []
    for (b, e, _, nb), parts in zip(fr["chunks"], jobs):
        m = e - b
        assert parts[0][0] == b and parts[-1][1] == e, where
        for (_, pe, _), (nb_, _, _) in zip(parts[:-1], parts[1:]):
            assert pe == nb_, where
        for pb, pe, cap in parts:
            assert pb < pe and pb in edges and pe in edges, where
            assert cap is None or pe - pb <= cap, where
            assert cap == J.cap_of(pe - pb), where
            if pe - pb > KCHUNK:  # one bucket
                assert not any(x in edges for x in range(pb + 1, min(pe, pb + 4 * KCHUNK))), where
        closed = e in closing  # (then e is a cut entry, also where e == nsub)
        assert not closed or e in fr["cuts"], where
        if nb > 1 and m > J.MINI and closed:
            assert len(parts) == 2 and parts[1][1] - parts[1][0] == closing[e], where
            split += 1
        else:
            assert len(parts) == 1, where
            if nb > 1:
                assert m <= KCHUNK, where
        if nb > 1 and m > KCHUNK:
            assert len(parts) == 2, where
        flat += parts
    # tie groups: runs of consecutive tied slots
    begins = np.array([p[0] for p in flat])
    at = 0
    for g in fr["groups"]:
        s0 = int(fr["slots"][at])
        at += len(g)
        k = int(np.searchsorted(begins, s0, side="right")) - 1
        assert flat[k][0] <= s0 and s0 + len(g) <= flat[k][1], (where, "a tie group spans two jobs")
    return split


def rounds_of(m):
    return [(a, s, fr) for a, att in enumerate(m["attempts"]) for s, fr in att["first"].items()]


def all_models():
    for cid, _, _, _ in S.all_cases():
        yield cid, S.model_of(cid)
    for c in C.CASES:
        yield c[0], C.model_of(c[0])
    for c in P.cases():
        yield c[0], P.model_of(c[0])


def test_rule_on_every_case_list():
    split = nrounds = 0
    for cid, m in all_models():
        for a, s, fr in rounds_of(m):
            split += check_round(fr, (cid, a, s))
            nrounds += 1
        n = J.job_counts(m["rounds"])
        st = m["stats"]
        # single buckets above 2 048 are a chunk and a job each; nothing is lost or doubled
        assert n[4096] == st["chunks_big"], cid
        assert sum(n.values()) >= st["chunks_tiny"] + st["chunks_small"] + st["chunks_big"], cid
        assert n[2048] <= st["chunks_small"], cid
    print("%d first rounds, %d chunks split" % (nrounds, split))
    assert split >= 20


@pytest.mark.parametrize("cid", [c[0] for c in J.CRAFTED])
def test_crafted_stream(cid):
    """Alone, and padded to a longer raw length (as in its GPU call): the
    named chunk is there and gives the listed jobs."""
    _, sizes, pair, at, want = [c for c in J.CRAFTED if c[0] == cid][0]
    lengths = [None] + [len(r) for call in J.CALLS for x, r in zip(call[1], J.rows_of(call[0])) if x == cid]
    assert len(lengths) > 1, "every crafted stream is part of a GPU call"
    for total in lengths:
        T = S.text_of(J.crafted_raw(cid, total))
        assert S.mode_of(T) == S.FULL
        fr = S.first_round(T, S.FULL)
        check_round(fr, cid)
        assert fr["hist"][fr["hist"] > 0][:len(sizes)].tolist() == list(sizes)
        (k,) = [k for k, c in enumerate(fr["chunks"]) if c[0] == at]
        jobs = J.jobs_of(fr)[k]
        if want is not None:
            assert [(e - b, cap) for b, e, cap in jobs] == want
        else:  # the stream's last chunk, of several buckets and above 512: one job
            b, e, _, nb = fr["chunks"][k]
            assert k == len(fr["chunks"]) - 1 and e == fr["nsub"] and nb > 1 and J.MINI < e - b <= KCHUNK
            assert jobs == [(b, e, 1024)]
        if pair is not None:
            lo = sum(sizes[:pair])
            (g,) = [g for g, s0 in zip(fr["groups"], group_starts(fr)) if lo <= s0 < lo + sizes[pair]]
            assert len(g) == 2


def group_starts(fr):
    at, out = 0, []
    for g in fr["groups"]:
        out.append(int(fr["slots"][at]))
        at += len(g)
    return out


def test_calls_are_what_they_claim():
    """The GPU calls: a run left to the text rounds beside split chunks, a
    restart, a kModeSortA stream with split chunks, and every sorter used."""
    seen = dict.fromkeys(J.CAPS, 0)
    for call, _ in J.CALLS:
        m = J.model_of(call)
        assert not any(m["host"]), call
        for a, s, fr in rounds_of(m):
            check_round(fr, (call, a, s))
        for cap, n in J.job_counts(m["rounds"]).items():
            seen[cap] += n
    left, restart, sort_a = J.model_of("JC-left-run"), J.model_of("JC-restart"), J.model_of("JC-sort-a")
    st = left["stats"]
    assert st["left_runs"] >= 1 and st["text_rounds"] == 1 and not st["restarted"] and not st["chunks_segmented"]
    assert any(len(p) == 2 for fr in left["rounds"].values() for p in J.jobs_of(fr))
    assert restart["stats"]["restarted"] == 1 and restart["it_full"]
    assert any(len(p) == 2 for fr in restart["rounds"].values() for p in J.jobs_of(fr))
    assert sort_a["modes"][1] == S.SORT_A and not sort_a["it_full"]
    assert any(len(p) == 2 for p in J.jobs_of(sort_a["rounds"][1]))
    assert J.model_of("JC-last-chunk")["modes"][1] == S.SORT_A
    pairs = J.model_of("JC-pairs")
    assert pairs["stats"]["left_runs"] == 0 and pairs["stats"]["first_ties"] >= 4
    assert all(seen[c] > 0 for c in J.CAPS[:3]), seen
