"""The premises of test_bwt_place_path_gpu.py, without a GPU: the rule that
decides how a call's sorted rotations are placed, as a function of the
model's stats, takes all three values over lists A to H, and each case of
tests/bz2_place_cases.py is what it is named for (where its tied slots lie in
their chunk, which chunk sizes occur, which rotations at the wrap are sorted,
which streams are flagged or sorted whole, how many slots are live)."""
import os
import re

import numpy as np
import pytest

import bz2_place_cases as P
import bz2_sort_cases as S
import test_bwt_induce_compact_cpu as M
from conftest import PKG


def test_rule_is_the_hosts():
    src = open(os.path.join(PKG, "csrc", "lfm_bzip2.hip")).read()
    assert re.search(r"return it_full \? 0u : \(fused_sorts && left_runs == 0 && text_rounds == 0\) \? 1u : 2u;", src)
    assert re.search(r"const bool fused = !B\.it_full && nch\[2\] == 0;", src)


def test_rule_takes_every_value_over_the_lists():
    """Lists A to H of bz2_sort_cases: every path is met, the three cases the
    GPU test names for paths 2 and 0 are on them, and so is list H."""
    seen = {}
    for cid, _, _, _ in S.all_cases():
        if cid.startswith("B-") or cid.startswith("G-batch"):  # (long models; the flagged stream is met below)
            continue
        seen.setdefault(P.place_path(S.model_of(cid)["stats"]), []).append(cid)
    seen.setdefault(P.place_path(S.h_model()[1]["stats"]), []).append("H-two-parts")
    print({k: len(v) for k, v in seen.items()})
    assert set(seen) == {P.NONE, P.FUSED, P.WHOLE}
    assert "E-agree-12" in seen[P.WHOLE] and "A-bucket-4097" in seen[P.WHOLE] and "D-agree-72" in seen[P.NONE]
    assert {"D-run-2", "D-run-31", "D-run-32", "D-agree-40-typed"} <= set(seen[P.FUSED])


WANT_PATH = {"A-bucket-4097": P.WHOLE, "E-agree-12": P.WHOLE, "D-agree-72": P.NONE, "H-two-parts": P.NONE}


@pytest.mark.parametrize("cid", [c[0] for c in P.cases() if c[0] != "P-flagged-between"])
def test_case_path(cid):
    """Every new case runs fused; of the lists' cases the ones named above do not."""
    m = P.model_of(cid)
    assert P.place_path(m["stats"]) == WANT_PATH.get(cid, P.FUSED), m["stats"]
    assert not any(m["host"])


def test_path_1_cases_with_ties():
    for cid in ("D-run-2", "D-run-31", "D-run-32", "D-agree-40-typed", "P-two-parts-direct"):
        st = P.model_of(cid)["stats"]
        assert st["first_ties"] > 0 and st["left_runs"] == 0, cid
    assert P.model_of("D-agree-40-typed")["modes"][0] != S.FULL


@pytest.mark.parametrize("cid,size,pos,cls,chunk", P.PAIRS, ids=[p[0] for p in P.PAIRS])
def test_pair_sits_where_the_case_says(cid, size, pos, cls, chunk):
    """The tied slots are pos and pos + 1 of a chunk of the named class that
    starts at slot 0, and the stream's last three slots."""
    m = P.model_of(cid)
    fr = m["rounds"][0]
    assert m["modes"] == [S.FULL]
    nsub = fr["nsub"]
    b, e, c, _ = fr["chunks"][0]
    assert (b, e) == (chunk or (0, nsub)) and c == cls
    assert fr["slots"].tolist() == [pos, pos + 1, nsub - 3, nsub - 2, nsub - 1]
    assert int(fr["hist"][(1 << 6) | (S.Y >> 2)]) == size
    # the pair is in the text in the order opposite to the sorted one
    pair = next(g for g in fr["groups"] if len(g) == 2)
    order, _ = S.ladder_order(P.texts_of(cid)[0])
    assert order.index(int(max(pair))) < order.index(int(min(pair)))


def test_pair_positions_cover_the_sorters():
    """First two, last two, and IPT t + IPT - 1 / IPT t + IPT for 256 x 4,
    512 x 4 and 512 x 8; the last slots of a tiny chunk are the 0xFB group's."""
    by_cls = {}
    for _, size, pos, cls, chunk in P.PAIRS:
        by_cls.setdefault(cls, set()).add("first" if pos == 0 else "last" if pos == size - 2 else
                                           "ipt" if (pos + 1) % (8 if cls == 2 else 4) == 0 else "?")
    assert by_cls == {0: {"first", "ipt"}, 1: {"first", "ipt", "last"}, 2: {"first", "ipt", "last"}}


def test_chunk_fill_sizes():
    sizes = set()
    for cid in ("A-bucket-1025", "A-bucket-2048", "A-bucket-2049", "A-bucket-4096", "A-bucket-4097", "A-multi-1024",
                "A-multi-1025", "A-multi-2048", "P-chunk-1"):
        sizes |= {e - b for b, e, _, _ in P.model_of(cid)["rounds"][0]["chunks"]}
    assert {1, 1024, 1025, 2048, 2049, 4096, 4097} <= sizes


@pytest.mark.parametrize("mode", (S.SORT_A, S.SORT_B))
def test_wrap_rows(mode):
    cid = "P-wrap-sort-a" if mode == S.SORT_A else "P-wrap-sort-b"
    m = P.model_of(cid)
    assert m["modes"] == [mode] * 5
    texts = P.texts_of(cid)
    n = len(texts[0])
    placed = M.scan_view(texts[0], mode)[1]
    assert not placed[[0, 1, 2, 3] + list(range(n - 8, n))].any()
    for k in range(4):
        T = texts[1 + k]
        placed = M.scan_view(T, mode)[1]
        live = placed & M.live_rule(T, mode)
        assert not placed[k] and placed[np.arange(k - 6, k)].all() and live[np.arange(k - 5, k)].all(), k


def test_stream_calls():
    for cid, count in (("P-two-streams", 2), ("P-nine-streams", 9)):
        texts = P.texts_of(cid)
        assert len(texts) == count and len({len(t) for t in texts}) == count
        assert len({len(np.unique(t)) for t in texts}) >= min(count, 5)
    assert {S.SORT_A, S.SORT_B} <= set(P.model_of("P-nine-streams")["modes"])
    m = P.model_of("P-full-beside-ordinary")
    assert m["modes"] == [S.SORT_A, S.FULL, S.SORT_B, S.SORT_A]


def test_flagged_between():
    m = P.model_of("P-flagged-between")
    assert m["host"] == [False, True, False] and P.place_path(m["stats"]) == P.FUSED
    assert S.FULL not in (m["modes"][0], m["modes"][2])


def test_live_slot_cases():
    def live(cid):
        T = P.texts_of(cid)[0]
        mode = P.model_of(cid)["modes"][0]
        placed = M.scan_view(T, mode)[1]
        return mode, int((placed & M.live_rule(T, mode)).sum()), int(placed.sum())
    assert live("P-no-live-slot")[:2] == (S.SORT_A, 0)
    mode, nl, npl = live("P-live-rising")
    assert mode == S.SORT_A and nl > 0.85 * npl
    mode, nl, npl = live("P-live-falling")
    assert mode == S.SORT_B and nl > 0.85 * npl


def test_parts_cases():
    """List H's second part holds a run of 33 copies that agree on 18 bytes:
    by the rule its call restarts (path 0).  The multi entry on the fused
    path is H's stream without that run."""
    m = P.model_of("P-two-parts-direct")
    assert len(m["texts"]) == 2 and m["stats"]["first_ties"] > 0
    assert len(P.model_of("H-two-parts")["texts"]) == 2
