"""The premises of test_bwt_sort_seams_gpu.py, without a GPU: the model of
tests/bz2_sort_cases.py restates the encoder's constants, its ladder ends in
the order of a naive sort on random and motif texts (every rung met), and each
case of lists A to H has the property it is named for."""
import os
import re

import numpy as np
import pytest

import bz2_sort_cases as S
from conftest import PKG


def test_model_constants_are_the_kernels():
    src = open(os.path.join(PKG, "csrc", "lfm_bzip2.hip")).read()
    for name, val in S.K.items():
        got = re.search(r"\b%s = (\d+)" % name, src)
        assert got and int(got.group(1)) == val, name
    assert re.search(r"kSmallCap = kCsThreads \* kCsItems, kBigCap = kBigThreads \* kBigItems", src)
    assert re.search(r"if \(tcut >= kMaxCuts\)", src), "the cut overflow goes to the host library"
    caps = open(os.path.join(PKG, "csrc", "lfm_bz_caps.h")).read()
    assert "block_bytes + block_bytes / 4 + 64, 256" in caps
    import lfm
    assert lfm.BWT_STATS == S.STATS


# ------------------------------------------------------------ the ladder --
ALPHABETS = (2, 3, 4, 16, 256)


def ladder_texts(count, seed):
    """Seeded texts of 2..400 bytes: random ones over 2, 3, 4, 16 and 256
    symbols; every fourth built of a repeated motif with a few bytes changed
    (runs longer than 32, agreements past 72 bytes, near-periodic and periodic
    texts); and every sixteenth 33..36 copies of a word of 8..22 bytes between
    distinct bytes, padded with random bytes until 4 x ties <= N, so that the
    text rounds run and end after one, two or three (these are up to 2 000
    bytes long: 33 copies of 23 bytes do not fit 400)."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        a = ALPHABETS[k % len(ALPHABETS)]
        n = int(rng.integers(2, 401))
        if k % 16 == 9:
            g, L = int(rng.integers(33, 37)), int(rng.integers(8, 23))
            w = S.word(L, k)
            marks = rng.permutation(np.arange(8, 250))[:g].tolist()
            body = b"".join(w + bytes([x]) for x in marks)
            yield np.frombuffer(body + S.fillers(rng, 4 * g * (L - 7), after=body[-1]), np.uint8).copy()
            continue
        if k % 4 == 3:
            motif = rng.integers(0, a, int(rng.integers(1, 40)))
            T = np.resize(motif, n)
            for _ in range(int(rng.integers(0, 4))):
                T[int(rng.integers(0, n))] = int(rng.integers(0, a))
        else:
            T = rng.integers(0, a, n)
        T = T.astype(np.uint8)
        if a < 256 and k % 2:
            T = (T * (255 // (a - 1))).astype(np.uint8)
        yield T


@pytest.mark.parametrize("part", range(4))
def test_ladder_ends_in_the_naive_order(part):
    """About 2 000 texts in all: the order by the bytes the ladder compared is
    the naive order of the sorted rotations, nothing is left tied unless the
    text is periodic, and the model flags exactly the periodic texts."""
    seen = dict.fromkeys(("direct", "left", "text1", "text2", "text3", "restart", "rank0", "gathered", "doubling",
                          "periodic", "skip_rounds"), 0)
    for T in ladder_texts(500, 0x50A7 + part):
        order, m = S.ladder_order(T)
        st = m["stats"]
        assert (order is None) == S.is_periodic(T) == bool(st["flag_periodic"])
        if order is not None:
            mode = S.FULL if m["it_full"] else m["modes"][0]
            assert order == S.naive_order(T, mode)
        seen["direct"] += st["first_ties"] > 0 and st["left_runs"] == 0
        seen["left"] += st["left_runs"] > 0
        if st["text_rounds"]:
            seen["text%d" % st["text_rounds"]] += 1
        seen["restart"] += st["restarted"]
        seen["rank0"] += st["rank_form"] == S.RANK0
        seen["gathered"] += st["rank_form"] == S.RANK_GATHERED
        seen["doubling"] += st["doubling_rounds"] > 0
        seen["periodic"] += st["flag_periodic"]
        seen["skip_rounds"] += st["left_runs"] > 0 and st["text_rounds"] == 0
    print(seen)
    assert all(seen[k] for k in seen), seen


# ------------------------------------------------------------- the cases --
def facts(cid, rows):
    m = S.model_of(cid)
    texts = [S.text_of(r) for r in rows]
    return m, texts


def group_agreements(T, groups):
    """(size, longest agreement of two members) per tied group."""
    out = []
    width = 4 * S.DIRECT_BYTES
    for g in groups:
        P = S.prefixes(T, g, width)
        P = P[np.lexsort(P.T[::-1])]  # the longest agreement is between neighbours in sorted order
        diff = P[1:] != P[:-1]
        out.append((len(g), int(np.where(diff.any(1), diff.argmax(1), width).max())))
    return out


CASES = S.a_cases() + S.c_cases() + S.d_cases() + S.e_cases() + S.f_cases() + S.g_cases()


@pytest.mark.parametrize("cid,rows,level,want", CASES, ids=[c[0] for c in CASES])
def test_case_has_the_property_it_is_named_for(cid, rows, level, want):
    m, texts = facts(cid, rows)
    st, fr = m["stats"], m["attempts"][0]["first"]
    print(cid, st)
    assert len({len(r) for r in rows}) == 1
    assert all(len(t) < S.nblock_max(level) for t in texts)
    for k in S.STATS:
        if k in want:
            assert st[k] == want[k], (k, st[k], want[k])
    assert [i for i, h in enumerate(m["host"]) if h] == want.get("periodic", [])
    assert [i for i, t in enumerate(texts) if S.is_periodic(t)] == want.get("periodic", [])
    f0 = fr[0]
    if "bucket" in want:
        assert want["bucket"] in f0["hist"].tolist() and m["modes"][0] == S.FULL
        single = [c for c in f0["chunks"] if c[1] - c[0] == want["bucket"] and c[3] == 1]
        assert bool(single) == (want["cls"] is not None)
        if want["cls"]:
            assert S.STATS[single[0][2]] == want["cls"]
    if "chunk" in want:
        size, multi = want["chunk"]
        assert [c for c in f0["chunks"] if c[1] - c[0] == size and (c[3] > 1) == multi]
    if "first_cut" in want:
        assert f0["cuts"][0] == want["first_cut"] and f0["chunks"][0][:2] == (0, want["first_cut"])
    if "dup_cut" in want:
        assert f0["cuts"].count(want["dup_cut"]) == 2
    if "nchunks" in want:
        assert len(f0["chunks"]) == want["nchunks"] and not f0["cuts"]
    if "n" in want:
        assert len(texts[0]) == want["n"]
    if "wrap_tie" in want:
        n = len(texts[0])
        assert any(int(i) + 8 > n for g in f0["groups"] for i in g), "a tied key reads past the end of the text"
        assert any(int(i) < 5 for g in f0["groups"] for i in g)
    if "min_ties" in want:
        assert st["first_ties"] >= want["min_ties"]
    ga = [x for s in fr for x in group_agreements(texts[s], fr[s]["groups"])] if len(rows) <= 4 and \
        st["first_ties"] < 1000 else []
    if "max_run" in want:
        assert max(g for g, _ in ga) == max(3, want["max_run"]) and want["max_run"] in [g for g, _ in ga]
    if "max_agree" in want:
        # (the three rotations that start with eight 0xFB agree on 9 bytes)
        assert want["max_agree"] in [a for _, a in ga] and max(a for _, a in ga) == max(9, want["max_agree"])
    if "left" in want:
        assert (st["left_runs"] > 0) == want["left"]
        assert want["left"] == any(g > S.K["kTieRunMax"] or a >= S.DIRECT_BYTES for g, a in ga)
    if "resolved_too" in want:
        assert any(g <= S.K["kTieRunMax"] and a < S.DIRECT_BYTES for g, a in ga)
    if "typed" in want:
        assert m["modes"][0] != S.FULL
    if "same_key" in want:
        keys = {int(S.keys8(texts[s])[fr[s]["groups"][0][0]]) for s in fr}
        assert len(keys) == 1 and all(len(fr[s]["groups"]) == 1 for s in fr)
    if "tied_slots" in want:
        assert set(want["tied_slots"]) <= set(f0["slots"].tolist())
    if "nsub_mod16" in want:
        assert f0["nsub"] % 16 == want["nsub_mod16"]
    if "last_slot_tied" in want:
        assert f0["slots"][-1] == f0["nsub"] - 1
    if "streams" in want:
        assert len(rows) == want["streams"]
        tied = [fr[s]["first_ties"] > 0 for s in range(len(rows))]
        assert any(tied) and not all(tied)


def test_class_count_batches():
    """1, 7, 8 and 9 streams with one chunk each in the small, big and
    segmented class: 8 * ceil(nc / 8) workgroups, c >= nch for 1, 7 and 9."""
    for cid, rows, level, want in S.a_cases():
        if cid.startswith("A-classes"):
            assert len(rows) == want["chunks_segmented"]


def test_b_overflow_premise():
    """List B: below nblockMAX at level 9; the model counts at least kMaxCuts
    cut entries, and the chunks of the unfixed rule (the entries past the kept
    ones dropped, the last chunk to nsub) end in one of many buckets, above
    kBigCap: the segmented sort's class.  The siblings need exactly 1 022,
    1 023 and 1 024 entries."""
    for cid, rows, level, want in S.b_cases():
        T = S.text_of(rows[0])
        assert level == 9 and len(T) < S.nblock_max(9) and S.kernel_mode(T) == S.FULL and not S.is_periodic(T[:4096])
        key = S.keys8(T)
        hist = np.bincount((key >> np.uint64(50)).astype(np.int64), minlength=1 << 14)
        cuts = S.cut_entries(hist)
        print(cid, len(T), "cut entries", len(cuts), "buckets", int((hist > 0).sum()), "above kChunk",
              int((hist > S.K["kChunk"]).sum()))
        m = S.model_of(cid)
        assert m["host"] == [len(cuts) >= S.K["kMaxCuts"]]
        if "cuts" in want:
            assert len(cuts) == want["cuts"]
            if not m["host"][0]:
                assert sum(m["stats"][k] for k in S.STATS[:4]) <= S.K["kMaxCuts"]
        else:
            assert len(cuts) >= want["min_cuts"] and len(cuts) == 1457
            kept = cuts[:S.K["kMaxCuts"] - 1]
            ends = np.cumsum(hist[hist > 0])
            tail_buckets = int((ends > kept[-1]).sum())
            assert len(T) - kept[-1] > S.BIG_CAP and tail_buckets > 1
            print("tail chunk of the unfixed rule: %d rotations, %d buckets" % (len(T) - kept[-1], tail_buckets))
            assert (len(T) - kept[-1], tail_buckets) == (264993, 219)


def test_g_swap_pair():
    first, second = S.g_swap_pair()
    tied = []
    for rows in (first, second):
        m = S.model([S.text_of(r) for r in rows], S.call_cap(rows, 2))
        tied.append([m["rounds"][s]["first_ties"] > 0 for s in range(len(rows))])
    assert len(first) == len(second) == 1025 and {len(r) for r in first + second} == {48}
    assert all(a != b for a, b in zip(*tied))


def test_h_two_parts():
    """List H: two parts at level 1; the repeat crosses the cut; the second
    part has a left run and the call runs text rounds."""
    raw, m = S.h_model()
    texts = m["texts"]
    assert len(raw) == S.H_BLOCK and len(texts) == 2 and len(texts[0]) == S.nblock_max(S.H_LEVEL)
    cut = len(texts[0])
    full = S.text_of(raw)
    rep = full[cut - 30:cut + 30].tobytes()
    assert full.tobytes().count(rep) == 2
    fr = m["attempts"][0]["first"]
    assert fr[1]["left_runs"] > 0 and m["stats"]["text_rounds"] == 3 and not any(m["host"])
    print(m["stats"])
