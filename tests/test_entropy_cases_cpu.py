"""The premises of test_entropy_hist_gpu.py, without a GPU.

(a) Two independent definitions of the bigram histogram agree on every case of
    tests/entropy_cases.py: the oracle's counting sort (lfm_oracle.c
    lfmo_entropy_chunk, read through oracle.bigram_hist) and the numpy sort
    definition (hist_by_sort of test_entropy_partner_cpu.py).
(b) Every case has the property it is named for.
(c) The cases discriminate: a partner model with one seam of the kernels'
    design broken (MUTANTS) counts a different histogram on at least one case,
    and on at least one case with a full chunk its entropy stays inside the
    tolerance of the float tests (1e-5 * max(1, H), tests/test_gpu.py) -- the
    exact comparison sees what that tolerance cannot."""
import os
import re

import numpy as np
import pytest

import entropy_cases as E
from conftest import PKG
from test_entropy_partner_cpu import hist_by_partner, hist_by_sort

CASES = E.all_cases()
SEG = E.K["kSeg"]


def test_case_constants_are_the_kernels():
    src = open(os.path.join(PKG, "csrc", "lfm_entropy.hip")).read()
    for text in ("kChunkPix = %d;" % E.K["kChunkPix"], "kChunkBytes = 2 * kChunkPix;", "kSub = %d;" % E.K["kSub"],
                 "kSeg = 4 * kSub;", "kSegMax = (kChunkBytes + kSeg - 1) / kSeg;"):
        assert "constexpr uint32_t " + text in src, text
    assert SEG == 4 * E.K["kSub"] and E.K["kSegMax"] == (E.CHUNK_BYTES + SEG - 1) // SEG
    assert E.CHUNK_BYTES == 54 * SEG + 15264
    assert 15264 - 3 * E.K["kSub"] == 2976 and 2976 % E.WINDOW == E.WINDOW // 2
    assert re.search(r"job = \(blk >> 5\) \* 8 \+ \(blk & 7\)", src)
    import lfm_oracle
    assert lfm_oracle.CHUNK_PIX == E.K["kChunkPix"]


def test_case_names_are_unique_and_sizes_cover_the_tails():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    tails = {2 * min(n - q, E.K["kChunkPix"]) % 16 for n in E.SIZES for q in range(0, n, E.K["kChunkPix"])}
    assert tails == set(range(0, 16, 2))
    assert {1, 7, 449999, 450000, 450001, 1000003, 2, 8, 9, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 24577,
            450007, 900000} <= set(E.SIZES)
    assert sorted((c.ncand, c.claims["nchunks"]) for c in E.job_cases()) == sorted(E.JOB_SHAPES)


# ------------------------------------------------------ the partner model --
MUTANTS = ("chunk_start_val_from_previous_chunk", "far_link_dropped", "sentinel_bigram_dropped", "end_of_L_counted",
           "key0_closed_by_next_key", "tail_bytes_as_zeros")


def links(c):
    """The same-key links of a chunk: every position's next occurrence of its
    byte (-1: none), and per present key (ascending) its first and last
    position."""
    order = np.argsort(c, kind="stable")
    ks = c[order]
    same = ks[1:] == ks[:-1]
    nxt = np.full(len(c), -1, np.int64)
    nxt[order[:-1][same]] = order[1:][same]
    head, tail = np.concatenate([[True], ~same]), np.concatenate([~same, [True]])
    return nxt, ks[head].astype(np.int64), order[head], order[tail]


def model_hist(c, mutant=None, prev_last=0, lk=None):
    """hist_by_partner's rule (test_entropy_partner_cpu.py), vectorised: bin
    (c[i-1] << 8) | partner[i] per position, partner = the val of the next
    occurrence of c[i]; the last occurrence of a key takes the first val of
    the next present key (key 0's the sentinel's val c[S-1]); the last element
    of L has no bigram; the sentinel's bigram closes key 0.  `mutant` breaks
    one seam the way a kernel bug would."""
    S = len(c)
    if mutant == "tail_bytes_as_zeros" and S % 16:  # load16's zero fill reaching below S
        c, lk = c.copy(), None
        c[S - S % 16:] = 0
    c = c.astype(np.int64)
    nxt, keys, firsts, lasts = lk or links(c)
    val = np.concatenate([[0], c[:-1]])
    if mutant == "chunk_start_val_from_previous_chunk":
        val[0] = prev_last
    partner = np.where(nxt >= 0, val[nxt], -1)
    if mutant == "far_link_dropped":  # more than one segment without the byte between the two
        i = np.flatnonzero(nxt >= 0)
        partner[i[nxt[i] // SEG - i // SEG > 2]] = 0
    fv = val[firsts]
    close = np.concatenate([fv[1:], [-1]])  # the first val of the next present key
    sentinel_next = close[0] if keys[0] == 0 else fv[0]
    if keys[0] == 0 and not (mutant == "key0_closed_by_next_key" and close[0] >= 0):
        close[0] = c[-1]
    partner[lasts[close >= 0]] = close[close >= 0]
    keep = np.ones(S, bool)
    if mutant == "end_of_L_counted":
        partner[lasts[close < 0]] = 0
    else:
        keep[lasts[close < 0]] = False
    h = np.bincount((val[keep] << 8) | partner[keep], minlength=65536)
    if sentinel_next >= 0 and mutant != "sentinel_bigram_dropped":
        h[(c[-1] << 8) | sentinel_next] += 1
    return h


def entropy64(h, S):
    """sum_bwt_GPU's sum in float64: bins below 0xFFFF, P = h / S."""
    p = h[:65535][h[:65535] > 0] / float(S)
    return float(-(p * np.log(p)).sum())


@pytest.mark.parametrize("kind", ["skewed", "uniform", "two_bytes", "zeros", "no_zero", "top_key_first"])
def test_vector_model_is_the_position_model(kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    for S in (1, 2, 3, 17, 64, 65, 200, 999, 40000):
        if kind == "skewed":
            c = np.minimum(np.abs(rng.normal(0, 6, S)).astype(np.int64), 255)
        elif kind == "uniform":
            c = rng.integers(0, 256, S)
        elif kind == "two_bytes":
            c = rng.choice([7, 200], S)
        elif kind == "zeros":
            c = np.zeros(S, np.int64)
        elif kind == "no_zero":
            c = rng.integers(1, 4, S)
        else:
            c = rng.integers(0, 9, S)
            c[0] = 250
        c = c.astype(np.uint8)
        assert np.array_equal(model_hist(c), hist_by_partner(c.astype(np.int64))), (kind, S)
        assert model_hist(c).sum() == S


# ------------------------------------------------------------- the cases --
def check_claims(case, cands, true):
    """`true`: the sort definition's histograms of candidate 0, per chunk."""
    chunks = E.chunks_of(cands[0])
    c, claims = chunks[0], case.claims
    assert len(chunks) == claims["nchunks"] == len(true)
    assert [len(x) for x in chunks[:-1]] == [E.CHUNK_BYTES] * (len(chunks) - 1)
    for b, ps in claims.get("positions", {}).items():
        assert np.flatnonzero(c == b).tolist() == ps, hex(b)
    for b, segs in claims.get("segments", {}).items():
        assert np.unique(np.flatnonzero(c == b) // SEG).tolist() == segs, hex(b)
    if "keys" in claims:
        assert np.unique(c).tolist() == claims["keys"]
    for b in claims.get("absent", []):
        assert b not in c
    if claims.get("sentinel_alone"):
        first = int(np.argmax(c == c.min()))
        assert c.min() > 0 and true[0][(int(c[-1]) << 8) | (int(c[first - 1]) if first else 0)] >= 1
    if "end_of_L" in claims:
        end = None if c.max() == 0 else int(np.flatnonzero(c == c.max())[-1])
        assert end == claims["end_of_L"]
    if "bins" in claims:
        assert {int(b): int(true[0][b]) for b in np.flatnonzero(true[0])} == claims["bins"]
    for q, b in enumerate(claims.get("seam_bytes", [])):
        whole = np.concatenate(chunks)
        assert chunks[q][-1] == b != 0 and int((whole == b).sum()) == 1
        row = slice(b << 8, (b << 8) + 256)
        assert int(true[q][row].sum()) == 1, "b is a val once in its own chunk: the sentinel's"
        assert int(true[q][b::256].sum()) == 1, "b is a partner once: it closes key 0"
        if q + 1 < len(chunks):
            assert not true[q + 1][row].any() and not true[q + 1][b::256].any(), "the next chunk starts with val 0"
    if claims.get("distinct"):
        assert len({x.tobytes() for x in cands}) == case.ncand > 1
        assert [x.ctypes.data - cands[0].ctypes.data for x in cands] == [2 * k for k in range(case.ncand)]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_histograms_agree_and_case_is_what_it_claims(oracle, case):
    cands = E.candidates(case)
    for k, cand in enumerate(cands):
        chunks = E.chunks_of(cand)
        true = [hist_by_sort(c.astype(np.int64)) for c in chunks]
        got = oracle.bigram_hist(cand)
        assert got.shape == (len(chunks), 65536) and got.dtype == np.uint32
        for q, c in enumerate(chunks):
            assert true[q].sum() == len(c)
            assert np.array_equal(got[q], true[q]), (k, q)
            if k == 0:
                assert np.array_equal(model_hist(c), true[q]), q
        if k == 0:
            check_claims(case, cands, true)


def test_tie_frames_tie_in_the_oracle(oracle):
    for name, frame, fam, tied, chosen in E.tie_frames():
        assert frame.shape == (E.TIE_H, E.TIE_W) and frame.dtype == np.uint16
        k, ent = oracle.select(frame, E.TIE_T, fam)
        assert [i for i in range(8) if ent[i] == ent.min()] == tied, (name, ent)
        assert k == chosen == max(tied), name


def test_every_mutant_is_caught_and_hides_inside_the_float_tolerance():
    """One pass over the one-candidate cases: per mutant, the cases whose
    histogram it changes, and among those with a full chunk the ones whose
    float64 entropy moves by no more than the float tests allow."""
    caught = {m: [] for m in MUTANTS}
    quiet = {m: [] for m in MUTANTS}
    for case in CASES:
        if case.ncand > 1:
            continue  # (the job-mapping cases are about which block counts which job)
        chunks = E.chunks_of(E.candidates(case)[0])
        lks = [links(c.astype(np.int64)) for c in chunks]
        true = [model_hist(c, lk=lk) for c, lk in zip(chunks, lks)]
        H = sum(entropy64(h, len(c)) for h, c in zip(true, chunks))
        for m in MUTANTS:
            hm = [model_hist(c, m, int(chunks[q - 1][-1]) if q else 0, lk) for q, (c, lk) in enumerate(zip(chunks, lks))]
            if all(np.array_equal(a, b) for a, b in zip(hm, true)):
                continue
            caught[m].append(case.name)
            dH = abs(sum(entropy64(h, len(c)) for h, c in zip(hm, chunks)) - H)
            if case.npix >= E.K["kChunkPix"] and dH <= 1e-5 * max(1.0, H):
                quiet[m].append((case.name, dH, H))
    for m in MUTANTS:
        print(m, "caught by", len(caught[m]), "cases; inside the float tolerance on", len(quiet[m]),
              ["%s dH=%.2e H=%.3f" % q for q in quiet[m][:4]])
    for m in MUTANTS:
        assert caught[m], "no case sees mutant %s: a case is missing" % m
        assert quiet[m], "mutant %s moves the entropy past 1e-5 * max(1, H) on every full-chunk case" % m
