"""Calls aimed at the tied list the placing chunk sorts of the GPU bzip2
encoder's BWT write themselves (bwt_chunk_sort<.., PLACE>: blocked load, sa
stored at tied slots only, the slots appended per workgroup), and at the
fallback that sorts again without PLACE when a run is left.  Shared by
test_bwt_tied_list_cpu.py (which proves from the first-round model of
bz2_sort_cases.py that every case hits the seams it is listed for) and
test_bwt_tied_list_gpu.py (bytes, flags, stats and place path against that
model).  TEST INFRASTRUCTURE ONLY.

The streams are random texts over a small alphabet (at most 20 000 bytes, at
most 8 per call), found by a seeded search: `search()` below walks the seeds
of each family, labels every stream with the seams it hits (`labels`), and
keeps the first stream per seam.  Its result is pinned in CASES; the CPU test
recomputes the labels.

A stream: (family, seed).  A family: (alphabet, raw length, plant) -- plant g > 0
puts g copies of one 8-byte word (drawn from the alphabet) into the text, for
the runs of kTieRunMax = 32 and of 33 that a random text does not hold.

Labels (cls: tiny = 256 x 4, small = 512 x 4, big = 512 x 8 sorter; IPT its
items per thread; slots are in-chunk sorted slots):
  len%IPT=r/cls      a chunk of that class with m % IPT == r
  len=m              a chunk of exactly m rotations
  single-big         a single-bucket chunk of 2 049 .. 4 096 rotations
  pair-thread/cls    a tied run of 2 on slots IPT t + IPT - 1 | IPT t + IPT
  run3-thread/cls    a run of 3 over such a boundary
  pair-wave/cls      a run of 2 on slots 64 IPT - 1 | 64 IPT
  run3-wave/cls      a run of 3 over that boundary
  pair-first/cls     a run of 2 on the first two slots of a chunk
  pair-last/cls      a run of 2 on the last two slots of a chunk with m % IPT != 0
  run32              a run of 32 (the longest tie_runs_direct takes)
  run33              a run of 33: left_runs 1, the sorts run again
  run-rot0           a run that holds rotation 0 (origPtr)
  two-chunks         tied runs in two chunks of one stream
and per call: streams3 (tied runs in three streams or more).
"""
import functools

import numpy as np

import bz2_sort_cases as S

SPREAD6 = (3, 44, 85, 126, 167, 208)  # six first bytes, six values of the next byte's top bits: 36 buckets
FAMILIES = {
    # four buckets (the second byte's top six bits are 0), of about 1, 2, 3 and 0 tenths
    # of the text: single-bucket chunks
    "q16h": ((0, 1, 2, 3), 16400, 0),  # the third bucket about 4 096
    "q16": ((0, 1, 2, 3), 16000, 0),   # ~ 1 400, 2 700, 4 000: both 4-item sorters' big neighbour
    "q12": ((0, 1, 2, 3), 12000, 0),   # the second bucket about 2 048
    "q9": ((0, 1, 2, 3), 9000, 0),
    "q7": ((0, 1, 2, 3), 7400, 0),
    # 36 buckets of a few hundred: multi-bucket chunks, tiny ones between and at the end
    "s20": (SPREAD6, 20000, 0),
    "s12": (SPREAD6, 12000, 0),
    "s5": (SPREAD6, 5000, 0),
    "s20x32": (SPREAD6, 20000, 32),
    "s20x33": (SPREAD6, 20000, 33),
}
CLS = ("tiny", "small", "big")
IPT = (4, 4, 8)
LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 4096)


@functools.lru_cache(maxsize=None)
def raw_of(family, seed):
    alpha, n, plant = FAMILIES[family]
    rng = np.random.default_rng([seed, n, plant])
    T = np.asarray(alpha, np.uint8)[rng.integers(0, len(alpha), n)]
    if plant:
        w = T[:8].copy()
        gap = n // (plant + 1)
        for j in range(1, plant):  # the word stands at 0 already
            at = j * gap + int(rng.integers(0, gap - 16))
            T[at:at + 8] = w
    return T.tobytes()


@functools.lru_cache(maxsize=None)
def first_round_of(family, seed):
    T = S.text_of(raw_of(family, seed))
    mode = S.mode_of(T)
    return T, mode, S.first_round(T, mode)


def runs_of(fr):
    """(chunk index, in-chunk slot, length, holds rotation 0) of every tied run."""
    out, at = [], 0
    begins = np.array([c[0] for c in fr["chunks"]])
    for g in fr["groups"]:
        slot = int(fr["slots"][at])
        assert fr["slots"][at:at + len(g)].tolist() == list(range(slot, slot + len(g)))
        at += len(g)
        ci = int(np.searchsorted(begins, slot, side="right")) - 1
        b, e = fr["chunks"][ci][:2]
        assert b <= slot and slot + len(g) <= e, "a run leaves its chunk"
        out.append((ci, slot - b, len(g), bool((np.asarray(g) == 0).any())))
    assert at == len(fr["slots"])
    return out


def labels(family, seed):
    """The seams one stream hits; empty unless it stays on the device and
    every chunk goes through the three sorters."""
    _, _, fr = first_round_of(family, seed)
    if fr["overflow"] or any(c[2] == 3 for c in fr["chunks"]):
        return frozenset()
    lab = set()
    for b, e, c, nb in fr["chunks"]:
        m = e - b
        lab.add("len%%IPT=%d/%s" % (m % IPT[c], CLS[c]))
        if m in LENGTHS:
            lab.add("len=%d" % m)
        if c == 2 and nb == 1:
            lab.add("single-big")
    runs = runs_of(fr)
    for ci, p, g, rot0 in runs:
        b, e, c, _ = fr["chunks"][ci]
        m, ipt = e - b, IPT[c]
        inner = range(p, p + g - 1)  # j: the run holds slots j and j + 1
        if g in (2, 3):
            name = "pair" if g == 2 else "run3"
            if any((j + 1) % ipt == 0 for j in inner):
                lab.add("%s-thread/%s" % (name, CLS[c]))
            if 64 * ipt - 1 in inner:
                lab.add("%s-wave/%s" % (name, CLS[c]))
        if g == 2 and p == 0:
            lab.add("pair-first/" + CLS[c])
        if g == 2 and p + 2 == m and m % ipt:
            lab.add("pair-last/" + CLS[c])
        if g == S.K["kTieRunMax"]:
            lab.add("run32")
        if g == S.K["kTieRunMax"] + 1:
            lab.add("run33")
        if rot0:
            lab.add("run-rot0")
    if len({r[0] for r in runs}) >= 2:
        lab.add("two-chunks")
    if fr["left_runs"]:
        lab.add("left")
    return frozenset(lab)


# every seam the suite must hit ("len=4096": see CASES)
def required():
    req = set()
    for c, ipt in zip(CLS, IPT):
        req |= {"len%%IPT=%d/%s" % (r, c) for r in ((0, 1, 2, 3, 5, 7) if ipt == 8 else (0, 1, 2, 3))}
        req |= {"%s/%s" % (k, c) for k in ("pair-thread", "run3-thread", "pair-wave", "run3-wave", "pair-first",
                                           "pair-last")}
    req |= {"len=%d" % m for m in LENGTHS if m != 4096}
    req |= {"single-big", "run32", "run33", "run-rot0", "two-chunks", "streams3"}
    return req


def chunk_lengths(family, seed):
    """The chunk lengths alone (first_round's cuts without its tie groups)."""
    T = S.text_of(raw_of(family, seed))
    mode = S.mode_of(T)
    srt = np.arange(len(T)) if mode == S.FULL else np.flatnonzero(~S.scan_view(T, mode)[1])
    key = S.keys8(T)[srt]
    hist = np.bincount((key >> np.uint64(64 - S.K["kBucketBits"])).astype(np.int64), minlength=1 << S.K["kBucketBits"])
    bounds = [0] + S.cut_entries(hist) + [len(srt)]
    return [e - b for b, e in zip(bounds[:-1], bounds[1:]) if e > b]


def search(all_seams=40, max_seed=1500):
    """The search CASES was pinned from: seeds 0 .. all_seams - 1 of every
    family for every seam, further seeds only where chunk_lengths shows one of
    LENGTHS that is still open; the first stream per seam is kept.  A stream
    with a run left counts for run33 alone, and only with exactly one such run.
    Returns [(family, seed, seams it was kept for)] and the seams not found."""
    open_ = (required() | {"len=4096"}) - {"streams3"}
    found = []
    for seed in range(max_seed):
        for fam in FAMILIES:
            if seed >= all_seams and not {"len=%d" % m for m in chunk_lengths(fam, seed)} & open_:
                continue
            lab = labels(fam, seed)
            if "left" in lab:
                ok = first_round_of(fam, seed)[2]["left_runs"] == 1 and "run33" in lab
                lab = {"run33"} if ok else set()
            hit = lab & open_
            if hit:
                found.append((fam, seed, sorted(hit)))
                open_ -= hit
        if not open_:
            break
    return found, open_


# (id, the call's streams, seams the call is kept for) -- the streams as search()
# found them, those of one raw length together, at most 8 per call.
# The search found every seam, the single-bucket chunk of exactly 4 096 too
# (q16h, seed 389).  L-fallback is put together by hand from its finds: the
# stream with the run of 33 beside three of the same length whose ties settle.
CASES = (
    ("L-q16h", (("q16h", 1), ("q16h", 11), ("q16h", 26), ("q16h", 389)),
     ("len%IPT=1/big", "pair-first/small", "run3-wave/big", "run3-wave/small", "len=4096", "streams3")),
    ("L-q16", (("q16", 0), ("q16", 1), ("q16", 6)),
     ("len%IPT=2/big", "len%IPT=3/small", "len%IPT=3/tiny", "pair-last/small", "pair-thread/big", "pair-thread/small",
      "run3-thread/big", "run3-thread/small", "single-big", "two-chunks", "len%IPT=0/big", "pair-last/big", "streams3")),
    ("L-q12", (("q12", 0), ("q12", 1), ("q12", 2), ("q12", 24), ("q12", 61)),
     ("len%IPT=1/small", "len%IPT=2/tiny", "len%IPT=3/big", "pair-first/big", "run-rot0", "pair-wave/big",
      "pair-wave/small", "len=2048", "len=2047")),
    ("L-s12", (("s12", 1), ("s12", 3), ("s12", 20)), ("pair-first/tiny", "len=1023", "len=1024")),
    ("L-q9", (("q9", 0), ("q9", 1), ("q9", 32)),
     ("len%IPT=0/tiny", "len%IPT=5/big", "pair-thread/tiny", "run3-thread/tiny", "len%IPT=7/big", "run3-wave/tiny")),
    ("L-q7", (("q7", 0), ("q7", 17)), ("len%IPT=0/small", "len%IPT=1/tiny", "len=1", "pair-wave/tiny")),
    ("L-s5", (("s5", 6),), ("pair-last/tiny",)),
    ("L-s20", (("s20", 0), ("s20x32", 1), ("s20x33", 73)), ("len%IPT=2/small", "run32", "len=1025")),
    ("L-fallback", (("s20", 0), ("s20x33", 0), ("s20", 1), ("s20", 2)), ("run33",)),
)


@functools.lru_cache(maxsize=None)
def rows_of(cid):
    (c,) = [c for c in CASES if c[0] == cid]
    return [raw_of(fam, seed) for fam, seed in c[1]]


@functools.lru_cache(maxsize=None)
def model_of(cid):
    rows = rows_of(cid)
    return S.model([S.text_of(r) for r in rows], S.call_cap(rows, LEVEL))


LEVEL = 2
CONTROL = "E-agree-23"  # bz2_sort_cases' restart after three text rounds (it_full), unchanged
