"""Calls aimed at the placement of the sorted rotations in the GPU bzip2
encoder's BWT: by the chunk sorts themselves (their PLACE epilogue, then
bwt_place_tied and bwt_pend_live), by bwt_place_sorted over the whole batch, or
not at all (restart).  Shared by test_bwt_place_path_cpu.py (which proves what
each case claims, on the model of bz2_sort_cases.py) and
test_bwt_place_path_gpu.py (bytes, flags and lfm.bzip2_last_place_path against
that model).  TEST INFRASTRUCTURE ONLY.

A case: (id, [raw streams of one call, all of one length], level, multi).
"""
import functools
import itertools

import numpy as np

import bz2_sort_cases as S
import test_bwt_induce_compact_cpu as M

NONE, FUSED, WHOLE = 0, 1, 2


def place_path(stats):
    """bwt_sort's rule (BwtStats::place_path) over the model's stats."""
    if stats["restarted"]:
        return NONE
    if stats["chunks_segmented"] or stats["left_runs"] or stats["text_rounds"]:
        return WHOLE
    return FUSED


# ------------------------------------------------------- tied pairs by slot --
def pair_bucket(size, pos, seed):
    """A kModeFull stream (the 0xFB lead) whose first bucket in key order,
    (1, Y >> 2), holds exactly `size` rotations -- sorted slots 0 .. size - 1 --
    of which those at slots pos and pos + 1 share their 8-byte prefix and
    differ in the ninth byte; of the two, the one earlier in the text sorts
    later.  Units `1 Y f1 f2 f3` with distinct filler triples order the bucket;
    the pair's triple is the one of rank pos, used twice, each copy followed by
    a unit with the same f1 (so the pair agrees on `1 Y f f f 1 Y g`).  Beside
    the pair only the text's last three slots tie (ten 0xFB: the rotations that
    start with eight of them)."""
    assert 4 <= size and 0 <= pos <= size - 2
    for sd in itertools.count(seed):
        rng = np.random.default_rng(sd)
        a, b = (100, 40, 50), (100, 20, 30)
        triples = {a, b}
        while len(triples) < size - 1:
            triples.add(tuple(S.fillers(rng, 3)))
        ts = sorted(triples)
        p = ts[pos]
        if p not in (a, b):
            break
    others = [t for t in ts if t not in (a, b, p)]
    rng.shuffle(others)
    h = len(others) // 2
    units = others[:h] + [p, a] + others[h:] + [p, b]
    assert len(units) == size
    return S.FB_RUN + b"".join(bytes((1, S.Y) + u) for u in units)


# (id, bucket size, slot of the pair, sorter class, chunk [begin, end) or None: the whole stream)
PAIRS = (
    ("P-pair-tiny-first", 200, 0, 0, None),
    ("P-pair-tiny-ipt", 200, 4 * 10 + 3, 0, None),
    ("P-pair-small-first", 1500, 0, 1, (0, 1500)),
    ("P-pair-small-ipt", 1500, 4 * 100 + 3, 1, (0, 1500)),
    ("P-pair-small-last", 1500, 1498, 1, (0, 1500)),
    ("P-pair-big-first", 3000, 0, 2, (0, 3000)),
    ("P-pair-big-ipt", 3000, 8 * 100 + 7, 2, (0, 3000)),
    ("P-pair-big-last", 3000, 2998, 2, (0, 3000)),
)


# ----------------------------------------------------------- text wrap --
WRAP_N = 3000


def _wrap_body(mode, seed):
    if mode == S.SORT_B:
        return M.triples_b(WRAP_N, seed).astype(np.int64)
    return np.random.default_rng(seed).integers(20, 200, WRAP_N)


def wrap_all_sorted(mode, seed):
    """Rotations n - 8 .. n - 1 and 0 .. 3 all of the sorted type: one
    monotone stretch over the wrap (falling for kModeSortA, rising for B)."""
    T = _wrap_body(mode, seed)
    ramp = 3 + 5 * np.arange(13)
    T[np.arange(-8, 5)] = ramp if mode == S.SORT_B else ramp[::-1]
    return T.astype(np.uint8).tobytes()


def wrap_chain(mode, k, seed):
    """Rotation k (0 .. 3) sorted, the six before it (over the wrap) placed by
    the scan in one chain from it, the nearest five live: they get
    T[k-2 .. k-4] from its entry."""
    T = _wrap_body(mode, seed)
    ramp = 10 + 30 * np.arange(7)
    T[np.arange(k - 6, k + 1)] = ramp if mode == S.SORT_A else 250 - ramp
    T[k + 1] = 5 if mode == S.SORT_A else 252
    return T.astype(np.uint8).tobytes()


def wrap_rows(mode):
    return [wrap_all_sorted(mode, 700 + mode)] + [wrap_chain(mode, k, 710 + 10 * mode + k) for k in range(4)]


# ------------------------------------------------------------- streams --
def padded(body, total, seed):
    """body, then runs of up to 255 equal bytes (a different byte per run) up
    to `total` raw bytes: five bytes of RLE1 text per run, so streams of one
    raw length get texts of different lengths."""
    body = bytes(body)
    rng = np.random.default_rng(seed)
    vals = [v for v in rng.permutation(np.arange(0, 250)).tolist() if v != body[-1]]
    out, k = bytearray(body), 0
    while len(out) < total:
        out += bytes([vals[k]]) * min(255, total - len(out))
        k += 1
    return bytes(out)


def _alpha(n, a, seed, scale=False):
    T = np.random.default_rng(seed).integers(0, a, n)
    return (T * (255 // (a - 1)) if scale else T).astype(np.uint8).tobytes()


STREAMS_RAW = 6000


def nine_streams():
    bodies = [_alpha(300, 2, 801, True), _alpha(950, 3, 802), _alpha(1600, 4, 803, True), _alpha(2250, 16, 804),
              _alpha(2900, 256, 805), M.bench_like(3550, 806).tobytes(), M.triples_b(4200, 807).tobytes(),
              M.ascending_runs(4850, 808).tobytes(), M.five_bytes(5500, 809).tobytes()]
    return [padded(b, STREAMS_RAW, 820 + i) for i, b in enumerate(bodies)]


def two_streams():
    return [padded(_alpha(1000, 4, 811), STREAMS_RAW, 831), padded(_alpha(5000, 256, 812), STREAMS_RAW, 832)]


def flagged_between():
    """List B's stream of exactly kMaxCuts cut entries (flagged for the host
    library by bwt_bucket) between two ordinary streams of its length."""
    (flagged,) = [rows[0] for cid, rows, _, _ in S.b_cases() if cid == "B-cuts-1024"]
    n = len(flagged)

    def ordinary(seed):
        return np.random.default_rng(seed).integers(8, 250, n).astype(np.uint8).tobytes()
    return [ordinary(840), flagged, ordinary(841)]


def full_beside_ordinary():
    """A kModeFull stream (510 times 0xFB: ten of them in the text, as the
    lead of lists A, D, E; their three rotations of eight are settled
    directly) between kModeSortA and kModeSortB ones: symbols and origPtr only
    for it."""
    n = 6000
    rng = np.random.default_rng(11)
    full = np.concatenate([np.full(510, 0xFB, np.uint8), rng.integers(0, 250, n - 510).astype(np.uint8)])
    return [M.bench_like(n, 12).tobytes(), full.tobytes(), M.triples_b(n, 13).tobytes(),
            M.ascending_runs(n, 14).tobytes()]


# ---------------------------------------------------------- live slots --
def zigzag(n, seed):
    """High, low, high, low: every placed rotation (the low bytes' of
    kModeSortA) follows a larger byte, so none is live."""
    rng = np.random.default_rng(seed)
    T = np.empty(n, np.int64)
    T[0::2] = rng.integers(120, 250, len(T[0::2]))
    T[1::2] = rng.integers(0, 100, len(T[1::2]))
    return T.astype(np.uint8).tobytes()


# --------------------------------------------------------------- parts --
@functools.lru_cache(maxsize=None)
def h_direct_case():
    """List H's stream without its run of 33 copies: two parts at level 1, a
    repeat of 60 bytes over the cut, every tie settled by tie_runs_direct."""
    rng = np.random.default_rng(900)
    cut = S.nblock_max(S.H_LEVEL)
    head = S.fillers(rng, cut - 30)
    rep = S.fillers(np.random.default_rng(901), 60, 1, 8)
    raw = head + rep + S.fillers(rng, 200) + bytes([251]) + rep + bytes([252])
    return raw + S.fillers(rng, S.H_BLOCK - len(raw), after=raw[-1])


def parts_model(raw, level):
    """As bz2_sort_cases.h_model: the slots' texts are the parts."""
    from bz2_parts import parts
    full = S.text_of(raw)
    texts, o = [], 0
    for _, _, tl in parts(raw, level):
        texts.append(full[o:o + tl])
        o += tl
    assert o == len(full)
    m = S.model(texts, S.call_cap([raw], level, multi=True))
    m["texts"] = texts
    m["stream_host"] = [any(m["host"])]
    return m


# ------------------------------------------------------------- the list --
FROM_LISTS = (
    # path 1 with ties: runs of 2, 31 and 32 settled directly (kModeFull streams), and typed ones
    "D-run-2", "D-run-31", "D-run-32", "D-agree-40-typed",
    # chunk fill: single buckets and multi-bucket chunks on the sorters' limits; 4 097 is the segmented sort's
    "A-bucket-1025", "A-bucket-2048", "A-bucket-2049", "A-bucket-4096", "A-bucket-4097", "A-multi-1024",
    "A-multi-1025", "A-multi-2048",
    # path 2 by a text round, path 0 by the restart
    "E-agree-12", "D-agree-72",
)


@functools.lru_cache(maxsize=None)
def cases():
    by_id = {cid: (cid, rows, level, False) for cid, rows, level, _ in S.all_cases()}
    c = [by_id[cid] for cid in FROM_LISTS]
    c += [(cid, [pair_bucket(size, pos, 600 + i)], 2, False) for i, (cid, size, pos, _, _) in enumerate(PAIRS)]
    # a chunk of exactly one rotation: a bucket of one in front of a bucket above kChunk
    c.append(("P-chunk-1", [S.sized_buckets([1, 1500], 650)], 2, False))
    c.append(("P-wrap-sort-a", wrap_rows(S.SORT_A), 2, False))
    c.append(("P-wrap-sort-b", wrap_rows(S.SORT_B), 2, False))
    c.append(("P-two-streams", two_streams(), 2, False))
    c.append(("P-nine-streams", nine_streams(), 2, False))
    c.append(("P-flagged-between", flagged_between(), 9, False))
    c.append(("P-full-beside-ordinary", full_beside_ordinary(), 2, False))
    c.append(("P-no-live-slot", [zigzag(6000, 860)], 2, False))
    c.append(("P-live-rising", [M.ascending_runs(12000, 861).tobytes()], 2, False))
    c.append(("P-live-falling", [M.descending_runs(12000, 862).tobytes()], 2, False))
    c.append(("H-two-parts", [S.h_case()], S.H_LEVEL, True))
    c.append(("P-two-parts-direct", [h_direct_case()], S.H_LEVEL, True))
    return c


def case(cid):
    (c,) = [c for c in cases() if c[0] == cid]
    return c


@functools.lru_cache(maxsize=None)
def model_of(cid):
    _, rows, level, multi = case(cid)
    if multi:
        return parts_model(rows[0], level)
    return S.model([S.text_of(r) for r in rows], S.call_cap(rows, level))


def texts_of(cid):
    return [S.text_of(r) for r in case(cid)[1]]
