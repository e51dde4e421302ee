"""The sort stage in the middle of the GPU bzip2 encoder's BWT -- everything
between bwt_bucket's histogram and bwt_place_sorted -- as a plain model, and
the case lists aimed at its limits.  Shared by test_bwt_sort_cases_cpu.py (the
premises, no GPU) and test_bwt_sort_seams_gpu.py (bytes against the reference
bzip2, lfm_hip_bzip2_last_bwt_stats against the model).  TEST INFRASTRUCTURE
ONLY.

The model of one call (the RLE1 texts of its streams, their cap, it_full = 0)
restates bwt_sort of csrc/lfm_bzip2.hip from its own constants:

  sorted set     the rotations that go through the sort in the stream's mode
                 (test_bwt_induce_compact_cpu.kernel_mode / scan_view)
  buckets        the top kBucketBits bits of the cyclic 8-byte prefix
  cut entries    cuts_of's rule: after a bucket that holds a multiple of kChunk
                 (from kChunk on), and before (unless at 0) and after a bucket
                 above kChunk -- two adjacent big buckets give the same entry
                 twice, an empty chunk.  kMaxCuts entries or more: the stream
                 is flagged for the host library and gets no chunks.
  chunks         between consecutive entries, the last to nsub; classes by
                 size: <= kTinyCap, <= kSmallCap, <= kBigCap, segmented sort
  first_ties     sorted rotations whose 8-byte prefix is shared
  left_runs      groups of equal 8-byte prefixes with more than kTieRunMax
                 members, or with two members that agree on kKeyBytes +
                 kTieCmpBytes = 72 bytes.  (An insertion sort compares every
                 pair that ends up adjacent, and a pair that agrees on 72 bytes
                 has an adjacent pair between them that does too: the scatter
                 order does not matter.)
  text rounds    covered 8 -> 13 -> 18 -> 23; a round runs while ties remain,
                 round 0 also needs left_runs > 0 and 4 * cnt <= N
  restart        ties at `covered` with it_full == 0: once more with every
                 rotation of every stream in the sort
  rank_rebuild   bwt_rank0 when no text round ran and 2 * cnt > N, else from
                 the gathered group keys
  doubling       h from `covered`, doubled per round, until no tie remains or
                 h >= cap; then the streams with ties left are flagged
                 (bwt_flag_periodic)

N = slots * cap.  The order every unflagged stream ends in is the order of
its rotations by their first `depth` bytes, depth the longest prefix any rung
the call reached compares; ladder_order returns it for the CPU tests to hold
against a naive sort.
"""
import functools

import numpy as np

from test_bwt_induce_compact_cpu import FULL, SORT_A, SORT_B, is_periodic, kernel_mode, rle1, scan_view  # noqa: F401

# csrc/lfm_bzip2.hip (test_bwt_sort_cases_cpu reads them back)
K = dict(kKeyBytes=8, kBucketBits=14, kChunk=1024, kTinyCap=1024, kMaxCuts=1024, kTieRunMax=32, kTieCmpBytes=64,
         kTextRounds=3, kTextBytes=5, kCsThreads=512, kCsItems=4, kBigThreads=512, kBigItems=8)
SMALL_CAP = K["kCsThreads"] * K["kCsItems"]
BIG_CAP = K["kBigThreads"] * K["kBigItems"]
DIRECT_BYTES = K["kKeyBytes"] + K["kTieCmpBytes"]  # 72
STATS = ("chunks_tiny", "chunks_small", "chunks_big", "chunks_segmented", "first_ties", "left_runs", "text_rounds",
         "restarted", "rank_form", "doubling_rounds", "flag_periodic")
RANK_NONE, RANK0, RANK_GATHERED = 0, 1, 2


def rle_cap(block_bytes):
    """lfm_bz_caps.h rle_cap"""
    return (block_bytes + block_bytes // 4 + 64 + 255) // 256 * 256


def nblock_max(level):
    return 100000 * level - 19


# ---------------------------------------------------------------- the model --
def mode_of(T):
    """kernel_mode, also for texts shorter than its 8-byte window."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    if n >= 8:
        return kernel_mode(T)
    ext = np.resize(T, n + 8)
    same = np.ones(n, bool)
    for d in range(1, 9):
        same &= ext[d:d + n] == T
    if same.any():
        return FULL
    nb = int(scan_view(T, SORT_A)[1].sum())
    return SORT_A if nb * 8 >= (n - nb) * 7 else SORT_B


def keys8(T):
    """The cyclic 8-byte prefix of every rotation, big endian."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    ext = np.concatenate([T] * (8 // n + 2))[:n + 8].astype(np.uint64)
    k = np.zeros(n, np.uint64)
    for d in range(8):
        k = (k << np.uint64(8)) | ext[d:d + n]
    return k


def prefixes(T, idx, L):
    """The first L bytes (cyclic) of the rotations idx, one row each."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    idx = np.asarray(idx, np.int64)
    return T[(idx[:, None] + np.arange(L)[None, :]) % n]


def split_groups(T, groups, L):
    """groups (arrays of rotations equal on fewer bytes) split by their first
    L bytes; the groups of more than one member."""
    out = []
    for g in groups:
        if len(g) < 2:
            continue
        _, inv = np.unique(prefixes(T, g, L), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for v in np.flatnonzero(np.bincount(inv) > 1):
            out.append(g[inv == v])
    return out


def cut_entries(hist):
    """cuts_of over a stream's bucket counts in bucket order."""
    chunk = K["kChunk"]
    cuts, off = [], 0
    for c in hist[hist > 0].tolist():
        e = off + c
        if c > chunk:
            if off:
                cuts.append(off)
            cuts.append(e)
        elif (e - 1) // chunk >= (off + chunk - 1) // chunk and e - 1 >= chunk:
            cuts.append(e)
        off = e
    return cuts


def chunk_class(m):
    return 0 if m <= K["kTinyCap"] else 1 if m <= SMALL_CAP else 2 if m <= BIG_CAP else 3


def first_round(T, mode):
    """bwt_bucket's cuts and the chunk sorts of one stream: a dict with
    nsub, hist, cuts, overflow, chunks [(begin, end, class, buckets)], groups
    (rotations per tied 8-byte prefix), slots (sorted slots that are tied),
    first_ties, left_runs."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    srt = np.arange(n) if mode == FULL else np.flatnonzero(~scan_view(T, mode)[1])
    key = keys8(T)[srt]
    order = np.argsort(key, kind="stable")
    ks, rot = key[order], srt[order]
    hist = np.bincount((ks >> np.uint64(64 - K["kBucketBits"])).astype(np.int64), minlength=1 << K["kBucketBits"])
    r = dict(nsub=len(srt), hist=hist, cuts=cut_entries(hist), chunks=[], groups=[], slots=np.zeros(0, np.int64),
             first_ties=0, left_runs=0)
    r["overflow"] = len(r["cuts"]) >= K["kMaxCuts"]
    if r["overflow"]:
        return r
    bkt = ks >> np.uint64(64 - K["kBucketBits"])
    bounds = [0] + r["cuts"] + [r["nsub"]]
    for b, e in zip(bounds[:-1], bounds[1:]):
        if e > b:
            r["chunks"].append((b, e, chunk_class(e - b), int((bkt[b + 1:e] != bkt[b:e - 1]).sum()) + 1))
    tied = np.zeros(len(ks), bool)
    if len(ks) > 1:
        eq = ks[1:] == ks[:-1]
        tied[1:] |= eq
        tied[:-1] |= eq
    r["slots"] = np.flatnonzero(tied)
    r["first_ties"] = int(tied.sum())
    if r["first_ties"]:
        starts = np.flatnonzero(tied & ~np.concatenate([[False], ks[1:] == ks[:-1]]))
        stops = np.flatnonzero(tied & ~np.concatenate([ks[1:] == ks[:-1], [False]])) + 1
        r["groups"] = [rot[a:b] for a, b in zip(starts, stops)]
        for g in r["groups"]:
            if len(g) > K["kTieRunMax"] or split_groups(T, [g], DIRECT_BYTES):
                r["left_runs"] += 1
    return r


def agree(T, i, j):
    """Bytes on which rotations i and j of T agree (cyclic; n for equal ones)."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    d = np.flatnonzero(np.roll(T, -i) != np.roll(T, -j))
    return int(d[0]) if len(d) else n


def model(texts, cap, it_full=0, flagged=None):
    """One bwt_sort call over the slots' texts (None or a flagged slot: not
    sorted).  Returns dict(stats, host (per slot: flagged by the sort), modes,
    rounds (first_round of the last attempt per slot), depth, attempts)."""
    texts = [None if t is None else np.asarray(t, np.uint8) for t in texts]
    host = [False] * len(texts)
    skip = [t is None or bool(flagged and flagged[s]) for s, t in enumerate(texts)]
    N = len(texts) * cap
    st = dict.fromkeys(STATS, 0)
    modes = [None if skip[s] else mode_of(t) for s, t in enumerate(texts)]
    attempts = []
    while True:
        live = [s for s in range(len(texts)) if not skip[s] and not host[s]]
        fr = {s: first_round(texts[s], FULL if it_full else modes[s]) for s in live}
        for s in live:
            host[s] |= fr[s]["overflow"]
        cls = [c[2] for s in live for c in fr[s]["chunks"]]
        for k in range(4):
            st[STATS[k]] = cls.count(k)
        st["first_ties"] = sum(fr[s]["first_ties"] for s in live)
        st["left_runs"] = sum(fr[s]["left_runs"] for s in live)
        st["text_rounds"] = 0
        groups = {s: fr[s]["groups"] for s in live}
        cnt = st["first_ties"]
        covered = K["kKeyBytes"]
        depth = DIRECT_BYTES if cnt else covered
        left = cnt
        if cnt == 0 or st["left_runs"] == 0:
            left = 0
        elif 4 * cnt <= N:
            for _ in range(K["kTextRounds"]):
                if left == 0:
                    break
                covered += K["kTextBytes"]
                st["text_rounds"] += 1
                groups = {s: split_groups(texts[s], g, covered) for s, g in groups.items()}
                left = sum(len(g) for gs in groups.values() for g in gs)
            depth = max(depth, covered)
        attempts.append(dict(first=fr, covered=covered, left=left))
        if left and not it_full:
            it_full = 1
            st["restarted"] = 1
            continue
        break
    if left:
        st["rank_form"] = RANK0 if covered == K["kKeyBytes"] and 2 * left > N else RANK_GATHERED
        # ranks: any labelling of the groups of equal `covered`-byte prefixes
        rank = {}
        for s in live:
            if groups[s]:
                _, inv = np.unique(prefixes(texts[s], np.arange(len(texts[s])), covered), axis=0, return_inverse=True)
                rank[s] = inv.reshape(-1).astype(np.int64)
        h = covered
        while left:
            if h >= cap:
                st["flag_periodic"] = 1
                for s in rank:
                    host[s] = True
                break
            left = 0
            for s in list(rank):
                n = len(texts[s])
                pair = rank[s] * (n + 1) + np.roll(rank[s], -(h % n))
                _, inv, c = np.unique(pair, return_inverse=True, return_counts=True)
                rank[s] = inv.reshape(-1).astype(np.int64)
                t = int(c[c > 1].sum())
                if t == 0:
                    del rank[s]
                left += t
            h *= 2
            st["doubling_rounds"] += 1
        depth = max(depth, h)
    return dict(stats=st, host=host, modes=modes, rounds=fr, depth=depth, attempts=attempts, it_full=it_full)


def ladder_order(T, cap=None):
    """The order the ladder leaves the sorted rotations of one stream in (a
    call of its own), or None when the stream comes back flagged; and the model."""
    T = np.asarray(T, np.uint8)
    m = model([T], cap or rle_cap(len(T)))
    if m["host"][0]:
        return None, m
    mode = FULL if m["it_full"] else m["modes"][0]
    srt = np.arange(len(T)) if mode == FULL else np.flatnonzero(~scan_view(T, mode)[1])
    depth = min(m["depth"], len(T))
    tb = T.tobytes() * (depth // len(T) + 2)
    keys = [tb[i:i + depth] for i in srt.tolist()]
    assert len(set(keys)) == len(keys), "the ladder leaves two rotations tied"
    return [i for _, i in sorted(zip(keys, srt.tolist()))], m


def naive_order(T, mode):
    T = np.asarray(T, np.uint8)
    n = len(T)
    srt = np.arange(n) if mode == FULL else np.flatnonzero(~scan_view(T, mode)[1])
    tb = T.tobytes() * 2
    return sorted(srt.tolist(), key=lambda i: tb[i:i + n])


# ------------------------------------------------------------ the builders --
FB = bytes([0xFB])
FB_RUN = FB * 510  # two RLE1 pieces of 255: ten 0xFB in the text, which forces kModeFull
Y = 250            # second byte of the sized buckets: bucket (x, Y >> 2)


def fillers(rng, n, lo=8, hi=250, after=None):
    """n bytes in lo..hi-1, no two neighbours equal, the first not `after`."""
    out = np.empty(n, np.int64)
    prev = -1 if after is None else after
    span = hi - lo
    for k in range(n):
        v = lo + int(rng.integers(0, span))
        if v == prev:
            v = lo + (v - lo + 1) % span
        out[k] = prev = v
    return out.astype(np.uint8).tobytes()


def sized_buckets(sizes, seed, fill=3, tail=0, lead=True):
    """A kModeFull stream whose first buckets in key order hold exactly
    `sizes` rotations: bucket k is (k, Y >> 2), from sizes[k] units `k Y f..`
    with `fill` filler bytes in 8..249 (no filler pair, and nothing else, starts
    with a byte below 8); the units are shuffled; `tail` more filler bytes at the
    end.  Bucket sizes are pair counts because every rotation is sorted."""
    assert len(sizes) <= 8
    rng = np.random.default_rng(seed)
    xs = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(xs)
    body = bytearray()
    for x in xs.tolist():
        body += bytes([x, Y]) + fillers(rng, fill)
    body += fillers(rng, tail, after=body[-1] if body else None)
    return (FB_RUN if lead else b"") + bytes(body)


def copies(word, g, seed, gap=40, lead=True, total=None, alphabet=(8, 250)):
    """g copies of `word`, each between filler bytes, the byte before and
    after each copy different from copy to copy (g <= 120): two copies agree on
    exactly len(word) - o bytes from offset o of the word."""
    rng = np.random.default_rng(seed)
    lo, hi = alphabet
    assert 2 * g <= hi - lo and not set(word) & set(range(lo, hi))
    marks = rng.permutation(np.arange(lo, hi))[:2 * g].tolist()
    body = bytearray()
    for j in range(g):
        body += fillers(rng, gap, lo, hi) + bytes([marks[2 * j]]) + bytes(word) + bytes([marks[2 * j + 1]])
    body += fillers(rng, gap, lo, hi)
    if total is not None:
        body += fillers(rng, total - len(body) - (len(FB_RUN) if lead else 0), lo, hi, after=body[-1])
    return (FB_RUN if lead else b"") + bytes(body)


def word(L, seed=0):
    """L bytes in 1..7 and 251..255 without a run (none is a filler)."""
    rng = np.random.default_rng(900 + seed)
    return fillers(rng, L, 1, 8)


def text_of(raw):
    return rle1(np.frombuffer(bytes(raw), np.uint8))


# ------------------------------------------------------------ the case lists --
# A case: (id, [raw streams of one call], level, want) -- want: the facts the
# CPU test must find in the model (witnessed once, pinned here), a dict over
# STATS names plus
#   bucket      a bucket of exactly that many rotations exists
#   chunk       (size, buckets > 1?) such a chunk exists
#   periodic    the slots the model flags
# Every case is a call of its own (its streams all of one raw length).

def _a_cases():
    c = []
    # single buckets on the class limits: 1024 joins a multi-bucket chunk,
    # 1025..2048 the small sorter, 2049..4096 the big one, 4097 the segmented sort
    for size, cls in ((1024, None), (1025, "chunks_small"), (2048, "chunks_small"), (2049, "chunks_big"),
                      (4096, "chunks_big"), (4097, "chunks_segmented")):
        # a small bucket first so that the sized one does not start at 0
        c.append(("A-bucket-%d" % size, [sized_buckets([5, size], 10 + size)], 2, dict(bucket=size, cls=cls)))
    # multi-bucket chunks: after a big bucket of `first`, buckets of 1000 and
    # m - 1000 rotations; the chunk ends with the bucket that holds slot 3072
    for m, first in ((1023, 2050), (1024, 2049), (1025, 2049)):
        c.append(("A-multi-%d" % m, [sized_buckets([first, 1000, m - 1000], 20 + m)], 2,
                  dict(chunk=(m, True))))
    c.append(("A-multi-2047", [sized_buckets([1023, 1024], 31)], 2, dict(chunk=(2047, True))))
    c.append(("A-multi-2048", [sized_buckets([1024, 1024], 32)], 2, dict(chunk=(2048, True))))
    c.append(("A-big-first", [sized_buckets([1500], 33)], 2, dict(chunk=(1500, False), first_cut=1500)))
    c.append(("A-big-back-to-back", [sized_buckets([3, 1500, 1600], 34)], 2, dict(dup_cut=1503)))
    c.append(("A-one-chunk", [sized_buckets([7], 35, tail=300)], 2, dict(nchunks=1)))
    return c


def _class_count_batch(k, seed):
    """One call whose streams each hold one single-bucket chunk for the big
    sorter and one for the segmented sort: k streams -> k and k chunks."""
    return [sized_buckets([1100, 2100, 4100], seed + s, fill=1) for s in range(k)]


@functools.lru_cache(maxsize=None)
def a_cases():
    c = _a_cases()
    for k in (1, 7, 8, 9):
        c.append(("A-classes-x%d" % k, _class_count_batch(k, 40), 2, dict(chunks_big=k, chunks_segmented=k)))
        # k streams of one chunk each: k chunks for the half-size sorter, no other
        c.append(("A-tiny-x%d" % k, [sized_buckets([7], 60 + s, tail=300) for s in range(k)], 2,
                  dict(chunks_tiny=k, chunks_small=0, chunks_big=0, chunks_segmented=0)))
    return c


B_ALPHA, B_LEN = 27, 890000


@functools.lru_cache(maxsize=None)
def overflow_body(alpha=B_ALPHA, n=B_LEN, seed=5):
    """n bytes over the `alpha` values 4 v without a run of four: alpha^2
    buckets in kModeFull, (4 v, v')."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, alpha, n)
    for i in np.flatnonzero((v[3:] == v[2:-1]) & (v[3:] == v[1:-2]) & (v[3:] == v[:-3])) + 3:
        if v[i] == v[i - 1] == v[i - 2] == v[i - 3]:
            v[i] = (v[i] + 1) % alpha
    return (4 * v).astype(np.uint8).tobytes()


# lengths of the same body at which the stream needs exactly 1 022, 1 023 and
# 1 024 cut entries (witnessed by a scan over the length; the CPU test recounts)
B_SIBLINGS = ((1022, 741909), (1023, 742362), (1024, 742305))


@functools.lru_cache(maxsize=None)
def b_cases(siblings=None):
    c = [("B-overflow-890k", [FB_RUN + overflow_body()], 9, dict(min_cuts=K["kMaxCuts"], periodic=[0]))]
    for ncut, n in (siblings or B_SIBLINGS):
        if n is not None:
            c.append(("B-cuts-%d" % ncut, [FB_RUN + overflow_body()[:n]], 9,
                      dict(cuts=ncut, periodic=[0] if ncut >= K["kMaxCuts"] else [])))
    return c


@functools.lru_cache(maxsize=None)
def c_cases():
    """Keys at the wrap: ties among the rotations that start in the last 7 and
    the first 5 bytes, n % 4 of 0..3, and texts of 9..16 bytes."""
    c = []
    w = word(20, 9)
    for extra in range(4):
        rng = np.random.default_rng(50 + extra)
        mid = fillers(rng, 600 + extra)
        # the word straddles the wrap (7 bytes at the end, 13 at the start) and
        # stands once more inside: the ties that start in its first 7 bytes
        # have keys over the wrap, those at offsets 7..11 start in T[0..4]
        raw = w[7:] + mid[:300] + w + mid[300:] + w[:7]
        c.append(("C-wrap-n%%4=%d" % (len(raw) % 4), [raw], 2, dict(min_ties=2, wrap_tie=True)))
    for n in range(9, 17):
        rng = np.random.default_rng(70 + n)
        raw = bytes([1, 2]) * 3 + fillers(rng, n - 6)  # 1 2 1 2 1 2: near-ties inside 8 bytes
        c.append(("C-short-%d" % n, [raw], 2, dict(n=n)))
    return c


@functools.lru_cache(maxsize=None)
def d_cases():
    """Direct runs: sizes 2, 31, 32, 33; the longest agreement 8, 15, 16, 71
    (resolved by tie_runs_direct) and 72 (left); a run over the wrap."""
    c = []
    for g in (2, 31, 32, 33):
        c.append(("D-run-%d" % g, [copies(word(20), g, 100 + g)], 2, dict(max_run=g, left=g > 32)))
    for L in (8, 15, 16, 71, 72):
        c.append(("D-agree-%d" % L, [copies(word(L), 3, 120 + L)], 2, dict(max_agree=L, left=L >= DIRECT_BYTES)))
    # the same without the 0xFB run: kModeSortA / kModeSortB streams
    c.append(("D-agree-40-typed", [copies(word(40), 5, 131, lead=False)], 2, dict(max_agree=40, left=False, typed=True)))
    c.append(("D-agree-72-typed", [copies(word(72), 5, 132, lead=False)], 2, dict(max_agree=72, left=True, typed=True)))
    rng = np.random.default_rng(140)
    w = word(30, 3)
    mid = fillers(rng, 500)
    c.append(("D-run-over-wrap", [w[20:] + mid[:250] + bytes([200]) + w + bytes([201]) + mid[250:] + w[:20]], 2,
              dict(wrap_tie=True, left=False)))
    # a left run beside resolved ones: the rounds re-sort the resolved runs
    c.append(("D-left-beside-resolved", [copies(word(72), 2, 141) + copies(word(30, 5), 4, 142, lead=False)], 2,
              dict(left=True, resolved_too=True)))
    return c


@functools.lru_cache(maxsize=None)
def e_cases():
    """Text rounds: runs of 33 (left by size) whose members agree on exactly
    12, 13, 17, 18, 22 and 23 bytes: resolved in round 1, 2, 2, 3, 3 and at
    the restart."""
    c = []
    for L, rounds, restart in ((12, 1, 0), (13, 2, 0), (17, 2, 0), (18, 3, 0), (22, 3, 0), (23, 3, 1)):
        c.append(("E-agree-%d" % L, [copies(word(L, L), 33, 200 + L)], 2,
                  dict(max_agree=L, text_rounds=rounds, restarted=restart)))
    # the same tied key at the edge of several streams (text_bounds' stream
    # test): 40 bytes of 0xFB are each stream's only tied group, 33 rotations
    # that start with eight of them, the last of one stream's list and the
    # first of the next one's
    rows = [FB * (255 * 8) + fillers(np.random.default_rng(230 + s), 2000) for s in range(4)]
    c.append(("E-same-key-4-streams", rows, 2, dict(text_rounds=3, restarted=1, same_key=True, one_group=True)))
    # off % n with n < 23.  Rotations of so short a text that tie on 8 bytes
    # and are not resolved before `off` passes n are equal: a text of 15 times
    # 0xFB (765 raw bytes), one run of 15 equal rotations, beside a stream that
    # needs the three rounds.  The short one comes back flagged.
    c.append(("E-short-15-beside-rounds", [FB * 765, copies(word(18, 18), 33, 240, gap=2, lead=False, total=765)], 2,
              dict(n=15, text_rounds=3, restarted=1, periodic=[0], flag_periodic=1)))
    return c


@functools.lru_cache(maxsize=None)
def f_cases():
    """Restart, ranks, doubling, periodic."""
    c = []
    rng = np.random.default_rng(300)
    R = fillers(rng, 6000)
    # nearly every rotation tied: round 0 is skipped (4 cnt > N), after the
    # restart 2 cnt > N: bwt_rank0
    c.append(("F-two-copies-changed", [R + bytes([1]) + R + bytes([2])], 2,
              dict(text_rounds=0, restarted=1, rank_form=RANK0, periodic=[])))
    # after the restart N / 4 < cnt <= N / 2: gathered from the first-round keys
    c.append(("F-half-tied", [R[:2500] + bytes([1]) + R[:2500] + bytes([2]) + fillers(rng, 7000)], 2,
              dict(text_rounds=0, restarted=1, rank_form=RANK_GATHERED, periodic=[])))
    # ties left after 23 bytes: gathered from the text keys; 1, 2 and many rounds
    for L, g, rounds in ((30, 33, 1), (80, 2, 2)):
        c.append(("F-repeat-%d" % L, [copies(fillers(np.random.default_rng(310 + L), L, 1, 8), g, 320 + L, total=9000)],
                  2, dict(text_rounds=3, restarted=1, rank_form=RANK_GATHERED, doubling_rounds=rounds, periodic=[])))
    # many rounds: 8 -> 16 -> ... -> 4 096 (two copies of 3 000 bytes are most
    # of the stream, so no text round runs and the ranks come from bwt_rank0)
    c.append(("F-repeat-3000", [copies(fillers(np.random.default_rng(3310), 3000, 1, 8), 2, 3320, total=9000)], 2,
              dict(text_rounds=0, restarted=1, rank_form=RANK0, doubling_rounds=9, periodic=[])))
    motif = bytes([9, 200, 31, 77, 5, 180, 66])
    per = motif * 600
    c.append(("F-period-7-last-changed", [per[:-1] + bytes([100])], 2, dict(restarted=1, periodic=[])))
    c.append(("F-period-7", [per], 2, dict(restarted=1, periodic=[0], flag_periodic=1)))
    c.append(("F-two-copies", [R[:3000] + R[:3000]], 2, dict(restarted=1, periodic=[0], flag_periodic=1)))
    c.append(("F-prime-constant-plus-one", [FB_RUN + bytes([61])], 2, dict(n=11, periodic=[])))
    mixed = [fillers(np.random.default_rng(330 + k), 4200) for k in range(3)]
    mixed.insert(1, per)
    c.append(("F-periodic-in-batch", mixed, 2, dict(restarted=1, periodic=[1], flag_periodic=1)))
    return c


def _short_rows(count, tied, seed):
    """count rows of 48 bytes; row s holds a 12-byte word twice when tied(s)."""
    rng = np.random.default_rng(seed)
    w = word(12, 7)
    rows = []
    for s in range(count):
        f = fillers(rng, 48)
        rows.append(f[:5] + w + f[17:30] + w + f[42:] if tied(s) else f)
    return rows


@functools.lru_cache(maxsize=None)
def g_cases():
    c = []
    # tied slots on tie_compact's wave (1 024 slots) and tile (4 096) edges: a
    # first bucket of K - 1 rotations, then a pair with one 8-byte prefix
    for edge in (1024, 4096):
        units = sized_buckets([edge - 1], 400 + edge)
        pair = bytes([1, Y, 9, 10, 11, 12, 13, 14, 20]) + bytes([1, Y, 9, 10, 11, 12, 13, 14, 30])
        c.append(("G-tied-at-%d" % edge, [units + pair + bytes([40])], 2, dict(tied_slots=(edge - 1, edge))))
    for r in (0, 1, 15):
        base = sized_buckets([40], 420, tail=100)
        pad = (r - len(text_of(base))) % 16
        c.append(("G-nsub%%16=%d" % r, [base + fillers(np.random.default_rng(421), pad, after=base[-1])], 2,
                  dict(nsub_mod16=r, last_slot_tied=True)))
    for count in (1025, 2049):
        c.append(("G-batch-%d" % count, _short_rows(count, lambda s: s % 3 == 0, 430), 2, dict(streams=count)))
    return c


@functools.lru_cache(maxsize=None)
def g_swap_pair():
    """Two calls of one shape for one workspace: the tied and the untied
    streams swapped."""
    return (_short_rows(1025, lambda s: s % 2 == 0, 440), _short_rows(1025, lambda s: s % 2 == 1, 440))


H_BLOCK, H_LEVEL = 110000, 1


@functools.lru_cache(maxsize=None)
def h_case():
    """One stream of two parts at level 1 (lfm_hip_bzip2_blocks_multi): a
    repeat of 60 bytes crosses the cut, and the second part holds a run of 33
    copies that agree on 18 bytes (text rounds)."""
    rng = np.random.default_rng(500)
    cut = nblock_max(H_LEVEL)
    head = fillers(rng, cut - 30)
    rep = fillers(np.random.default_rng(501), 60, 1, 8)
    second = copies(word(18, 18), 33, 502, lead=False)
    raw = head + rep + fillers(rng, 200) + bytes([251]) + rep + bytes([252]) + second
    return raw + fillers(rng, H_BLOCK - len(raw), after=raw[-1])


@functools.lru_cache(maxsize=None)
def h_model():
    """(raw, model) of list H's call: the slots' texts are the parts libbzip2
    cuts the stream into (consecutive ranges of its RLE1 text)."""
    from bz2_parts import parts
    raw = h_case()
    full = text_of(raw)
    texts, o = [], 0
    for _, _, tl in parts(raw, H_LEVEL):
        texts.append(full[o:o + tl])
        o += tl
    assert o == len(full)
    m = model(texts, call_cap([raw], H_LEVEL, multi=True))
    m["texts"] = texts
    m["stream_host"] = [any(m["host"])]
    return raw, m


def call_cap(rows, level, multi=False):
    n = len(rows[0])
    cap = rle_cap(n)
    if multi:
        from bz2_encode_cases import max_parts
        if max_parts(n, level) > 1:
            cap = min(cap, (nblock_max(level) + 5 + 64 + 255) // 256 * 256)
    return cap


@functools.lru_cache(maxsize=None)
def all_cases():
    return a_cases() + b_cases() + c_cases() + d_cases() + e_cases() + f_cases() + g_cases()


@functools.lru_cache(maxsize=None)
def _model_of(cid):
    for c, rows, level, _ in all_cases():
        if c == cid:
            return model([text_of(r) for r in rows], call_cap(rows, level))
    raise KeyError(cid)


def model_of(cid):
    return _model_of(cid)
