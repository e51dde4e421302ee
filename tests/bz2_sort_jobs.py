"""The sort jobs of the GPU bzip2 encoder's BWT -- which sorter runs over
which slots of a chunk -- as a plain function over the first-round model of
bz2_sort_cases.py (imported, not edited), and the crafted streams aimed at the
rule's seams.  Shared by test_bwt_sort_jobs_cpu.py (the rule's properties on
every case list, no GPU) and test_bwt_sort_jobs_gpu.py (bytes against the
reference bzip2, lfm.bzip2_last_sort_jobs and the BWT stats against the
models).  TEST INFRASTRUCTURE ONLY.

The rule (bwt_bucket of csrc/lfm_bzip2.hip, ChunkLists):

  a chunk is one job, or two.  Two when cuts_of closed it after its last
  bucket (a bucket of at most kChunk that holds a multiple of kChunk), it has
  more than one bucket and more than kMiniCap = 512 rotations: its slots
  before that bucket, and the bucket.  The chunks cuts_of does not close that
  way -- the stream's last one, which ends at nsub, a chunk in front of a
  bucket above kChunk, and that bucket itself -- hold no multiple of kChunk
  beside a single bucket's, and are one job each.

  a job goes to the smallest sorter that holds it: 512, 1 024, 2 048, 4 096
  slots; a larger one (a single bucket) is the segmented sort's.

Every multi-bucket chunk above kChunk is closed after its last bucket, so no
multi-bucket job is longer than kChunk.
"""
import functools

import numpy as np

import bz2_sort_cases as S

CAPS = (512, 1024, 2048, 4096)
MINI = CAPS[0]


def cap_of(m):
    """The smallest sorter that holds m rotations; None: the segmented sort."""
    for c in CAPS:
        if m <= c:
            return c
    return None


def closing_buckets(hist):
    """{cut position: size of the bucket in front of it} for the entries
    cut_entries emits after a bucket of at most kChunk."""
    chunk = S.K["kChunk"]
    out, off = {}, 0
    for c in hist[hist > 0].tolist():
        e = off + c
        if c <= chunk and (e - 1) // chunk >= (off + chunk - 1) // chunk and e - 1 >= chunk:
            out[e] = c
        off = e
    return out


def jobs_of(fr):
    """The jobs of one stream's first round (bz2_sort_cases.first_round): a
    list per chunk of (begin, end, capacity)."""
    closing = closing_buckets(fr["hist"])
    out = []
    for b, e, _, _ in fr["chunks"]:
        m = e - b
        last = closing.get(e, m)
        if last < m and m > MINI:
            parts = [(b, e - last), (e - last, e)]
        else:
            parts = [(b, e)]
        out.append([(pb, pe, cap_of(pe - pb)) for pb, pe in parts])
    return out


def job_counts(rounds):
    """lfm.bzip2_last_sort_jobs of a call: rounds = the model's first rounds of
    its last attempt (model()["rounds"])."""
    n = dict.fromkeys(CAPS, 0)
    for fr in rounds.values():
        for jobs in jobs_of(fr):
            for _, _, cap in jobs:
                if cap is not None:
                    n[cap] += 1
    return n


# ------------------------------------------------------- crafted streams --
def with_pair(sizes, x, seed, tail=0):
    """sized_buckets(sizes) with two of bucket x's rotations tied on their
    8-byte prefix (as bz2_sort_cases' G-tied-at): bucket x still holds
    sizes[x]."""
    sizes = list(sizes)
    sizes[x] -= 2
    pair = bytes([x, S.Y, 9, 10, 11, 12, 13, 14, 20]) + bytes([x, S.Y, 9, 10, 11, 12, 13, 14, 30])
    body = S.sized_buckets(sizes, seed) + pair + bytes([40])
    return body + S.fillers(np.random.default_rng(seed + 1), tail, after=40)


# (id, bucket sizes in key order, tied pair in bucket x or None,
#  want: the jobs [(size, capacity)] of the chunk that begins at slot `at`)
BIG = 2772  # a bucket for the big sorter that ends 300 slots before slot 3 072
CRAFTED = (
    # the first part on the quarter-size sorter's limit
    ("J-first-511", [511, 600], None, 0, [(511, 512), (600, 1024)]),
    ("J-first-512", [512, 600], None, 0, [(512, 512), (600, 1024)]),
    ("J-first-513", [513, 600], None, 0, [(513, 1024), (600, 1024)]),
    # the last bucket on it
    ("J-last-511", [600, 511], None, 0, [(600, 1024), (511, 512)]),
    ("J-last-512", [600, 512], None, 0, [(600, 1024), (512, 512)]),
    ("J-last-513", [600, 513], None, 0, [(600, 1024), (513, 1024)]),
    # both on the half-size sorter's
    ("J-1-1024", [1, 1024], None, 0, [(1, 512), (1024, 1024)]),
    ("J-1023-1024", [1023, 1024], None, 0, [(1023, 1024), (1024, 1024)]),
    ("J-1024-1024", [1024, 1024], None, 0, [(1024, 1024), (1024, 1024)]),
    ("J-1023-1", [2049, 1023, 1], None, 2049, [(1023, 1024), (1, 512)]),
    # a multi-bucket chunk of exactly 512 stays one job, of 513 is two
    ("J-multi-512", [BIG, 300, 212], None, BIG, [(512, 512)]),
    ("J-multi-513", [BIG, 300, 213], None, BIG, [(300, 512), (213, 512)]),
    # single buckets: one job whatever the size
    ("J-single-1025", [5, 1025], None, 5, [(1025, 2048)]),
    # chunks cuts_of does not close after their last bucket: in front of a
    # bucket above kChunk, and the stream's last chunk (here the whole stream)
    ("J-before-big", [300, 300, 1500], None, 0, [(600, 1024)]),
    ("J-last-chunk-multi", [7], None, 0, None),
    # a tied pair inside a first part, and inside a last bucket
    ("J-pair-first", [600, 600], 0, 0, [(600, 1024), (600, 1024)]),
    ("J-pair-last", [600, 600], 1, 0, [(600, 1024), (600, 1024)]),
)
LAST_CHUNK_TAIL = 700  # J-last-chunk-multi: 5 * 7 + 700 + 13 rotations, below kChunk


def _units(cid):
    (c,) = [c for c in CRAFTED if c[0] == cid]
    return c


def crafted_raw(cid, total=None):
    """The crafted stream, with filler bytes at its end up to `total` raw
    bytes (the fillers' rotations sort behind the sized buckets)."""
    _, sizes, pair, _, _ = _units(cid)
    seed = 7000 + [c[0] for c in CRAFTED].index(cid)
    tail = LAST_CHUNK_TAIL if cid == "J-last-chunk-multi" else 0
    for _ in range(2):
        raw = with_pair(sizes, pair, seed, tail) if pair is not None else S.sized_buckets(sizes, seed, tail=tail)
        if total is None or len(raw) == total:
            return raw
        tail += total - len(raw)
    raise AssertionError(cid)


LEVEL = 2


def bench_like_raw(n, seed):
    """16-bit little-endian symbols (test_bwt_induce_compact_cpu.bench_like):
    sorted in kModeSortA."""
    from test_bwt_induce_compact_cpu import bench_like
    return bench_like(n, seed).tobytes()


# GPU calls: (id, the call's streams by crafted id -- or a builder taking the
# call's raw length -- ).  The streams of a call are padded to one raw length,
# so that the job lists of several streams interleave.
def _left_run(n):
    """A run of 33 copies that agree on 12 bytes: left by tie_runs_direct, settled by one text round."""
    return S.copies(S.word(12, 12), 33, 7212, total=n)


def _restart_run(n):
    """... on 23 bytes: three text rounds, then the whole batch again with every rotation in the sort."""
    return S.copies(S.word(23, 23), 33, 7223, total=n)


def _sort_a(n):
    return bench_like_raw(n, 7300)


CALLS = (
    ("JC-mini-seams", ("J-first-511", "J-first-512", "J-first-513", "J-last-511", "J-last-512", "J-last-513")),
    ("JC-tiny-seams", ("J-1-1024", "J-1023-1024", "J-1024-1024", "J-single-1025", "J-before-big")),
    ("JC-last-chunk", ("J-last-chunk-multi", _sort_a)),
    ("JC-behind-big", ("J-1023-1", "J-multi-512", "J-multi-513")),
    ("JC-pairs", ("J-pair-first", "J-pair-last", "J-first-512")),
    ("JC-left-run", ("J-first-513", "J-last-512", _left_run)),
    ("JC-restart", ("J-first-513", "J-last-512", _restart_run)),
    ("JC-sort-a", ("J-multi-513", _sort_a)),
)


@functools.lru_cache(maxsize=None)
def rows_of(call):
    (c,) = [c for c in CALLS if c[0] == call]
    n = max(len(crafted_raw(x)) for x in c[1] if isinstance(x, str))
    return [crafted_raw(x, n) if isinstance(x, str) else x(n) for x in c[1]]


@functools.lru_cache(maxsize=None)
def model_of(call):
    rows = rows_of(call)
    return S.model([S.text_of(r) for r in rows], S.call_cap(rows, LEVEL))
