"""The bucket pass of the GPU bzip2 encoder with eight rotations per lane
(bwt_bucket: the word-level classifier, the histogram walk, the scatter walk,
the 8 192-byte tile) against the reference bzip2, byte for byte.

Every stream must come back with flags == 0: a stream handed to the host
library would hide a wrong bucket pass.  So each test asserts on the CPU that
its texts are non-periodic and run in the mode it means.  The output is
compared whole: a wrong count, a wrong bucket or a wrong preceding byte (the
BWT's output column is the byte each rotation carries) shows in the bytes."""
import numpy as np
import pytest

import test_bwt_induce_compact_cpu as M
from test_bwt_induce_compact_gpu import encode, ref_bz2

pytestmark = pytest.mark.gpu

# bwt_bucket's geometry (csrc/lfm_bzip2.hip: kBktG, kBucketThreads, kBktTile;
# the library does not export them)
G = 8
THREADS = 1024
TILE = THREADS * G
WAVE = 64 * G
RUN_BYTE = 0xFB  # the only byte whose runs of more than 5 survive the first run-length step


def plain(n, seed, lo=0, hi=200):
    """n bytes in [lo, hi), no two neighbours equal: the first run-length step
    leaves them as they are, and no byte is RUN_BYTE."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, hi - lo, n)
    return (lo + (int(rng.integers(0, hi - lo)) + np.cumsum(step)) % (hi - lo)).astype(np.uint8)


def run_piece(length):
    """Raw bytes whose text is `length` equal bytes (2, 3: as they are; 7, 8, 9:
    255 RUN_BYTEs become 4 and the count 251 == RUN_BYTE, then 2, 3 or 4 more;
    after 4 more the count byte 0 follows)."""
    if length <= 3:
        return np.full(length, 0x50, np.uint8)
    return np.full(255 + length - 5, RUN_BYTE, np.uint8)


def with_run(raw_len, length, end, seed):
    """A raw stream of raw_len bytes whose text has a run of `length` equal
    bytes ending at text position `end` (end=None: at the text's last
    position; for 9 bytes, 8 at the end and one at the start: a 9-byte run can
    only close the text across the wrap, a count byte follows it otherwise)."""
    piece = run_piece(length)
    if end is None:
        if length == 9:
            piece = run_piece(8)
            raw = np.concatenate([[RUN_BYTE], plain(raw_len - len(piece) - 1, seed), piece]).astype(np.uint8)
        else:
            raw = np.concatenate([plain(raw_len - len(piece), seed), piece])
    else:
        p = end - length + 1
        raw = np.concatenate([plain(p, seed), piece, plain(raw_len - p - len(piece), seed + 1)])
    assert len(raw) == raw_len
    T = M.rle1(raw)
    b = T[len(T) - 1 if end is None else end]
    run = 1
    e = len(T) - 1 if end is None else end
    while T[(e - run) % len(T)] == b:
        run += 1
    fwd = 0
    while T[(e + 1 + fwd) % len(T)] == b:
        fwd += 1
    assert run + fwd == length and (fwd == 0 or end is None), (length, end, run, fwd)
    return raw


def mode_of(T):
    """M.kernel_mode, also for texts shorter than its 8-byte lookahead (a
    non-constant text of fewer than 9 bytes has no 9 equal bytes in a row)."""
    T = np.asarray(T, np.uint8)
    if len(T) >= 8:
        return M.kernel_mode(T)
    if (T == T[0]).all():
        return M.FULL
    _, placed = M.scan_view(T, M.SORT_A)
    nb = int(placed.sum())
    return M.SORT_A if nb * 8 >= (len(T) - nb) * 7 else M.SORT_B


def check_batch(lfmlib, oracle, gpu, rows, modes=None):
    """Encode equal-length raw streams in one batch; each must stay on the
    device and match the reference.  modes: the mode each text must run in
    (None: not kModeFull)."""
    for i, raw in enumerate(rows):
        T = M.rle1(raw)
        assert not M.is_periodic(T), i
        mode = mode_of(T)
        if modes is None:
            assert mode != M.FULL, i
        else:
            assert mode == modes[i], (i, mode, modes[i])
    got, flags = encode(lfmlib, gpu, rows)
    for i, raw in enumerate(rows):
        assert flags[i] == 0, i
        assert got[i] == ref_bz2(oracle, np.asarray(raw, np.uint8).tobytes(), 2), i


LENGTHS = list(range(1, G + 3)) + [TILE - 1, TILE, TILE + 1, TILE + G - 1, 2 * TILE + 1, WAVE - 1, WAVE + 1]
# (threads * G +- 1 are TILE +- 1: every thread walks one group of a tile)


@pytest.mark.parametrize("n", LENGTHS)
def test_text_lengths(lfmlib, oracle, gpu, n):
    """Texts of n bytes after the first run-length step: shorter than a
    group, one byte around a group's, a wave's and a tile's end, the last
    group cut inside the lookahead, three tiles."""
    rows = [plain(n, 100 + s) for s in range(3)] + [M.bench_like(n, 7, p=0.3)]
    rows = [r for r in rows if len(M.rle1(r)) == n and not M.is_periodic(r)]
    assert len(rows) >= 3
    # (a text of one byte is 9 equal bytes in a row, cyclically: kModeFull)
    check_batch(lfmlib, oracle, gpu, rows, [M.FULL] * len(rows) if n == 1 else None)


@pytest.mark.parametrize("length", [2, 3, 7, 8, 9])
def test_equal_runs_at_the_seams(lfmlib, oracle, gpu, length):
    """A run of `length` equal bytes ending on a group's, a wave's, a tile's
    and the text's last position (decided across the wrap), followed by a
    smaller and by a larger byte.  Nine equal bytes leave a type undecided:
    kModeFull."""
    raw_len = TILE + 1200
    ends = [5 * G + G - 1, WAVE - 1, 3 * WAVE - 1, TILE - 1, None]
    rows = [with_run(raw_len, length, e, 300 + 10 * i) for i, e in enumerate(ends)]
    if length in (7, 8):  # followed by a larger byte (plain() stays below RUN_BYTE)
        for e in ends[:-1]:
            r = with_run(raw_len, length, e, 400).copy()
            r[int(np.flatnonzero(r == RUN_BYTE)[-1]) + 1] = 0xFE
            rows.append(r)
    check_batch(lfmlib, oracle, gpu, rows, [M.FULL] * len(rows) if length == 9 else None)


def test_deepest_lookahead(lfmlib, oracle, gpu):
    """Exactly eight equal bytes that start on a group's last position: the
    byte that decides the type is the sixteenth byte of the lane's load.  A
    smaller and a larger byte after the run, in the first tile, at a tile's
    end (the bytes kept past the tile) and at the text's end (the wrap)."""
    raw_len = TILE + 601
    rows = []
    for k in (20 * G, WAVE - G, TILE - G):
        for larger in (False, True):
            r = with_run(raw_len, 8, k + 14, 500 + k).copy()
            if larger:
                r[int(np.flatnonzero(r == RUN_BYTE)[-1]) + 1] = 0xFD
            T = M.rle1(r)
            assert T[k + 6] != RUN_BYTE and (T[k + 7:k + 15] == RUN_BYTE).all() and (T[k + 15] > RUN_BYTE) == larger
            rows.append(r)
    # the run closes the text and starts on a group's last position: T[0] decides
    r = with_run(raw_len, 8, None, 600)
    assert (len(M.rle1(r)) - 8) % G == G - 1
    rows.append(r)
    check_batch(lfmlib, oracle, gpu, rows)


def test_each_exit_of_the_mode_restart(lfmlib, oracle, gpu):
    """A kModeSortA, a kModeSortB and a kModeFull text of three tiles in one
    batch: the histogram walk runs once, twice (A, then B) and twice (A, then
    whole)."""
    n = 2 * TILE + 1
    full = np.concatenate([plain(n - 5000, 22), np.full(600, RUN_BYTE, np.uint8), plain(4400, 23)])
    rows = [M.bench_like(n, 12), M.triples_b(n, 13), full, M.ascending_runs(n, 14)]
    check_batch(lfmlib, oracle, gpu, rows, [M.SORT_A, M.SORT_B, M.FULL, M.SORT_A])


def test_hot_buckets(lfmlib, oracle, gpu):
    """16-bit symbols 0..3 only: nearly every sorted rotation falls into the
    four buckets (low byte < 4, zero high byte), whose counts and scatter
    atomics contend most."""
    n = TILE + 2 * G + 2
    rows = []
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        v = rng.integers(0, 4, n // 2).astype("<u2")
        v[v == 0] = rng.integers(0, 4, int((v == 0).sum()))  # fewer zeros
        rows.append(v.view(np.uint8).copy())
    for r in rows:
        T = M.rle1(r)
        mode = mode_of(T)
        _, placed = M.scan_view(T, mode)
        hot = (~placed) & (T < 4) & (np.roll(T, -1) < 4)
        assert hot.sum() > 0.8 * (~placed).sum() > 1000
    check_batch(lfmlib, oracle, gpu, rows)


def test_zero_first_bytes_live_and_dead(lfmlib, oracle, gpu):
    """Unsorted rotations that start with byte 0 are counted by popcounts:
    live ones (0x0000 symbols: a zero before the zero) and dead ones (a
    non-zero low byte before every zero high byte)."""
    n = TILE + WAVE + 6
    rng = np.random.default_rng(50)
    live = M.bench_like(n, 51, p=0.5)
    dead = np.stack([rng.integers(1, 200, n // 2), np.zeros(n // 2, np.int64)], 1).reshape(-1).astype(np.uint8)
    both = np.where(np.arange(n) < n // 2, live, dead)
    rows = [live, dead, both]
    counts = []
    for r in rows:
        T = M.rle1(r)
        mode = M.kernel_mode(T)
        assert mode == M.SORT_A
        _, placed = M.scan_view(T, mode)
        z = placed & (T == 0)
        counts.append((int((z & M.live_rule(T, mode)).sum()), int((z & ~M.live_rule(T, mode)).sum())))
    print("zero-first unsorted rotations (live, dead):", counts)
    assert counts[0][0] > 500 and counts[1][0] == 0 and counts[1][1] > 2000 and min(counts[2]) > 300
    check_batch(lfmlib, oracle, gpu, rows)


def test_preceding_bytes_at_the_edges(lfmlib, oracle, gpu):
    """Rotation 0 carries T[n - 1]; the first position of the second tile
    carries the previous tile's last byte; a group's first position carries
    the previous lane's last byte.  Those bytes occur nowhere else in the
    text, so a wrong one changes the output."""
    n = TILE + 3 * G
    rows = []
    for seed, (at, val) in enumerate([(n - 1, 250), (TILE - 1, 251), (WAVE - 1, 252), (G - 1, 253)]):
        r = plain(n, 60 + seed)
        r[at] = val
        assert (r == val).sum() == 1 and len(M.rle1(r)) == n
        rows.append(r)
    check_batch(lfmlib, oracle, gpu, rows)
