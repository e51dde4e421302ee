"""The case list of the run-head tests of the GPU bzip2 encoder's MTF stage
(mtf_win walks only the run heads of the BWT column), shared by
test_mtf_run_heads_cpu.py (the premises, against the reference library's own
streams) and test_mtf_run_heads_gpu.py.  TEST INFRASTRUCTURE ONLY.

A case is (id, raw bytes, witness), as in bz2_encode_cases.py: witness(raw, d)
asserts the column property the id names on d = dissect(reference stream) and
returns the facts it found.

Notation: S = 4096 (kSeg, one wave's segment), W = 64 (one load of the
column).  A position is a *head* when it is its segment's first position or
its column symbol differs from the one before it; that is how the kernel
counts them.  The kernel takes a load with DENSE heads or more as a window as
it stands, after emptying its ring of pending heads; the heads of any other
load go into the ring, which gives up 64 whenever it holds as many
(ring_before below restates that).

Construction.  The column is written directly instead of searched for: a text
of four-byte words  p_i M h_i l_i  with a marker byte M that occurs nowhere
else and keys (h_i, l_i) that grow with i sorts its rotations that start with
M by i, so the column in front of them is p_0 p_1 ... in text order.  With
M = 1, the smallest byte of the text, these are the column's first positions;
with M = 255, the largest, its last.  No byte run is longer than two, so RLE1
leaves the text alone and the column is as long as the row.  p is drawn from
run_free (never two equal neighbours) and stretched into runs as the case
needs.  Every witness checks the planted column on the reference's stream
first.  The workload-like row is searched by seed (_search) until its head
fraction is the one its id states."""
import functools

import numpy as np

from bz2_craft import is_periodic
from bz2_dissect import bwt_column, mvals
from bz2_encode_cases import LEVEL, _facts, _search, ref_dissect
from bz2_parts import nblock_max, run_free

S, W = 4096, 64
DENSE = 48          # kMtfDense
WORDS = 9216          # planted column positions of the standard row: segments 0, 1 and a quarter of 2
ROW = 4 * WORDS       # 36 864 bytes
P_LO, P_N = 10, 50    # the planted symbols: 10 .. 59
K_LO, K_N = 60, 190   # the key bytes: 60 .. 249


# ---------------------------------------------------------------- helpers --
def column_and_values(d):
    vals, runs = mvals(d["syms"])
    return bwt_column(vals, d["used"]), vals, runs


def heads_of(col):
    """Boolean array: position j is a head."""
    col = np.asarray(col)
    h = np.ones(len(col), bool)
    h[1:] = col[1:] != col[:-1]
    h[::S] = True
    return h


def heads_per_segment(col):
    h = heads_of(col)
    return [int(h[a:a + S].sum()) for a in range(0, len(col), S)]


def symbols(n, seed):
    """n planted symbols, no two neighbours equal (run_free's 5..244 folded
    onto P_N values would repeat; a walk with non-zero steps does not)."""
    rng = np.random.default_rng(seed)
    return (P_LO + np.cumsum(rng.integers(1, P_N, n, dtype=np.int64)) % P_N).astype(np.uint8)


def stretch(lengths, seed):
    """Runs of the given lengths, neighbouring runs of different symbols."""
    lengths = np.asarray(lengths, np.int64)
    assert (lengths > 0).all()
    return np.repeat(symbols(len(lengths), seed), lengths)


def split_runs(total, count, seed):
    """`count` run lengths >= 2 that sum to `total`, uneven."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, total // 2), count - 1, replace=False)) * 2
    out = np.diff(np.concatenate(([0], cuts, [total])))
    assert len(out) == count and out.sum() == total and (out >= 2).all()
    return out


def join(*parts):
    """Concatenate planted stretches; a part that would start with the symbol
    the one before it ends in is rotated within the alphabet, so that the seam
    is a head (the cases that want a run over a seam build it in one part)."""
    out = []
    for p in parts:
        p = np.asarray(p, np.uint8).copy()
        if out and len(p) and p[0] == out[-1][-1]:
            p = (P_LO + (p - P_LO + 1) % P_N).astype(np.uint8)
        out.append(p)
    return np.concatenate(out)


def words(ps, marker, tail=b""):
    ps = np.asarray(ps, np.uint8)
    n = len(ps)
    assert n <= K_N * K_N and marker in (1, 255) and ps.min() >= P_LO and ps.max() < P_LO + P_N
    i = np.arange(n)
    w = np.stack([ps, np.full(n, marker, np.uint8), (K_LO + i // K_N).astype(np.uint8), (K_LO + i % K_N).astype(np.uint8)], 1)
    raw = w.tobytes() + bytes(tail)
    assert not is_periodic(raw) and 4096 <= len(raw) < min(41000, nblock_max(LEVEL))
    return raw


def planted(raw, d, ps, marker):
    """The reference's column, values and zero runs, after checking that the
    planted positions hold ps."""
    col, vals, runs = column_and_values(d)
    assert len(col) == len(raw), "RLE1 changed the text"
    got = col[:len(ps)] if marker == 1 else col[len(col) - len(ps):]
    assert np.array_equal(got, ps), "the planted column is not where the words put it"
    return col, vals, runs


def _case(cid, ps, check, marker=1, tail=b""):
    ps = np.asarray(ps, np.uint8)
    raw = words(ps, marker, tail)

    def witness(raw, d):
        col, vals, runs = planted(raw, d, ps, marker)
        return check(col, vals, runs)
    return (cid, raw, witness)


def _fill(ps, seed):
    """ps followed by dense symbols up to WORDS positions."""
    assert len(ps) <= WORDS
    return join(ps, symbols(WORDS - len(ps), seed)) if len(ps) < WORDS else np.asarray(ps, np.uint8)


# ------------------------------------------------------------------ cases --
def _one_head_after_63():
    """1, 2 (63), 5: segment 0 has 63 heads; segment 1 is one symbol, the one
    segment 0 ends in, so the run covers S - 1 and S and the forced head at S
    has value 0."""
    seg0 = stretch(split_runs(S, 63, 11), 12)
    ps = _fill(np.concatenate([seg0, np.full(S, seg0[-1], np.uint8)]), 13)

    def check(col, vals, runs):
        hs = heads_per_segment(col)
        assert hs[0] == 63 and hs[1] == 1 and col[S - 1] == col[S] and (col[S:2 * S] == col[S]).all()
        assert vals[S] == 0
        return _facts(heads=hs[:2], symbol=int(col[S]), value_at_S=int(vals[S]))
    return _case("seg-1-head-after-63", ps, check)


def _heads_64_65():
    """2 (64, 65): the ring fills exactly once / leaves one head at the flush."""
    ps = _fill(join(stretch(split_runs(S, 64, 21), 22), stretch(split_runs(S, 65, 23), 24)), 25)

    def check(col, vals, runs):
        hs = heads_per_segment(col)
        assert hs[:2] == [64, 65]
        return _facts(heads=hs[:2])
    return _case("seg-64-65-heads", ps, check)


def _heads_128():
    """2 (128): two full windows and no flush; then a dense segment."""
    ps = _fill(stretch(split_runs(S, 128, 31), 32), 33)

    def check(col, vals, runs):
        hs = heads_per_segment(col)
        assert hs[0] == 128 and hs[1] == S
        return _facts(heads=hs[:2])
    return _case("seg-128-heads", ps, check)


def ring_before(per_load):
    """Heads pending in the kernel's ring in front of each load of a segment."""
    out, cnt = [], 0
    for nh in per_load:
        out.append(cnt)
        cnt = 0 if nh >= DENSE else (cnt + int(nh)) % W
    return out


def _load_seams():
    """3, 4, 6: in segment 0 a run over positions W - 1 | W and a run that ends
    exactly on 2 W - 1; in segment 1 loads of 21, 21 and 21 heads, then one of
    47 (the ring at its fullest, 63 + 47), one of 64 heads (the ring holds 46)
    and 24 loads of one head each."""
    seg0 = join(stretch([60, 8, 58, 2], 41), stretch(split_runs(S - 128, 300, 42), 43))
    per = [21, 21, 21, 47, 64]
    loads = [stretch(split_runs(W, 21, 44 + i), 144 + i) for i in range(3)] + [_load_of(47, 147), symbols(W, 45)]
    sparse = stretch([W] * 24, 46)                    # heads on lane 0 only
    seg1 = join(*loads, sparse, symbols(S - 29 * W, 47))
    ps = _fill(join(seg0, seg1), 48)

    def check(col, vals, runs):
        h = heads_of(col)
        assert col[W - 1] == col[W] and not h[W]
        assert col[2 * W - 2] == col[2 * W - 1] != col[2 * W] and h[2 * W]
        per_load = h[S:2 * S].reshape(-1, W).sum(1)
        before = ring_before(per_load)
        assert per_load[:5].tolist() == per and before[3] == 63 and before[4] == 46 and (per_load[5:29] == 1).all()
        return _facts(run_over=(W - 1, W), run_ends=2 * W - 1, ring_before_load3=before[3], heads_load3=int(per_load[3]))
    return _case("load-seams-ring-110", ps, check)


def _load_of(heads, seed):
    """One load of W positions with `heads` runs (of one or two positions)."""
    lens = np.array([2] * (W - heads) + [1] * (2 * heads - W))
    return stretch(np.random.default_rng(seed).permutation(lens), seed + 1)


def _dense_threshold():
    """The kernel takes a load of DENSE = 48 heads or more as a window of its
    own once the ring is empty: loads of 47, 48 (ring holds 47), 48 (ring
    empty), 47 and 64 heads (ring holds 47), then one head per load."""
    per = [47, 48, 48, 47, 64]
    seg0 = join(*[_load_of(h, 90 + 2 * i) for i, h in enumerate(per)], stretch([W] * 20, 101), symbols(S - 25 * W, 102))
    ps = _fill(join(seg0, stretch(split_runs(S, 200, 103), 104)), 105)

    def check(col, vals, runs):
        h = heads_of(col)
        got = h[:S].reshape(-1, W).sum(1)
        assert got[:5].tolist() == per and (got[5:25] == 1).all()
        return _facts(heads_per_load=got[:6].tolist())
    return _case("dense-threshold-47-48", ps, check)


def _slow_window():
    """7, 9: runs of ten positions (under 8 heads a load), so the first window
    of segment 0 gathers its 64 heads from ten loads; heads 3, 4, 5 are
    a..a b..b a..a, and the second a has value 1."""
    sy = symbols(410, 51)
    sy[5] = sy[3]
    assert sy[4] != sy[3] and sy[6] != sy[5]
    seg0 = np.repeat(sy, 10)[:S]
    ps = _fill(join(seg0, symbols(S, 52)), 53)

    def check(col, vals, runs):
        pos = np.flatnonzero(heads_of(col)[:S])
        span = int(pos[63] - pos[0])
        assert span > 8 * W
        a, b, a2 = pos[3], pos[4], pos[5]
        assert col[a] == col[a2] != col[b] and b - a >= 2 and a2 - b >= 2 and pos[6] - a2 >= 2
        assert vals[a2] == 1 and (vals[a2 + 1:pos[6]] == 0).all()
        return _facts(first_window_spans=span, aba_heads=(int(a), int(b), int(a2)), value=int(vals[a2]))
    return _case("window-over-10-loads-aba", ps, check)


def _dense_sparse(order):
    """8: a dense segment (every position a head) next to a sparse one (128
    heads) in the workgroup of segments 0 .. 3, in both orders."""
    dense, sparse = symbols(S, 61), stretch(split_runs(S, 128, 62), 63)
    ps = _fill(join(dense, sparse) if order == "dense-sparse" else join(sparse, dense), 64)

    def check(col, vals, runs):
        hs = heads_per_segment(col)
        want = hs[:2] if order == "dense-sparse" else hs[1::-1]
        assert want[0] >= 4000 and want[1] <= 200
        return _facts(heads=hs[:2])
    return _case(order, ps, check)


def _last_segment(rest, run):
    """10: the last segment holds n mod S = rest positions and the column ends
    in a run of `run` equal symbols, the stream's last zero run (marker 255:
    the planted positions are the column's last)."""
    n = S + rest
    nw, tail = divmod(n, 4)
    ps = join(symbols(nw - run, 70 + rest), stretch([run], 80 + rest))

    def check(col, vals, runs):
        assert len(col) == n and n % S == rest
        assert (col[n - run:] == col[n - 1]).all() and col[n - run - 1] != col[n - 1]
        assert runs and runs[-1] == (n - run + 1, run - 1)
        return _facts(n=n, last_segment=rest, final_zero_run=runs[-1])
    return _case("last-segment-%d" % rest, ps, check, marker=255, tail=bytes([3, 7, 5][:tail]))


def _pixels(seed):
    """11: u16 little-endian pixels, low byte random in 0..63, high byte 0
    with about 1 % ones."""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.integers(0, 64, ROW // 2, dtype=np.uint8), (rng.random(ROW // 2) < 0.01).astype(np.uint8)], 1)
    return px.tobytes()


def _pixel_check(col):
    """The rotations that start at a low byte follow the (mostly zero) high
    byte: about half of the column repeats its predecessor."""
    frac = float(heads_of(col).mean())
    assert len(col) < nblock_max(LEVEL) and 0.45 <= frac <= 0.60, frac
    return frac


def _workload_like():
    def ok(d):
        try:
            _pixel_check(column_and_values(d)[0])
            return True
        except AssertionError:
            return False
    raw = _search(lambda t: _pixels(1100 + t), ok, "a pixel row with about half of its column as heads", tries=8)

    def witness(raw, d):
        col, vals, runs = column_and_values(d)
        frac = _pixel_check(col)
        hs = heads_per_segment(col)
        return _facts(head_fraction=round(frac, 4), heads_min=min(hs), heads_max=max(hs))
    return ("pixels-u16", raw, witness)


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, raw, witness)]: the rows of ROW bytes first, then the three rows
    whose length is their point."""
    out = [_one_head_after_63(), _heads_64_65(), _heads_128(), _load_seams(), _dense_threshold(), _slow_window(),
           _dense_sparse("dense-sparse"), _dense_sparse("sparse-dense"), _workload_like()]
    out += [_last_segment(1, 3), _last_segment(63, 5), _last_segment(65, 2)]
    return out


MIXED = ("seg-1-head-after-63", "seg-64-65-heads", "seg-128-heads", "dense-sparse", "sparse-dense", "pixels-u16")


def mixed_batch():
    """Cases 1, 2, 8 and 11 side by side: rows of one length for one call."""
    by_id = {cid: raw for cid, raw, _ in cases()}
    rows = [(cid, by_id[cid]) for cid in MIXED]
    assert len(set(len(raw) for _, raw in rows)) == 1
    return rows
