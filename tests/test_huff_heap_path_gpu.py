"""huff_lengths_heap (the path sift over pref bits, csrc/lfm_huff_heap.h)
against the reference bzip2, byte for byte, at the heap sizes where the sift
changes its level count and the pref bits change their word.

Rows are drawn over k distinct byte values with no run of four equal bytes, so
RLE1 adds no count byte and alphaSize = k + 2; the alphabets met are read back
from the reference's streams (tests/bz2_dissect.py).  Neighbouring rows
alternate small and large alphabets: a wave of 32 (stream, table) heaps then
holds shallow heaps beside deep ones.  Every test is one bzip2_device call, and
no stream may come back flagged for the host library."""
import numpy as np
import pytest

import bz2_dissect as D
from test_bwt_induce_compact_gpu import ref_bz2

pytestmark = pytest.mark.gpu

# heap sizes at which a level is added (4, 8, .. 256 entries), one each side,
# and the pref words' first and last nodes (alphaSize / 2 = 32, 64, 96 .. 129)
ALPHAS = [5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 131, 255, 256, 257, 258]
LEVEL = 2


def draw_row(k, n, seed, skew):
    """n bytes over exactly k values (k <= n), no four equal in a row; skew:
    value frequencies fall off as 1 / rank (else near-equal: many ties)."""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(256)[:k].astype(np.uint8)
    p = 1.0 / np.arange(1, k + 1) if skew else np.ones(k)
    x = rng.choice(k, n, p=p / p.sum())
    x[:k] = rng.permutation(k)  # every value is in use
    while True:
        run4 = np.flatnonzero((x[3:] == x[2:-1]) & (x[2:-1] == x[1:-2]) & (x[1:-2] == x[:-3])) + 3
        if not len(run4):
            break
        x[run4[::2]] = (x[run4[::2]] + 1) % k  # (k >= 2) the runs' last bytes, every other one of a long run
    assert len(np.unique(x)) == k
    return vals[x].tobytes()


def alternating(ks):
    """small, large, next small, next large ..."""
    ks = sorted(ks)
    out = []
    while ks:
        out.append(ks.pop(0))
        if ks:
            out.append(ks.pop())
    return out


def alphabet_rows(n, seed):
    ks = alternating([a - 2 for a in ALPHAS if a - 2 <= n])
    return [draw_row(k, n, seed + 7 * i + k, skew) for skew in (False, True) for i, k in enumerate(ks)]


def check_batch(lfmlib, torch, oracle, rows, level=LEVEL, alphas=None):
    n = len(rows[0])
    assert all(len(r) == n for r in rows)
    d = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy()).cuda()
    got, flags = lfmlib.bzip2_device(d, [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], 1, level=level)
    exp = [ref_bz2(oracle, r, level) for r in rows]
    assert not any(flags), [i for i, f in enumerate(flags) if f]
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, bad
    if alphas is not None:
        met = {D.dissect(e)["alpha"] for e in exp[:len(rows) // 2]}  # (the second half: the same alphabets, skewed)
        assert met == set(alphas), sorted(set(alphas) ^ met)
    return exp


def test_six_tables_many_ties(lfmlib, oracle, gpu):
    """Rows of 2 500 bytes: six tables per stream (five where a small
    alphabet's zero runs leave fewer than 2 400 symbols), small frequencies."""
    exp = check_batch(lfmlib, gpu, oracle, alphabet_rows(2500, 100), alphas=ALPHAS)
    groups = [D.dissect(e)["ngroups"] for e in exp]
    assert set(groups) <= {5, 6} and groups.count(6) > len(groups) // 2


def test_rows_of_30000(lfmlib, oracle, gpu):
    check_batch(lfmlib, gpu, oracle, alphabet_rows(30000, 200), alphas=ALPHAS)


def test_two_tables_weights_of_one(lfmlib, oracle, gpu):
    """Rows of 150 bytes, the alphabets that fit: two tables, almost every
    frequency 0 or 1."""
    fit = [a for a in ALPHAS if a - 2 <= 150]
    exp = check_batch(lfmlib, gpu, oracle, alphabet_rows(150, 300), alphas=fit)
    assert {D.dissect(e)["ngroups"] for e in exp} == {2}


def test_skewed_trees_beside_ordinary_ones(lfmlib, oracle, gpu):
    """Geometric rows as test_gpu's geometric_small (first trees longer than
    17: the halving retry) between ordinary rows: a wave holds heaps that retry
    beside heaps that do not."""
    n = 30000
    rng = np.random.default_rng(400)
    rows = []
    for i, k in enumerate(alternating([a - 2 for a in ALPHAS])):
        rows.append(draw_row(k, n, 400 + i, bool(i & 1)))
        if i % 3 == 0:
            rows.append(np.minimum(rng.geometric(0.5, n) - 1, 40 + i).astype(np.uint8).tobytes())
    check_batch(lfmlib, gpu, oracle, rows)


def test_wide_heaps_beside_narrow(lfmlib, oracle, gpu):
    """Rows of 140 000 bytes at level 2: nMTF + alphaSize >= 2^17 gives u64
    entries (16 heaps per workgroup); two rows of tripled bytes, whose zero
    runs keep them under 2^17, take u32 entries in the same launch."""
    n = 140000
    rows = [draw_row(k, n, 500 + k + j, bool(j)) for j in (0, 1) for k in (62, 126, 254, 256)]
    rng = np.random.default_rng(501)
    for k in (40, 200):
        rows.insert(3 if k == 40 else 7, np.repeat(rng.integers(0, k, n // 3 + 1, dtype=np.uint8), 3)[:n].tobytes())
    exp = check_batch(lfmlib, gpu, oracle, rows, level=2)
    # the premise, from the reference's own streams: which rows are wide
    wide = [len(D.dissect(e)["syms"]) + D.dissect(e)["alpha"] >= 1 << 17 for e in (exp[0], exp[3], exp[7])]
    assert wide == [True, False, False]
