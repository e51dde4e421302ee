"""The Huffman stage outside the merge trips against the reference bzip2,
byte for byte: huff_final's selector move-to-front as a scan (lanes of
kSelChunk = 32 selectors, passes of 64 lanes, csrc/lfm_sel_mtf.h) and its
codes on a wave per table, the partition walk in the first huff_select_reg
launch, and huff_lengths_heap's loads and level-wise inserts.

Rows are found on the CPU with the oracle by varying the row length; what a
row is there for (its selector count, its selectors, its table count, its
alphabet) is read back from the reference's stream with bz2_dissect and
asserted.  Every test is one bzip2_device call, and no stream may come back
flagged for the host library."""
import functools

import numpy as np
import pytest

import bz2_dissect as D
import lfm_oracle
from test_huff_heap_path_gpu import ALPHAS, alphabet_rows, alternating, check_batch, draw_row

pytestmark = pytest.mark.gpu

GROUP = 50       # kGSize
CHUNK = 32       # kSelChunk: selectors per lane
PASS = 64 * CHUNK
BANDS = (200, 600, 1200, 2400)  # nMTF from which 3, 4, 5, 6 tables are used


def _dissect(raw, level):
    return D.dissect(lfm_oracle.bzip2().compress(raw, level))


def _row(n, seed, values=256):
    return np.random.default_rng(seed).integers(0, values, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def row_with_symbols(want, level=2):
    """Random bytes whose reference stream has exactly `want` symbols (EOB
    included): the length follows the miss, then the seeds are walked."""
    n = max(want - 1, 1)
    for t in range(400):
        raw = _row(n, 31 * want + t)
        got = len(_dissect(raw, level)["syms"])
        if got == want:
            return raw
        if abs(got - want) > 3 or t % 8 == 7:  # (a few symbols off: another seed of this length may hit)
            n = max(n + want - got, 1)
    raise AssertionError("no row with %d symbols" % want)


def rows_beside(raw, seeds):
    """Other rows of raw's length: the call's other streams."""
    return [raw] + [_row(len(raw), 7000 + s) for s in seeds]


# selector counts at the seams of the scan: the lane chunk, 64, one wave pass
@pytest.mark.parametrize("nsel", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 63, 64, 65, PASS - 1, PASS, PASS + 1])
def test_selector_count(lfmlib, oracle, gpu, nsel):
    """The stream nearest the seam: one above a seam, the last selector's
    group holds one symbol (the shortest stream with nsel selectors), else 50
    (the longest)."""
    above = nsel - 1 in (1, CHUNK, 64, PASS)
    raw = row_with_symbols(GROUP * (nsel - 1) + 1 if above else GROUP * nsel)
    exp = check_batch(lfmlib, gpu, oracle, rows_beside(raw, (1, 2)))
    d = D.dissect(exp[0])
    assert d["nsel"] == nsel and len(d["syms"]) % GROUP == (1 if above else 0)


def test_selector_passes_with_carry(lfmlib, oracle, gpu):
    """A level-9 row of 250 000 bytes: 5 000 selectors, three passes of the
    scan with the list carried from each into the next."""
    raw = draw_row(254, 250000, 1, False)
    exp = check_batch(lfmlib, gpu, oracle, [raw, draw_row(200, 250000, 2, True)], level=9)
    assert all(D.dissect(e)["nsel"] > 2 * PASS for e in exp)


def test_selectors_all_equal(lfmlib, oracle, gpu):
    """Four byte values, near-equal frequencies: six tables, and one of them
    takes every group (chunks of one repeated symbol, summaries of one)."""
    exp = check_batch(lfmlib, gpu, oracle, [draw_row(4, 5953, s, False) for s in (0, 1, 2)])
    d = D.dissect(exp[0])
    assert d["nsel"] > 3 * CHUNK and len(set(d["selectors"])) == 1 and d["ngroups"] == 6


def alternating_text(words, block):
    """Words p 1 h l with increasing keys h l (as bz2_encode_cases.odd_values):
    the rotations that start with 1 are sorted by word, so their column is the
    p in text order.  The p of `block` words run through five values in turn
    (move-to-front value 4), those of the next `block` through two (value 1):
    with block = 50 every other group of that stretch favours another table."""
    out = bytearray()
    for i in range(words):
        p = 10 + i % 2 if (i // block) & 1 else 20 + i % 5
        out += bytes([p, 1, 60 + i // 190, 60 + i % 190])
    return bytes(out)


def longest_alternation(sel):
    """Length of the longest stretch a b a b ... (a != b) of sel."""
    best = cur = 2 if len(sel) > 1 and sel[0] != sel[1] else 1
    for i in range(2, len(sel)):
        cur = cur + 1 if sel[i] != sel[i - 1] and sel[i] == sel[i - 2] else (2 if sel[i] != sel[i - 1] else 1)
        best = max(best, cur)
    return best


def test_selectors_alternating(lfmlib, oracle, gpu):
    """A stretch of selectors that alternates between two tables over more
    than two lanes' chunks: summaries of two symbols, composed across lanes."""
    rows = [alternating_text(4000, b) for b in (50, 100, 37)]
    exp = check_batch(lfmlib, gpu, oracle, rows)
    assert longest_alternation(D.dissect(exp[0])["selectors"]) > 2 * CHUNK


def test_six_tables_inside_lane_chunks(lfmlib, oracle, gpu):
    """Runs of three equal bytes: six tables that change from group to group,
    so single lanes' chunks hold all six (summaries of six)."""
    rng = np.random.default_rng(77)
    rows = [np.repeat(rng.integers(0, 256, 20000 // 3 + 1, dtype=np.uint8), 3)[:20000].tobytes() for _ in range(3)]
    exp = check_batch(lfmlib, gpu, oracle, rows)
    sel = D.dissect(exp[0])["selectors"]
    full = [i for i in range(0, len(sel) - CHUNK + 1, CHUNK) if len(set(sel[i:i + CHUNK])) == 6]
    assert len(full) >= 2, len(full)


# table counts: the partition walk of the first select launch
@functools.lru_cache(maxsize=None)
def rows_at_band(band):
    """Rows of one length, the first with band - 1 symbols, the second with
    band, then the others drawn on the way (a few symbols either side)."""
    n = band
    for _ in range(30):  # eight byte values: zero runs, so rows of one length differ in their symbol counts
        rows = [_row(n, 8000 + s, 8) for s in range(40)]
        nsym = [len(_dissect(r, 2)["syms"]) for r in rows]
        if band - 1 in nsym and band in nsym:
            a, b = nsym.index(band - 1), nsym.index(band)
            return [rows[a], rows[b]] + [r for i, r in enumerate(rows[:12]) if i not in (a, b)]
        n += (band - sorted(nsym)[20]) or 1
    raise AssertionError("no rows on both sides of %d symbols" % band)


@pytest.mark.parametrize("band", BANDS)
def test_table_count(lfmlib, oracle, gpu, band):
    """nMTF one below and at a band of nGroups, and a few symbols either side
    (other partitions for the walk, its odd-group step back among them)."""
    exp = check_batch(lfmlib, gpu, oracle, rows_at_band(band))
    groups = 2 + BANDS.index(band)
    ds = [D.dissect(e) for e in exp[:2]]
    assert [len(d["syms"]) for d in ds] == [band - 1, band] and [d["ngroups"] for d in ds] == [groups, groups + 1]


# heaps
def test_heaps_shallow_beside_deep(lfmlib, oracle, gpu):
    """Small alphabets alternate with large ones: the waves of
    huff_lengths_heap are mixed, their pops are at different positions."""
    check_batch(lfmlib, gpu, oracle, alphabet_rows(2500, 900), alphas=ALPHAS)


def test_heaps_all_258(lfmlib, oracle, gpu):
    """Every stream has 258 symbols and six tables: whole waves of heaps of
    one size."""
    rows = [draw_row(256, 3000, 600 + i, bool(i & 1)) for i in range(40)]
    exp = check_batch(lfmlib, gpu, oracle, rows)
    ds = [D.dissect(e) for e in exp]
    assert {d["alpha"] for d in ds} == {258} and {d["ngroups"] for d in ds} == {6}


def test_heap_retry_beside_ordinary(lfmlib, oracle, gpu):
    """test_gpu's geometric row (a tree longer than 17 bits in an early pass:
    the halving retry.  A stream cannot show the retry; the witness is the
    depth the reference's tables reach, 15, as in bz2_encode_cases) between
    ordinary rows."""
    from test_gpu import _bz2_cases
    geo = _bz2_cases()["geometric"].tobytes()
    rows = [draw_row(k, len(geo), 700 + k, False) for k in alternating([a - 2 for a in ALPHAS])[:4]]
    rows.insert(2, geo)
    exp = check_batch(lfmlib, gpu, oracle, rows)
    d = D.dissect(exp[2])
    assert max(max(ln) for ln in d["lengths"]) == 15 and d["ngroups"] == 6


def test_heap_wide_beside_narrow(lfmlib, oracle, gpu):
    """One row of 140 000 run-free bytes (nMTF + alphaSize >= 2^17: u64
    entries) beside rows of tripled bytes, which stay narrow."""
    n = 140000
    rng = np.random.default_rng(801)
    rows = [np.repeat(rng.integers(0, k, n // 3 + 1, dtype=np.uint8), 3)[:n].tobytes() for k in (40, 200, 256)]
    rows.insert(1, draw_row(254, n, 802, False))
    exp = check_batch(lfmlib, gpu, oracle, rows, level=2)
    wide = [len(d["syms"]) + d["alpha"] >= 1 << 17 for d in (D.dissect(e) for e in exp)]
    assert wide == [False, True, False, False]
