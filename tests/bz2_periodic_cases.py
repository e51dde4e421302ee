"""A model of how libbzip2 decodes a block whose text after RLE1 is exactly
periodic, and the inputs of the periodic-block tests, shared by
test_bunzip2_periodic_cpu.py (the model and the inputs' premises, against
libbzip2 on the host) and test_bunzip2_periodic_gpu.py.  TEST INFRASTRUCTURE
ONLY.

The rule (decompress.c): n steps along tt from tt[origPtr].  The LF
permutation of w w ... w (r copies of a primitive w of q bytes) has r cycles
of q rows each, so the walk goes n / q times round the start's cycle."""
import functools

import numpy as np

import bz2_cases as K
from bz2_craft import craft, sorted_rotations

MARK, KEEP = 128, 512  # kMark and kWalkKeep of csrc/lfm_bunzip2.hip


def rotations(text):
    """bz2_craft.sorted_rotations (equal rotations in index order) by prefix
    doubling: the same list, in n log^2 n."""
    a = np.frombuffer(bytes(text), np.uint8).astype(np.int64)
    n, idx, k = len(a), np.arange(len(a)), 1
    rank = a
    while True:
        nxt = rank[(idx + k) % n]
        order = np.lexsort((nxt, rank))
        r1, r2 = rank[order], nxt[order]
        new = np.zeros(n, np.int64)
        new[order[1:]] = np.cumsum((r1[1:] != r1[:-1]) | (r2[1:] != r2[:-1]))
        rank, k = new, 2 * k
        if k >= n:
            break
    return [int(i) for i in np.lexsort((idx, rank))]


def build_tt(text, rot=None):
    """(ll, tt) as decompress.c builds them (bz2_cases.chain_wraps): ll the
    last column, tt[LF(i)] = i."""
    n = len(text)
    rot = rotations(text) if rot is None else rot
    ll = [text[i - 1] for i in rot]
    count = [0] * 257
    for c in ll:
        count[c + 1] += 1
    for c in range(256):
        count[c + 1] += count[c]
    tt = [0] * n
    for i, c in enumerate(ll):
        tt[count[c]] = i
        count[c] += 1
    return ll, tt


def start_cycle(ll, tt, orig):
    """The rows of the start's cycle, in walk order from tt[orig]."""
    rows, pos = [], tt[orig]
    while True:
        rows.append(pos)
        pos = tt[pos]
        if pos == tt[orig]:
            return rows


def model(text, orig, rot=None):
    """(q, bytes): the start cycle's length and its bytes repeated to n, which
    is libbzip2's n steps from origPtr."""
    ll, tt = build_tt(text, rot)
    cyc = bytes(ll[p] for p in start_cycle(ll, tt, orig))
    q, n = len(cyc), len(text)
    return q, (cyc * (n // q + 1))[:n]


def segments(text, orig, rot=None):
    """Lengths of bzd_walk's segments on the start's cycle: from one marker (a
    row that is a multiple of kMark, or the start tt[orig]) to the next."""
    ll, tt = build_tt(text, rot)
    rows = start_cycle(ll, tt, orig)
    cuts = [k for k, p in enumerate(rows) if p % MARK == 0 or k == 0]
    return [b - a for a, b in zip(cuts, cuts[1:] + [len(rows)])]


def tied_origs(text, m, rot=None):
    """The sorted rows of the rotations 0, m, 2 m, ...: every origPtr that
    stands for the text w w ... w with |w| = m."""
    rot = rotations(text) if rot is None else rot
    return [rot.index(j) for j in range(0, len(text), m)]


SEAM_MS = (2, 3, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1300)
SEAM_RS = (2, 3, 7)
SEAM_STRIDE = 12289


@functools.lru_cache(maxsize=None)
def long_segment_text():
    """(text, m, orig): w w w with |w| = 3000 and a tied origPtr whose cycle has
    markers of its own and a segment longer than kWalkKeep next to shorter
    ones (found by search with the model)."""
    for seed in range(200):
        m = 3000
        text = K.noruns(m, 900 + seed) * 3
        rot = rotations(text)
        for orig in tied_origs(text, m, rot):
            seg = segments(text, orig, rot)
            if len(seg) > 4 and max(seg) > KEEP and min(seg) < MARK:
                return text, m, orig
    raise AssertionError("no text with a long segment found")


@functools.lru_cache(maxsize=None)
def seam_cases():
    """[(name, text, stream)]: texts noruns(m) * r crafted at level 1 (RLE1 is
    the identity on them), for the periods around the fill's 16-byte stores,
    kMark and kWalkKeep; with every tied origPtr for r = 3 and for m = 1300
    (r = 2, the second row: every regular marker lies on the other cycle, so
    the start's cycle is one segment of 1300 bytes, longer than kWalkKeep).
    Then thousands of 2-cycles, q = 1, and long_segment_text()."""
    out = []

    def add(name, text, m, all_origs):
        rot = rotations(text)
        origs = tied_origs(text, m, rot)
        for j, orig in enumerate(origs if all_origs else origs[:1]):
            out.append(("%s_o%d" % (name, j), text, craft(text, level=1, orig_override=orig)[0]))

    for m in SEAM_MS:
        for r in SEAM_RS:
            if m * r < SEAM_STRIDE:
                add("m%d_r%d" % (m, r), K.noruns(m, 40 + m) * r, m, r == 3 or m == 1300)
    add("m2_r4500", K.noruns(2, 7) * 4500, 2, False)
    name, data, stream, _, _ = [c for c in K.crafted_good() if c[0] == "ninuse1_n5"][0]
    out.append((name, data, stream))
    text, m, orig = long_segment_text()
    out.append(("long_segment", text, craft(text, level=1, orig_override=orig)[0]))
    return out


@functools.lru_cache(maxsize=None)
def wrong_start():
    """(text, stream, model's bytes): w w with an origPtr that names the row
    of rotation 1, which is not one of rotation 0's equal rows: libbzip2 walks
    the other text's cycle and the CRC does not match."""
    text = K.noruns(31, 1, 200) * 2
    rot = sorted_rotations(text)
    orig = rot.index(1)
    assert orig not in tied_origs(text, 31, rot)
    return text, craft(text, level=1, orig_override=orig)[0], model(text, orig, rot)[1]
