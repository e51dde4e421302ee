"""The case lists of the GPU bzip2 encoder's seam tests (everything after the
BWT and the first run-length step before it), shared by
test_bz2_encode_seams_cpu.py (the premises, against the reference library on
the host) and test_bzip2_seams_gpu.py.  TEST INFRASTRUCTURE ONLY.

A case is (id, raw bytes, witness).  The witness proves that the input puts
what its id names on the seam it names; it is a predicate over the raw bytes
(list A, B: RLE1 works on raw positions) or over dissect(reference stream)
(lists C to F), never over what the encoder under test wrote.  witness(raw, d)
returns a dict of the facts it found, or raises AssertionError; d is None for
the lists that do not need the reference stream (NEEDS_REF).

The streams of one GPU call all have the same length, so cases of one list
that may share a length are padded to it with distinct run-free tails here
(the witness is taken on the padded row); cases whose length is the point
(list A, the nMTF targets of lists E and F) stand alone and the GPU tests
group them by length.

alphaSize 3 and 4: a text of one byte value is periodic unless it is one byte
long, so the only alphaSize-3 stream the device encodes is a raw length of 1
(list A holds it, list D names it); two byte values give alphaSize 4 (b"aab").
"""
import functools

import numpy as np

import lfm_oracle
from bz2_craft import is_periodic
from bz2_dissect import bwt_column, dissect, mvals
from bz2_parts import nblock_max, pieces, run_free

# The kernel geometry the cases aim at, each with the constant of
# csrc/lfm_bzip2.hip it restates (test_bz2_encode_seams_cpu reads them back).
RLE1 = dict(CHUNK=32,       # kRleChunk: bytes per thread
            WAVE=2048,      # 64 lanes x kRleChunk
            TILE=16384,     # kRleTile = kRleThreads x kRleChunk
            UNIT=16,        # bytes per store of the text
            SLOW_FROM=224)  # carried piece length from which a chunk may walk sequentially
MTF = dict(WINDOW=64, ITER=256, SEG=4096)            # lanes, positions per mtf_last iteration, kSeg
RLE2 = dict(PER=64, WAVE=4096, TILE=16384)           # kRle2Per, 64 x kRle2Per, kRle2Tile
HUFF = dict(GROUP=50, BANDS=(200, 600, 1200, 2400), SEL_LOAD=64)  # kGSize, the nGroups bands, selectors per load
EMIT = dict(PER=16, ROUND=4096, SEL_SPLIT=256)       # kEmitC, kEmitThreads x kEmitC, selector share per thread

LEVEL = 2            # test_bwt_induce_compact_gpu.encode's level: the witnesses' streams
MULTI_BLOCK = 80000  # block size of the multi runs: max_parts(80000, 1) == 2
TRIES = 400
NEEDS_REF = {"A": False, "B": False, "C": True, "D": True, "E": True, "F": True}


def max_parts(block_bytes, level):
    """lfm_bz_caps.h max_parts: the slots a stream owns in the multi entry."""
    return (block_bytes + block_bytes // 4 + 1) // nblock_max(level) + 1


def from_img(dims0, bs0, bpp=1):
    """The from_img condition of lfm_hip_bzip2_blocks for a 16-byte aligned
    image: RLE1 reads the image itself (rle1_crc<true, .>), else gather_blocks
    copies the blocks first (rle1_crc<false, .>)."""
    return (bs0 * bpp) % 16 == 0 and (dims0 * bpp) % 16 == 0 and ((dims0 % bs0) * bpp) % 16 == 0


# ---------------------------------------------------------------- helpers --
def rle1_np(raw):
    """bz2_craft.rle1 with numpy (the rows here are up to 80 kB)."""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    start, length = pieces(a)
    if start.size == 0:
        return b""
    n = np.minimum(length, 4) + (length >= 4)
    out = np.repeat(a[start], n)
    end = np.cumsum(n) - 1
    out[end[length >= 4]] = (length[length >= 4] - 4).astype(np.uint8)
    return out.tobytes()


def text_len(raw):
    _, length = pieces(raw)
    return int((np.minimum(length, 4) + (length >= 4)).sum())


@functools.lru_cache(maxsize=None)
def ref_stream(raw, level=LEVEL):
    return lfm_oracle.bzip2().compress(raw, level)


@functools.lru_cache(maxsize=None)
def ref_dissect(raw, level=LEVEL):
    return dissect(ref_stream(raw, level))


def _search(make, ok, what, tries=TRIES):
    """The first make(k), k < tries, whose reference stream satisfies ok(d)."""
    for k in range(tries):
        raw = make(k)
        if raw is not None and ok(ref_dissect(raw)):
            return raw
    raise AssertionError("no input found for " + what)


def tail(n, seed, after=None):
    """n run-free bytes in 5..244 that do not start with `after`."""
    t = run_free(n + 1, seed=1000 + seed)
    return t[1:] if n and after is not None and t[0] == after else t[:n]


def pad(raw, n, seed):
    assert len(raw) <= n
    return raw + tail(n - len(raw), seed, raw[-1] if raw else None)


@functools.lru_cache(maxsize=None)
def multi_filler():
    """The whole blocks of the multi runs' grids: MULTI_BLOCK run-free bytes."""
    return tail(MULTI_BLOCK, 4242)


def rand_bytes(n, seed, alphabet=256):
    return np.random.default_rng(seed).integers(0, alphabet, n, dtype=np.uint8).tobytes()


def _facts(**kw):
    return kw


# ------------------------------------------------------- A: raw lengths --
LENGTH_SEAMS = (128, 256, 2048, 4096, 16384, 32768)
LENGTHS = tuple(range(1, 71)) + tuple(p + d for p in LENGTH_SEAMS for d in (-1, 0, 1)) + (32767, 49153)


@functools.lru_cache(maxsize=None)
def length_cases():
    """Every length as random bytes and over a four-symbol alphabet; a row is
    dropped only if its text is periodic (length 2 and 3 of a tiny alphabet)."""
    out = []
    for n in sorted(set(LENGTHS)):
        for name, alphabet in (("rand", 256), ("alpha4", 4)):
            raw = rand_bytes(n, 7 * n + alphabet, alphabet)
            if is_periodic(rle1_np(raw)):
                continue

            def witness(raw, d, n=n):
                assert len(raw) == n
                return _facts(length=n)
            out.append(("len%d-%s" % (n, name), raw, witness))
    return out


# ------------------------------------------------ B: RLE1 on raw positions --
RLE1_SEAMS = (32, 64, 2048, 16384, 32768)
RLE1_ROW = {32: 4096, 64: 4096, 2048: 4096, 16384: 20480, 32768: 36864}  # row length of the seam's batch
RUN_J = (0, 1, 2, 3, 4, 5)
RUN_R = (2, 3, 4, 5, 8, 255, 256, 259, 260, 510, 514, 765)
CARRY_J = (222, 223, 224, 225, 254, 255, 256)
CARRY_R = (0, 1, 2, 31, 32, 33)
RUN_BYTES = (1, 0xFB, 250)  # outside run_free's 5..244; 1 and 0xFB also occur as count bytes
SHRINK_BYTE = 2


def expected_pieces(a, R):
    return [(a + 255 * i, min(255, R - 255 * i)) for i in range((R + 254) // 255)]


def _run_witness(P, j, R, a):
    def witness(raw, d):
        start, length = pieces(raw)
        have = set(zip(start.tolist(), length.tolist()))
        want = expected_pieces(a, R)
        assert all(p in have for p in want), "the run's pieces are not in the row"
        facts = _facts(run_start=a, run_len=R, seam=P, text_offset=text_len(raw[:a]))
        if P is not None and a < P < a + R:  # the chunk at P starts inside a piece
            i = int(np.searchsorted(start, P, side="right")) - 1
            assert start[i] <= P < start[i] + length[i]
            carried = P - int(start[i])
            assert carried == j % 255 and (int(start[i]), int(length[i])) in want
            facts.update(carried=carried, piece_len=int(length[i]))
        return facts
    return witness


def _rle1_row(n, P, j, R, idx):
    """A run-free row of n bytes with a run of R bytes from P - j; where the run
    starts past byte 40 a run of 5 + k bytes near the front takes k bytes out of the
    text (k = idx mod 16), so that the text offset at the seam takes every
    value mod 16 (a plain prefix would leave it at the raw offset)."""
    a = P - j
    row = bytearray(run_free(n, seed=idx + 1))
    k = idx % 16
    if a >= 40:
        row[8:8 + 5 + k] = bytes([SHRINK_BYTE]) * (5 + k)
    b = RUN_BYTES[idx % 3]
    assert a >= 0 and a + R <= n
    row[a:a + R] = bytes([b]) * R
    return bytes(row)


@functools.lru_cache(maxsize=None)
def rle1_cases(extra=0):
    """{group: [(id, row, witness)]}: the rows of a group share a length, the
    table's plus `extra` (0: rows of whole 16-byte units, RLE1 reads the image;
    1: gather_blocks runs first)."""
    groups = {n: [] for n in sorted(set(RLE1_ROW.values()))}
    idx = 0
    for P in RLE1_SEAMS:
        n = RLE1_ROW[P] + extra
        combos = [(j, R) for j in RUN_J for R in RUN_R]
        combos += [(j, j + r) for j in CARRY_J for r in CARRY_R if P - j >= 0]
        for j, R in combos:
            row = _rle1_row(n, P, j, R, idx)
            groups[RLE1_ROW[P]].append(("P%d-j%d-R%d" % (P, j, R), row, _run_witness(P, j, R, P - j)))
            idx += 1
    # a run over a whole chunk, wave and tile, one byte beyond either end
    for name, lo, size in (("chunk", 96, 32), ("wave", 2048, 2048), ("tile", 16384, 16384)):
        base = 4096 if lo + size + 1 < 4096 else 36864
        row = bytearray(run_free(base + extra, seed=idx + 1))
        row[lo - 1:lo + size + 1] = bytes([250]) * (size + 2)
        groups[base].append(("whole-" + name, bytes(row), _run_witness(None, 0, size + 2, lo - 1)))
        idx += 1
    # a run as the stream's last bytes
    for R in (4, 5, 255, 259, 510):
        n = 4096 + extra
        row = run_free(n - R, seed=idx + 1) + bytes([RUN_BYTES[idx % 3]]) * R
        groups[4096].append(("last-R%d" % R, row, _run_witness(None, 0, R, n - R)))
        idx += 1
    return groups


@functools.lru_cache(maxsize=None)
def rle1_facts(extra=0):
    """{id: what the witness found} for every row of rle1_cases(extra)."""
    return {cid: witness(raw, None) for group in rle1_cases(extra).values() for cid, raw, witness in group}


@functools.lru_cache(maxsize=None)
def rle1_solo_cases():
    """Rows whose length is their point, each a call of its own: one chunk that
    is a single run of 4, and one byte value over three tiles and five bytes
    (also as whole 16-byte units)."""
    out = []
    for name, n in (("run4", 4), ("tiles3+5", 3 * 16384 + 5), ("tiles3+16", 3 * 16384 + 16)):
        out.append((name, bytes([7]) * n, _run_witness(None, 0, n, 0)))
    return out


# ------------------------------------------------ C: second run-length step --
RLE2_SEAMS = (64, 4096, 16384)
RLE2_SMALL, RLE2_LARGE, RLE2_HUGE = 1536, 33808, 80512


def pairs(k, n, seed):
    """(1 2) k times, then run-free bytes in 100..249 up to n bytes: the sorted
    rotations that start with 1 and with 2 come first, each group preceded by
    one byte value, so the column starts with two zero runs of about k."""
    rng = np.random.default_rng(seed)
    m = n - 2 * k
    t = (100 + np.cumsum(rng.integers(1, 150, m, dtype=np.int64)) % 150).astype(np.uint8).tobytes()
    return bytes([1, 2]) * k + t


def _runs(d):
    vals, runs = mvals(d["syms"])
    return vals, runs


def _pairs_witness(k):
    def witness(raw, d):
        vals, runs = _runs(d)
        near = [(s, l) for s, l in runs if k - 3 <= l <= k]
        assert near, "no zero run of about %d values" % k
        return _facts(nmtf=len(d["syms"]), runs=near)
    return witness


def _final_run_witness(want):
    def witness(raw, d):
        vals, runs = _runs(d)
        assert runs and runs[-1][0] + runs[-1][1] == len(vals), "the final value is not zero"
        f = runs[-1][1]
        assert f == want if isinstance(want, int) else f > 4096
        return _facts(final_run=f, nvals=len(vals))
    return witness


def _final_run_row(want, n):
    """(3 255) m times: the largest rotations all follow a 3."""
    lo = want if isinstance(want, int) else 4100
    ok = _final_run_witness(want)

    def good(d):
        try:
            ok(None, d)
            return True
        except AssertionError:
            return False
    return _search(lambda t: pad(bytes([3, 255]) * (lo + t % 8), n, 300 + t // 8), good, "final run %s" % (want,))


@functools.lru_cache(maxsize=None)
def rle2_cases():
    """{row length: [(id, row, witness)]}."""
    small, large, huge = [], [], []
    for B in RLE2_SEAMS:
        for k in range(B - 4, B + 5):
            n = RLE2_SMALL if B == 64 else RLE2_LARGE
            (small if B == 64 else large).append(("pairs%d" % k, pairs(k, n, k), _pairs_witness(k)))
    huge.append(("pairs40000", pairs(40000, RLE2_HUGE, 40000), _pairs_witness(40000)))
    for want in (1, 2, 3, 63, 64, 65):
        small.append(("final%d" % want, _final_run_row(want, RLE2_SMALL), _final_run_witness(want)))
    large.append(("final-over-4096", _final_run_row("long", RLE2_LARGE), _final_run_witness("long")))

    def nonzero_end(raw, d):
        vals, runs = _runs(d)
        assert vals[-1] != 0
        return _facts(last_value=int(vals[-1]))
    small.append(("final-nonzero", _search(lambda t: pad(rand_bytes(700, 50 + t), RLE2_SMALL, t),
                                           lambda d: mvals(d["syms"])[0][-1] != 0, "nonzero final value"), nonzero_end))

    def hot(raw, d):
        vals, _ = _runs(d)
        nz = vals[vals != 0]
        share = float(((nz >= 1) & (nz <= 4)).mean())
        assert share > 0.9
        return _facts(share_1_to_4=round(share, 4))
    large.append(("values1to4", pad(rand_bytes(33000, 41, 4), RLE2_LARGE, 41), hot))
    return {RLE2_SMALL: small, RLE2_LARGE: large, RLE2_HUGE: huge}


@functools.lru_cache(maxsize=None)
def rle2_solo_cases():
    """No zero at all: only a short text can have it (own length)."""
    def no_zero(raw, d):
        vals, runs = _runs(d)
        assert not runs and len(vals) == len(raw)
        return _facts(nvals=len(vals))
    raw = _search(lambda t: bytes(np.random.default_rng(t).permutation(np.arange(40, 70, dtype=np.uint8))[:24]),
                  lambda d: not mvals(d["syms"])[1], "no zero value")
    return [("no-zero", raw, no_zero)]


# ------------------------------------------------------------------ D: MTF --
def _column(d):
    return bwt_column(mvals(d["syms"])[0], d["used"])


def _rank_order(t):
    t2 = t + t[:64]
    return sorted(range(len(t)), key=lambda i: t2[i:i + 64])


def _planted(n, seed, plants, ok, what):
    """A run-free text of n bytes in 5..244 with byte c written in front of the
    rotation of rank r + shift for every (r, c) of `plants`; the shifts are
    searched until the reference's column satisfies ok."""
    base = run_free(n, seed=seed)
    rot = _rank_order(base)

    def make(t):
        row = bytearray(base)
        for q, (r, c) in enumerate(plants):
            sh = (t // (5 ** q)) % 5 - 2
            row[(rot[r + sh] - 1) % n] = c
        return bytes(row)
    return _search(make, lambda d: ok(_column(d)), what, tries=min(TRIES, 5 ** len(plants)))


@functools.lru_cache(maxsize=None)
def mtf_cases():
    """[(id, raw, witness)], each of its own length."""
    S = MTF["SEG"]
    out = []
    for n in (S - 1, S, S + 1, 2 * S, 2 * S + 1):
        def length(raw, d, n=n):
            col = _column(d)
            assert len(col) == n == len(raw)
            return _facts(column=n)
        out.append(("text%d" % n, run_free(n, seed=n), length))

    # a symbol whose last occurrence before segment 2 is segment 1's last /
    # first position, and that segment 2 uses again
    def last_at(p):
        def ok(col):
            c = col[p]
            return c == 255 and c not in col[p + 1:2 * S] and c in col[2 * S:] and \
                (p == S or c not in col[S:p])
        return ok
    for name, p in (("seg-last", 2 * S - 1), ("seg-first", S)):
        def witness(raw, d, p=p):
            col = _column(d)
            assert last_at(p)(col)
            return _facts(symbol=int(col[p]), last_before_segment2=p, again=int(2 * S + np.flatnonzero(col[2 * S:] == col[p])[0]))
        raw = _planted(3 * S, 60 + p, [(p, 255), (2 * S + 900, 255)], last_at(p), name)
        out.append((name, raw, witness))

    # two symbols first seen in segment 2, the larger byte value first
    def fresh(col):
        new = sorted(set(col[2 * S:].tolist()) - set(col[:2 * S].tolist()))
        if len(new) < 2:
            return None
        first = [2 * S + int(np.flatnonzero(col[2 * S:] == c)[0]) for c in new]
        return new, first

    def fresh_witness(raw, d):
        got = fresh(_column(d))
        assert got and got[1][0] > got[1][-1], "never-seen symbols not met in descending order"
        return _facts(symbols=got[0], first_seen=got[1])
    raw = _planted(3 * S, 77, [(2 * S + 500, 254), (2 * S + 1500, 253)],
                   lambda col: bool(fresh(col)) and fresh(col)[1][0] > fresh(col)[1][-1], "symbols first seen in segment 2")
    out.append(("first-seen-seg2", raw, fresh_witness))

    # a symbol met in segment 0, not in segment 1, and again in segment 2 after
    # a symbol first seen there: mtf_prefix has to carry its position over a
    # segment without it, or it changes places with the never-seen one
    def skipped(col):
        a, b, c = col[:S], col[S:2 * S], col[2 * S:]
        return 255 in a and 255 not in b and 255 in c and 254 not in col[:2 * S] and 254 in c

    def skipped_witness(raw, d):
        col = _column(d)
        assert skipped(col)
        return _facts(symbol=255, seen=np.flatnonzero(col == 255).tolist(), fresh=np.flatnonzero(col == 254).tolist())
    out.append(("skips-segment1", _planted(3 * S, 91, [(300, 255), (2 * S + 700, 255), (2 * S + 1500, 254)], skipped,
                                           "a symbol absent from segment 1"), skipped_witness))

    # a run of equal column symbols that ends one position past an iteration / a segment
    for p in (MTF["ITER"], S):
        def ok(col, p=p):
            return len(col) > p + 1 and col[p - 1] == col[p] != col[p + 1]

        def witness(raw, d, p=p, ok=ok):
            col = _column(d)
            assert ok(col)
            return _facts(run_over=(p - 1, p), symbol=int(col[p]))
        raw = _search(lambda t, p=p: pairs(p - 6 + t, 2 * p + 700, p + t), lambda d, ok=ok: ok(_column(d)),
                      "column run over %d|%d" % (p - 1, p), tries=14)
        out.append(("colrun%d" % p, raw, witness))

    # a run of at least four equal column symbols that ends exactly on an
    # iteration's last position (255), its symbol not met again in segment 0,
    # while a smaller byte value is first seen in segment 1: if position 255 is
    # not taken as the run's end, the symbol counts as never seen and changes
    # places with the smaller one in segment 1's first list
    def run_end(col):
        p, S = MTF["ITER"] - 1, MTF["SEG"]
        c = col[p]
        return len(col) > S and (col[p - 3:p + 1] == c).all() and c not in col[p + 1:S] and \
            0 not in col[:S] and 0 in col[S:] and c > 0

    def run_end_witness(raw, d):
        col = _column(d)
        assert run_end(col)
        return _facts(run_ends_at=MTF["ITER"] - 1, symbol=int(col[MTF["ITER"] - 1]),
                      first_seen_in_segment1=int(MTF["SEG"] + np.flatnonzero(col[MTF["SEG"]:] == 0)[0]))

    def run_end_row(t):
        base = pairs(250 + t % 12, 6000, 3 + t // 12)
        rot = _rank_order(base)
        row = bytearray(base)
        row[rot[5000 + t // 12] - 1] = 0
        return bytes(row)
    out.append(("colrun-ends-255", _search(run_end_row, lambda d: run_end(_column(d)), "a column run ending on 255", tries=96),
                run_end_witness))

    def alpha(want):
        def witness(raw, d):
            assert d["alpha"] == want
            return _facts(alpha=d["alpha"], used=len(d["used"]))
        return witness
    rng = np.random.default_rng(256)
    out.append(("alpha258", bytes(rng.permutation(256).astype(np.uint8)) + rand_bytes(2400, 257), alpha(258)))
    out.append(("alpha5-one-value", b"\x07" * 1000, alpha(5)))
    out.append(("alpha4", b"aab", alpha(4)))
    out.append(("alpha3", b"q", alpha(3)))
    return out


# -------------------------------------------------------------- E: Huffman --
def _ngroups(nmtf):
    return 2 + sum(nmtf >= b for b in HUFF["BANDS"])


def _nmtf_case(name, want, alphabet=256, extra=None):
    """Random bytes with exactly `want` symbols (EOB included)."""
    def witness(raw, d):
        assert len(d["syms"]) == want and d["ngroups"] == _ngroups(want) and d["nsel"] == -(-want // HUFF["GROUP"])
        if extra:
            extra(d)
        return _facts(nmtf=want, ngroups=d["ngroups"], nsel=d["nsel"])
    guess = want - 1 if alphabet == 256 else want

    def make(t):
        n = guess + (t % 9) - 4 + (0 if alphabet == 256 else want // 3)
        return rand_bytes(n, 13 * want + t // 9, alphabet) if n > 0 else None
    raw = _search(make, lambda d: len(d["syms"]) == want, "nMTF %d" % want)
    return (name, raw, witness)


@functools.lru_cache(maxsize=None)
def huffman_cases():
    out = []
    for b in HUFF["BANDS"]:
        out.append(_nmtf_case("nmtf%d" % (b - 1), b - 1))
        out.append(_nmtf_case("nmtf%d" % b, b))
    G = HUFF["GROUP"]
    for q, r in ((7, 0), (7, 1), (7, 49)):
        out.append(_nmtf_case("nmtf50q+%d" % r, G * q + r))
    for nsel in (63, 64, 65, 255, 256, 257):
        out.append(_nmtf_case("nsel%d" % nsel, G * nsel - 7))

    from test_gpu import _bz2_cases
    geo = _bz2_cases()["geometric"].tobytes()

    # test_gpu's "geometric": a tree beyond 17 bits in an early pass of the
    # length computation (the weight-halving retry).  The stream cannot show
    # that: the reference's written tables reach 15 bits (levels 2 and 9), and a
    # Huffman tree of the last pass's frequencies, which the stream does give,
    # is exactly as deep.  No input built here (geometric and Fibonacci-weighted
    # columns up to 115 kB) made the reference write a 17-bit code, so the
    # witness is the depth the reference has.
    def deep(raw, d):
        longest = [max(ln) for ln in d["lengths"]]
        assert max(longest) == 15 and d["ngroups"] == 6
        return _facts(maxlen=longest, nmtf=len(d["syms"]))
    out.append(("geometric", geo, deep))

    def jump(d):
        return max(abs(a - b) for ln in d["lengths"] for a, b in zip(ln, ln[1:]))

    def delta(raw, d):
        assert jump(d) >= 10
        return _facts(max_delta=jump(d), alpha=d["alpha"])

    out.append(("length-delta10", _search(odd_values, lambda d: jump(d) >= 10, "a length table with a step of 10",
                                          tries=8), delta))
    return out


def odd_values(seed, words=12000):
    """A text whose column starts with a stretch of chosen symbols: words
    p 1 h l with increasing keys h l, so the rotations that start with 1 are
    sorted by word and their column is the p in text order.  The p are picked
    to have the move-to-front values 1, 3, 5 ... with halving frequency and no
    even value: in that stretch's table value 1 gets one bit and its neighbour
    value 2, never used, one of the longest codes."""
    rng = np.random.default_rng(seed)
    order = list(range(10, 36))
    out = bytearray()
    for i in range(words):
        v = 2 * min(int(rng.geometric(0.5)), 12) - 1
        p = order.pop(v)
        order.insert(0, p)
        out += bytes([p, 1, 60 + i // 190, 60 + i % 190])
    return bytes(out)


# ----------------------------------------------------- F: emit and compaction --
@functools.lru_cache(maxsize=None)
def emit_cases():
    out = []
    R = EMIT["ROUND"]
    for want in (R - 1, R, R + 1, 2 * R, 2 * R + 1):
        out.append(_nmtf_case("nmtf%d" % want, want))
    for r in (0, 1, 8, 9, 15):
        out.append(_nmtf_case("nmtf-round+%d" % r, R + 16 * 7 + r))
    for field in ("hdr_bits", "data_end"):
        for r in (0, 1, 31):
            def witness(raw, d, field=field, r=r):
                assert d[field] % 32 == r
                return _facts(**{field: d[field]})
            raw = _search(lambda t: rand_bytes(300 + t % 161, 5000 + t, 6), lambda d, field=field, r=r: d[field] % 32 == r,
                          "%s mod 32 == %d" % (field, r))
            out.append(("%s-mod32-%d" % (field, r), raw, witness))
    return out


@functools.lru_cache(maxsize=None)
def compaction_batch():
    """Eight one-byte rows whose reference streams (each under 44 bytes) put
    the payload offsets on every residue mod 4."""
    rows = [bytes([v]) for v in (0, 1, 65, 127, 128, 200, 254, 255)]
    return rows


def compaction_witness(streams):
    offs = np.concatenate(([0], np.cumsum([len(s) for s in streams])))[:-1]
    assert set((offs % 4).tolist()) == {0, 1, 2, 3} and min(len(s) for s in streams) < 44
    return _facts(offsets=offs.tolist())


# ------------------------------------------------------------- everything --
def all_cases(extra=0):
    """[(list, id, raw, witness)] of every case of lists A to F."""
    out = [("A",) + c for c in length_cases()]
    for g in rle1_cases(extra).values():
        out += [("B",) + c for c in g]
    out += [("B",) + c for c in rle1_solo_cases()]
    for g in rle2_cases().values():
        out += [("C",) + c for c in g]
    out += [("C",) + c for c in rle2_solo_cases()]
    out += [("D",) + c for c in mtf_cases()]
    out += [("E",) + c for c in huffman_cases()]
    out += [("F",) + c for c in emit_cases()]
    return out


# --------------------------------------------------------- the mixed batch --
MIXED_DIMS, MIXED_BS = [4 * 2048 + 16, 18 + 2, 2, 1, 1], [2048, 18, 1, 1, 1]


def place_blocks(dims, bs, streams):
    """The image (z, y, x) whose x-fastest block grid holds `streams` in order."""
    X, Y, Z = dims[:3]
    nb = [-(-d // b) for d, b in zip(dims[:3], bs[:3])]
    img = np.zeros((Z, Y, X), np.uint8)
    assert len(streams) == nb[0] * nb[1] * nb[2]
    for k, raw in enumerate(streams):
        i, j, z = k % nb[0], k // nb[0] % nb[1], k // (nb[0] * nb[1])
        w, h = min(bs[0], X - i * bs[0]), min(bs[1], Y - j * bs[1])
        assert bs[2] == 1 and len(raw) == w * h
        img[z, j * bs[1]:j * bs[1] + h, i * bs[0]:i * bs[0] + w] = np.frombuffer(raw, np.uint8).reshape(h, w)
    return img


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """[(id, raw)] in block order for MIXED_DIMS / MIXED_BS: blocks of 36 864,
    4 096, 288 and 32 bytes (border blocks), rows of every list side by side:
    2 to 6 coding tables, alphaSize 5 and 258, one to three RLE1 tiles."""
    big = {c[0]: c[1] for c in rle1_cases(0)[36864]}
    mid = {c[0]: c[1] for c in rle1_cases(0)[4096]}
    full = [("B:P32768-j3-R259", big["P32768-j3-R259"]), ("B:whole-tile", big["whole-tile"]),
            ("C:pairs16384", pairs(16384, 36864, 5)), ("A:rand36864", rand_bytes(36864, 36864)),
            ("B:P32768-j224-R256", big["P32768-j224-R256"]), ("C:values1to4", rand_bytes(36864, 6, 4)),
            ("D:pairs4096", pairs(4096, 36864, 7)), ("F:alpha6", rand_bytes(36864, 8, 6))]
    rng = np.random.default_rng(258)
    bottom = [("D:alpha5", b"\x07" * 4096), ("D:alpha258", bytes(rng.permutation(256).astype(np.uint8)) + rand_bytes(3840, 9)),
              ("E:groups3", pairs(1900, 4096, 10)), ("E:groups4", pairs(1650, 4096, 11)),
              ("E:groups5", pairs(1200, 4096, 12)), ("B:P2048-j255-R287", mid["P2048-j255-R287"]),
              ("B:last-R510", mid["last-R510"]), ("B:whole-chunk", mid["whole-chunk"])]
    right = [("E:rand288", rand_bytes(288, 13)), ("F:alpha6-288", rand_bytes(288, 14, 6))]
    corner = [("A:rand32", rand_bytes(32, 15)), ("A:alpha4-32", rand_bytes(32, 16, 4))]
    out = []
    for z in range(2):
        out += full[4 * z:4 * z + 4] + [right[z]] + bottom[4 * z:4 * z + 4] + [corner[z]]
    return out


def mixed_witness(dissected):
    """dissected: dissect(reference stream) per stream of mixed_batch()."""
    groups = sorted(set(d["ngroups"] for d in dissected))
    alphas = set(d["alpha"] for d in dissected)
    assert groups == [2, 3, 4, 5, 6] and {5, 258} <= alphas
    return _facts(ngroups=groups, alphas=sorted(alphas))
