"""Inputs for the exact check of predictor selection's bigram histograms
(csrc/lfm_entropy.hip: ent_next -> ent_link -> ent_rows), shared by
test_entropy_cases_cpu.py (the premises, without a GPU) and
test_entropy_hist_gpu.py (the kernels against the oracle, bin for bin).

A case is a named, seeded uint16 buffer and a candidate count: candidate k is
the view buffer[k : k + npix], so one-candidate cases are the buffer itself and
the job-mapping cases get candidates at byte offsets 2k of one allocation (the
layout lfm_hip_select produces for odd npix).  `claims` says what the case is
for, in terms test_entropy_cases_cpu.py verifies from the bytes alone.

The kernels' constants are restated in K (read back from the source by the
CPU test).  A chunk is at most K["kChunkPix"] pixels = 900 000 bytes: 54 full
segments of kSeg bytes plus one of 15 264, whose fourth wave holds 2 976 bytes
and ends in a half-full 64-lane window."""
import collections
import zlib

import numpy as np

K = {"kChunkPix": 450000, "kSub": 4096, "kSeg": 16384, "kSegMax": 55}
CHUNK_BYTES = 2 * K["kChunkPix"]
WINDOW = 64

Case = collections.namedtuple("Case", "name npix ncand build claims")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def candidates(case, buf=None):
    """The case's candidates as views of its buffer."""
    buf = case.build() if buf is None else buf
    assert buf.dtype == np.uint16 and buf.size == case.npix + case.ncand - 1
    return [buf[k:k + case.npix] for k in range(case.ncand)]


def chunks_of(cand):
    """The byte strings c[0..S) of a candidate's chunks."""
    b = np.ascontiguousarray(cand).view(np.uint8)
    return [b[o:o + CHUNK_BYTES] for o in range(0, b.size, CHUNK_BYTES)]


# --------------------------------------------------- sizes x distributions --
# the npix lists of test_entropy_single_candidate and test_entropy_partner_links
# (tests/test_gpu.py), two full chunks, and 3..6 pixels so that S % 16 takes
# every value a byte count of uint16 symbols can (0, 2, .. 14)
SIZES = sorted({1, 7, 449999, 450000, 450001, 1000003,
                1, 2, 8, 9, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 24577, 449999, 450000, 450007,
                900000, 3, 4, 5, 6})
DISTS = ("small", "bytes", "few", "runs")


def draw(dist, n, rng):
    """The four distributions of test_entropy_partner_links."""
    if dist == "small":
        return np.abs(rng.normal(0, 40, size=n)).astype(np.uint16)
    if dist == "bytes":
        return rng.integers(0, 65536, size=n, dtype=np.uint16)
    if dist == "few":
        return rng.choice(np.array([0x0100, 0x0302, 0x0001], np.uint16), size=n)
    assert dist == "runs"
    return np.repeat(rng.integers(0, 6, size=n // 50 + 1, dtype=np.uint16), 50)[:n]


def size_cases():
    out = []
    for dist in DISTS:
        for n in SIZES:
            name = "size-%s-%d" % (dist, n)
            out.append(Case(name, n, 1, lambda dist=dist, n=n, name=name: draw(dist, n, _rng(name)),
                            {"nchunks": -(-n // K["kChunkPix"])}))
    return out


# ----------------------------------------------------------- byte layouts --
def _chunk(name, fillers, places, S=CHUNK_BYTES):
    """S bytes drawn from `fillers`, then byte b at positions ps for every
    (b, ps) of `places`, as uint16 symbols (byte 2i is the low byte of symbol i)."""
    c = _rng(name).choice(np.array(fillers, np.uint8), S)
    for b, ps in places:
        assert b not in fillers
        c[np.asarray(ps, np.int64)] = b
    return c.view(np.uint16)


def _one_chunk(name, fillers, places, claims):
    places = [(b, [p % CHUNK_BYTES for p in ps]) for b, ps in places]  # (-1 is S - 1)
    claims = dict(claims, nchunks=1, positions={b: sorted(ps) for b, ps in places})
    return Case(name, K["kChunkPix"], 1, lambda: _chunk(name, fillers, places), claims)


def link_cases():
    seg = K["kSeg"]
    every = [s * seg + int(o) for s, o in enumerate(_rng("every-segment").integers(0, 15264, K["kSegMax"]))]
    return [
        # the next occurrence is 54 segments on: 53 empty tables between the two
        _one_chunk("link-twice-seg0-seg54", (0, 5, 9), [(0x77, [100, 54 * seg + 200])], {"segments": {0x77: [0, 54]}}),
        # every segment's last occurrence is closed by the next segment's first val (key 0 absent)
        _one_chunk("link-once-every-segment", (3, 8), [(0x77, every)], {"segments": {0x77: list(range(55))}}),
        # one link each across a window seam, a wave seam and a segment seam
        _one_chunk("link-window-wave-segment-seams", (0, 5, 9), [(0x77, [63, 64, 4095, 4096, 16383, 16384])],
                   {"segments": {0x77: [0, 1]}}),
        # a key whose one element is first and last at once, with val c[-1] = 0 ...
        _one_chunk("link-only-at-0", (0, 5, 9), [(0x07, [0])], {}),
        # ... and with the sentinel's val
        _one_chunk("link-only-at-end", (0, 5, 9), [(0x07, [-1])], {}),
    ]


def key_cases():
    seg, n = K["kSeg"], K["kChunkPix"]
    full = lambda name, f, claims: Case(name, n, 1, f, dict(claims, nchunks=1))  # noqa: E731
    return [
        full("key-only-0", lambda: np.zeros(n, np.uint16), {"keys": [0], "end_of_L": None,
                                                            "bins": {0x0000: CHUNK_BYTES}}),
        # c[-1] = 0 and the sentinel's key 0 put one bigram each in (255, 0) and (0, 255); every other
        # one lands in bin 0xFFFF, which is counted and never summed: H = 2 * -(1/S) ln(1/S)
        full("key-only-255", lambda: np.full(n, 0xFFFF, np.uint16),
             {"keys": [255], "end_of_L": CHUNK_BYTES - 1,
              "bins": {0xFFFF: CHUNK_BYTES - 2, 0xFF00: 1, 0x00FF: 1}}),
        # the sentinel is alone in key 0: its bigram is (c[S-1] << 8) | first val of the lowest key
        full("key-0-absent", lambda: _rng("key-0-absent").integers(1, 256, CHUNK_BYTES, dtype=np.uint8).view(np.uint16),
             {"absent": [0], "sentinel_alone": True}),
        full("key-only-0-and-255", lambda: _chunk("key-only-0-and-255", (0, 255), []), {"keys": [0, 255]}),
        full("key-all-256", lambda: _rng("key-all-256").integers(0, 256, CHUNK_BYTES, dtype=np.uint8).view(np.uint16),
             {"keys": list(range(256))}),
        # the end of L -- the one position without a bigram -- is the last occurrence of the highest key
        _one_chunk("end-of-L-at-0", (0, 5, 9), [(0xFE, [0])], {"end_of_L": 0}),
        _one_chunk("end-of-L-at-S-1", (0, 5, 9), [(0xFE, [1000, 500000, -1])], {"end_of_L": CHUNK_BYTES - 1}),
        _one_chunk("end-of-L-last-of-segment", (0, 5, 9), [(0xFE, [10, seg + 5, 3 * seg - 1])],
                   {"end_of_L": 3 * seg - 1}),
        _one_chunk("end-of-L-first-of-segment", (0, 5, 9), [(0xFE, [10, seg + 5, 3 * seg])], {"end_of_L": 3 * seg}),
    ]


def seam_cases():
    """Two and three chunks; the last byte of chunk q is 0xE0 + q, which occurs
    nowhere else in the buffer: a first val or a sentinel that crossed a chunk
    seam would fill a bin (0xE0 + q, .) or (., 0xE0 + q) of the wrong chunk."""
    out = []
    for tag, extra in (("two", 1031), ("three", 517)):
        name = "seam-%s-chunks" % tag
        nch = 2 if tag == "two" else 3
        npix = (nch - 1) * K["kChunkPix"] + extra
        ends = [min((q + 1) * CHUNK_BYTES, 2 * npix) - 1 for q in range(nch)]

        def build(name=name, npix=npix, ends=ends):
            return _chunk(name, (0, 5, 9, 0x21), [(0xE0 + q, [p]) for q, p in enumerate(ends)], S=2 * npix)
        out.append(Case(name, npix, 1, build, {"nchunks": nch, "seam_bytes": [0xE0 + q for q in range(nch)]}))
    return out


def hot_cases():
    """One constant symbol over two full chunks and one pixel: counts far above
    16 bits in one bin, bin 0 (held in registers) and bin 0xFFFF among them.
    `bins` is the whole histogram of the first chunk."""
    S = CHUNK_BYTES
    want = {0x0000: {0x0000: S},
            0x0101: {0x0101: S - 2, 0x0100: 1, 0x0001: 1},
            0xFFFF: {0xFFFF: S - 2, 0xFF00: 1, 0x00FF: 1},
            # keys 0 at the odd positions (val 0xFF), then the sentinel (val 0), then keys 0xFF (val 0)
            0x00FF: {0xFFFF: S // 2 - 1, 0xFF00: 1, 0x0000: S // 2}}
    return [Case("hot-%04x" % v, 900001, 1, lambda v=v: np.full(900001, v, np.uint16), {"nchunks": 3, "bins": bins})
            for v, bins in want.items()]


# (ncand, nchunks): job counts 7, 9, 10, 16 and 24 for ent_rows' job-to-block mapping
JOB_SHAPES = ((7, 1), (3, 3), (5, 2), (8, 2), (8, 3))
JOB_NPIX = {1: 30001, 2: 451237, 3: 900733}  # odd: the chunk tails differ per candidate


def job_cases():
    out = []
    for ncand, nch in JOB_SHAPES:
        name = "jobs-%dx%d" % (ncand, nch)
        npix = JOB_NPIX[nch]
        out.append(Case(name, npix, ncand, lambda name=name, n=npix + ncand - 1: draw("small", n, _rng(name)),
                        {"nchunks": nch, "distinct": True}))
    return out


# ------------------------------------------------------------------- ties --
TIE_W, TIE_H, TIE_T = 52, 39, 13


def tie_frames():
    """(name, frame, family, candidates that tie for the minimum, chosen):
    frames on which lfmo_select's candidates tie exactly, so the rule that ties
    go to the highest index decides."""
    y, x = np.mgrid[0:TIE_H, 0:TIE_W]
    const = np.full((TIE_H, TIE_W), 1000, np.uint16)
    lenslets = ((y // TIE_T) * 7 + (x // TIE_T) * 3 + 100).astype(np.uint16)
    return [("const-tiles", const, "tiles", [1, 2, 3, 4, 6, 7], 7),
            ("const-angle", const, "angle", [1, 2, 3, 4, 5, 6, 7], 7),
            ("const-space", const, "space", [1, 2, 3, 4, 5, 6, 7], 7),
            ("rows-angle", (y * 5 + 100).astype(np.uint16), "angle", [1, 4], 4),
            ("lenslets-angle", lenslets, "angle", [4, 7], 7),
            ("columns-space", (x * 5 + 100).astype(np.uint16), "space", [2, 4], 4)]


def all_cases():
    return size_cases() + link_cases() + key_cases() + seam_cases() + hot_cases() + job_cases()
