"""Block-grid geometries for the code that maps a 5-D image to bzip2 streams and
back: gather_blocks and rle1_crc<FROM_IMG> (lfm_bzip2.hip), scatter_blocks and
scatter_blocks16 (lfm_bunzip2.hip).  Shared by test_block_grid_cases_cpu.py
(which checks every claim a case makes, without a GPU) and
test_block_grid_gpu.py.  TEST INFRASTRUCTURE ONLY: no GPU, no torch.

All three kernels compute block id -> origin / size -> row address on their
own; rle1_crc<FROM_IMG> divides with a float reciprocal and one correction step
(FDiv).  A case names the path it takes and the property it is in the table
for; `claims` is what the CPU test verifies by arithmetic.

dims and bs are [x, y, z, c, t]; images are indexed [t, c, z, y, x].

The two launcher predicates have a fourth clause,
((dims[0] % bs[0]) * bpp) % 16 == 0 (the ragged last block's rows).  It follows
from the two before it: dims[0] % bs[0] = dims[0] - k * bs[0], so its bytes are
dims[0] * bpp - k * bs[0] * bpp, a difference of two multiples of 16.  No case
can make it the one clause that fails; the kernels keep it all the same.

FDiv's `q -= 1` branch is unreachable below 2^23 (where FDiv switches to the
integer division): the raw quotient fl(fl(x) * fl(1 / d)) exceeds x // d only
when the two roundings, each at most 2^-24 relative, add more than the 1 / d
that x = k * d - 1 lies below k, i.e. when k * 2^-23 > 1 / d, x >= 2^23.
test_block_grid_cases_cpu.py::test_minus_one_branch_search runs the search and
asserts that it finds nothing, so the table has no case for that branch.

lfm_hip_bzip2_blocks checks only bpp != 0, so the table has a bpp 8 case.
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

import lfm_oracle as O

NP_OF_BPP = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.float64}
FDIV_LIMIT = 1 << 23   # FDiv::div: integer division from here on
RLE_TILE = 16384       # kRleTile: bytes of a block one rle1_crc round reads
GATHER_ROW_GROUPS = 64    # gather_blocks / scatter_blocks: row workgroups per stream
GATHER_ROW_THREADS = 256  # ... and threads (bytes per pass) of one row
SCATTER16_UNITS = 8 * 256  # scatter_blocks16: 16-byte units one pass of a stream moves


@dataclass(frozen=True)
class Case:
    name: str
    dims: tuple
    bs: tuple
    bpp: int = 2
    level: int = 1
    multi: bool = False
    base_off: int = 0      # the image starts this many bytes past a 256-byte aligned address
    first: int = 0
    count: int = None      # None: every block from `first` on
    from_img: bool = True  # claimed: rle1_crc reads the image itself (else gather_blocks runs first)
    why_not: str = None    # the one clause of the predicate a gather case fails: "base", "bs" or "dims"
    hot: tuple = ()        # claimed: ((divisor label, d, block id), ...) whose FDiv needs the +1
    cold: bool = False     # claimed: no division of any block needs a correction
    claims: dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def dtype(self):
        return np.dtype(NP_OF_BPP[self.bpp])

    @property
    def nb(self):
        return [-(-d // b) for d, b in zip(self.dims, self.bs)]

    @property
    def total(self):
        return int(np.prod(self.nb))

    @property
    def span(self):
        """(first, count) of the streams a test compresses or scatters."""
        return self.first, self.total - self.first if self.count is None else self.count

    @property
    def block_bytes(self):
        return int(np.prod(self.bs)) * self.bpp

    @property
    def image_bytes(self):
        return int(np.prod(self.dims)) * self.bpp

    @property
    def v16(self):
        """Claimed: lfm_hip_scatter_blocks takes scatter_blocks16, given a
        16-byte aligned block buffer at stride block_bytes."""
        return self.from_img


def _case(name, dims, bs, **kw):
    return Case(name, tuple(dims), tuple(bs), **kw)


IMG5 = dict(dims=[88, 10, 5, 3, 3], bs=[40, 4, 2, 2, 2])
_DEEP = dict(streams=108, ragged_all=True, deep=True)

CASES = [
    # ---- image-direct path: ragged in every dimension, sz[3] and sz[4] > 1
    _case("img-5d", **IMG5, cold=True, claims=dict(_DEEP, units_per_block=("<", SCATTER16_UNITS))),
    _case("img-5d-u8", [112, 10, 5, 3, 3], [48, 4, 2, 2, 2], bpp=1, cold=True, claims=_DEEP),
    _case("img-5d-f32", [28, 10, 5, 3, 3], [12, 4, 2, 2, 2], bpp=4, cold=True, claims=_DEEP),
    _case("img-5d-b8", [14, 10, 5, 3, 3], [6, 4, 2, 2, 2], bpp=8, cold=True, claims=_DEEP),
    # ---- FDiv: one named divisor needs the +1 at an offset block 0 reads
    _case("fdiv-row", [664, 7, 1, 1, 1], [328, 3, 1, 1, 1], hot=(("row", 656, 0),)),
    _case("fdiv-y", [24, 87, 5, 1, 1], [8, 41, 2, 1, 1], hot=(("y", 41, 0),)),
    _case("fdiv-z", [16, 3, 50, 3, 1], [8, 1, 47, 2, 1], hot=(("z", 47, 0),)),
    _case("fdiv-c", [16, 2, 2, 59, 3], [8, 1, 1, 55, 2], hot=(("c", 55, 0),)),
    # 369 984 B * 5/4 needs level 5 to stay one bzip2 block
    _case("fdiv-all", [704, 47, 3, 4, 3], [376, 41, 2, 3, 2], level=5,
          hot=(("row", 752, 0), ("y", 41, 0), ("row", 656, 1)),
          claims=dict(max_block_bytes=369984, rle_tiles=23, units_per_block=(">", SCATTER16_UNITS))),
    # ---- gather path: not from_img, for one reason each
    _case("gather-dims", [90, 10, 5, 3, 3], IMG5["bs"], from_img=False, why_not="dims",
          claims=dict(_DEEP, image_row_bytes=180)),
    _case("gather-bs", IMG5["dims"], [36, 4, 2, 2, 2], from_img=False, why_not="bs",
          claims=dict(deep=True, block_row_bytes=72)),
    _case("gather-base", **IMG5, base_off=2, from_img=False, why_not="base", claims=_DEEP),
    # (two blocks side by side in x rather than in t: with dims[0] == bs[0] == 1000
    # both the "bs" and the "dims" clause would fail)
    _case("gather-loops", [2000, 9, 10, 1, 1], [1000, 9, 10, 1, 1], bpp=1, level=2, from_img=False, why_not="bs",
          claims=dict(block_row_bytes=1000, rows_per_block=(">", GATHER_ROW_GROUPS, 90),
                      row_bytes=(">", GATHER_ROW_THREADS))),
    # the geometry of gather-dims with other data: block 107, the last, is ragged
    # in every dimension and has 2 rows of 20 bytes; no block has more than 32 rows of 80
    _case("gather-short", [90, 10, 5, 3, 3], IMG5["bs"], from_img=False, why_not="dims",
          claims=dict(short_block=(107, 2, 20), rows_per_block=("<", GATHER_ROW_GROUPS, 32),
                      row_bytes=("<", GATHER_ROW_THREADS))),
    # ---- streams of several bzip2 blocks (lfm_hip_bzip2_blocks_multi)
    _case("multi-img", [664, 50, 2, 3, 1], [328, 41, 2, 2, 1], multi=True,
          claims=dict(max_block_bytes=107584, parts_of_block0=2)),
    _case("multi-gather", [666, 50, 2, 3, 1], [328, 41, 2, 2, 1], multi=True, from_img=False, why_not="dims",
          claims=dict(max_block_bytes=107584, parts_of_block0=2)),
    # the first block reaches FDiv's integer division; the second stream is as thin
    # as a 16-byte row allows
    _case("huge", [672, 41, 47, 7, 1], [656, 41, 47, 7, 1], bpp=1, level=9, multi=True,
          hot=(("row", 656, 0), ("y", 41, 0), ("z", 47, 0)),
          claims=dict(max_block_bytes=8848784, streams=2, over_fdiv_limit=True)),
    # ---- sub-ranges of the grid
    _case("img-5d-sub", **IMG5, first=37, count=29, cold=True, claims=_DEEP),
    _case("gather-dims-sub", [90, 10, 5, 3, 3], IMG5["bs"], first=37, count=29, from_img=False, why_not="dims",
          claims=_DEEP),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------ data --
def make_image(case):
    """The case's image [t, c, z, y, x] in its dtype: random bytes 0 .. 199 from
    a seed that is the case's name (no period, runs of four are rare, 56 byte
    values never occur)."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    raw = rng.integers(0, 200, case.image_bytes, dtype=np.uint8)
    return raw.view(case.dtype).reshape(tuple(case.dims[::-1]))


def boxes(case):
    """[(block id, origin, size)] of every block, origin and size [x, y, z, c, t]."""
    return list(O.iter_blocks(list(case.dims), list(case.bs)))


def expected_blocks(case, img=None):
    """The bytes of every block of the grid (not only the case's span), x
    fastest, then y, z, c, t."""
    img = make_image(case) if img is None else img
    return [O.gather_block(img, coord, size) for _, coord, size in boxes(case)]


def scattered_image(case, img=None, fill=0xA5):
    """The image's bytes, as rows [t, c, z, y, x * bpp], after the blocks of the
    case's span were scattered into an image of `fill` bytes."""
    img = make_image(case) if img is None else img
    rows = img.view(np.uint8).reshape(tuple(case.dims[:0:-1]) + (case.dims[0] * case.bpp,))
    out = np.full_like(rows, fill)
    first, count = case.span
    for _, (x0, y0, z0, c0, t0), (sx, sy, sz, sc, st) in boxes(case)[first:first + count]:
        box = (slice(t0, t0 + st), slice(c0, c0 + sc), slice(z0, z0 + sz), slice(y0, y0 + sy),
               slice(x0 * case.bpp, (x0 + sx) * case.bpp))
        out[box] = rows[box]
    return out


def byte_address(case, bid, k):
    """Where byte k of block bid lies: its row and column (bytes) in the block
    and the image coordinates of that row."""
    _, coord, size = boxes(case)[bid]
    rowb = size[0] * case.bpp
    row, col = divmod(k, rowb)
    q, y = divmod(row, size[1])
    q, z = divmod(q, size[2])
    t, c = divmod(q, size[3])
    return dict(block=bid, row=row, col=col, t=coord[4] + t, c=coord[3] + c, z=coord[2] + z, y=coord[1] + y,
                x=coord[0] + col // case.bpp)


def first_difference(case, bid, got, want):
    """byte_address of the first byte in which two versions of block bid
    differ (a length difference counts from the shorter one's end), with both
    bytes; None when they are equal."""
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    n = min(a.size, b.size)
    ne = np.flatnonzero(a[:n] != b[:n])
    if ne.size == 0 and a.size == b.size:
        return None
    k = int(ne[0]) if ne.size else n
    where = byte_address(case, bid, min(k, max(b.size - 1, 0)))
    where.update(byte=k, got=int(a[k]) if k < a.size else None, want=int(b[k]) if k < b.size else None,
                 got_len=int(a.size), want_len=int(b.size))
    return where


# ------------------------------------------------------------ predicates --
def from_img_clauses(case, ptr):
    """The independent clauses of the from_img test (lfm_bzip2.hip, bzip2_blocks)
    that fail for an image at address ptr."""
    d0, b0, bpp = case.dims[0], case.bs[0], case.bpp
    failed = []
    if ptr % 16:
        failed.append("base")
    if (b0 * bpp) % 16:
        failed.append("bs")
    if (d0 * bpp) % 16:
        failed.append("dims")
    return failed


def from_img(case, ptr):
    """bzip2_blocks' from_img for an image at address ptr."""
    d0, b0, bpp = case.dims[0], case.bs[0], case.bpp
    return (ptr % 16 == 0 and (b0 * bpp) % 16 == 0 and (d0 * bpp) % 16 == 0
            and ((d0 % b0) * bpp) % 16 == 0)


def v16(case, blocks_ptr, img_ptr, stride):
    """lfm_hip_scatter_blocks' v16 (lfm_bunzip2.hip)."""
    d0, b0, bpp = case.dims[0], case.bs[0], case.bpp
    ok = (blocks_ptr % 16 == 0 and img_ptr % 16 == 0 and stride % 16 == 0
          and (d0 * bpp) % 16 == 0 and (b0 * bpp) % 16 == 0)
    if ok and d0 % b0:
        ok = ((d0 % b0) * bpp) % 16 == 0
    return ok


# ------------------------------------------------------------------ FDiv --
def fdiv_raw(x, d):
    """FDiv::div's quotient before its correction step, in IEEE float32:
    (uint32)((float)x * (1.0f / (float)d)); x a scalar or an array below 2^23."""
    inv = np.float32(1.0) / np.float32(d)
    return (np.asarray(x).astype(np.float32) * inv).astype(np.int64)


def fdiv_dividends(size, bpp):
    """{label: (d, dividends)} of the four divisions rle1_crc<FROM_IMG>'s load16
    makes for a block of `size`: the 16-byte offsets g of [0, L) by the row
    bytes, then the row index by sz[1], that quotient by sz[2], and that one by
    sz[3].  (Every load is clamped to L - 16, the prefetch past the block's
    end included, so these are all the offsets there are.)"""
    rowb = size[0] * bpp
    g = np.arange(0, rowb * int(np.prod(size[1:])), 16, dtype=np.int64)
    row = np.unique(g // rowb)
    qy = np.unique(row // size[1])
    qz = np.unique(qy // size[2])
    return {"row": (rowb, g), "y": (size[1], row), "z": (size[2], qy), "c": (size[3], qz)}


def fdiv_corrections(size, bpp):
    """{label: first dividend below 2^23 whose raw quotient is not x // d, or
    None} for a block of `size`."""
    out = {}
    for label, (d, xs) in fdiv_dividends(size, bpp).items():
        xs = xs[xs < FDIV_LIMIT]
        bad = np.flatnonzero(fdiv_raw(xs, d) != xs // d)
        out[label] = int(xs[bad[0]]) if bad.size else None
    return out
