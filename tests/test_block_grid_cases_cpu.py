"""The premises of tests/block_grid_cases.py, checked without a GPU: which
launcher path a case takes, that its hot FDiv divisor really needs the
correction step under IEEE float32 at an offset the kernel forms (and that the
cold cases never do), the block sizes against the bzip2 block limit, the
geometry claims by plain arithmetic on oracle.iter_blocks, and the recorded
search for FDiv's `q -= 1` branch."""
import os
import re

import numpy as np
import pytest

import block_grid_cases as G
import bz2_parts
from conftest import PKG

CASES = G.CASES
IDS = [c.name for c in CASES]
BASE = 0x7F0000001000  # a 256-byte aligned address, as the GPU test places the image


def sizes(case):
    return [size for _, _, size in G.boxes(case)]


def test_table_is_the_issue_s():
    assert IDS == ["img-5d", "img-5d-u8", "img-5d-f32", "img-5d-b8", "fdiv-row", "fdiv-y", "fdiv-z", "fdiv-c",
                   "fdiv-all", "gather-dims", "gather-bs", "gather-base", "gather-loops", "gather-short",
                   "multi-img", "multi-gather", "huge", "img-5d-sub", "gather-dims-sub"]
    for c in CASES:
        first, count = c.span
        assert 0 <= first and count >= 1 and first + count <= c.total == len(G.boxes(c)), c.name
    assert [c.span for c in CASES if c.name.endswith("-sub")] == [(37, 29), (37, 29)]
    assert G.BY_NAME["img-5d-sub"].span != (0, G.BY_NAME["img-5d-sub"].total)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_launcher_predicates(case):
    """from_img / v16 as claimed; a gather case fails exactly the clause it names."""
    ptr = BASE + case.base_off
    assert G.from_img(case, ptr) == case.from_img
    failed = G.from_img_clauses(case, ptr)
    assert failed == ([] if case.from_img else [case.why_not])
    assert case.block_bytes % 16 == 0 or not case.v16
    assert G.v16(case, BASE, ptr, case.block_bytes) == case.v16
    if case.v16:  # what the three extra scatter cases of the GPU test do, each alone
        assert not G.v16(case, BASE + 8, ptr, case.block_bytes)
        assert not G.v16(case, BASE, ptr + 2, case.block_bytes)
        assert not G.v16(case, BASE, ptr, case.block_bytes + 8)


def test_predicates_and_strides_read_back_from_the_sources():
    """The two predicates, FDiv's limit and the loop strides the cases sit on
    both sides of, as the sources state them: a change there moves the cases
    or fails here."""
    enc = open(os.path.join(PKG, "csrc", "lfm_bzip2.hip")).read()
    dec = open(os.path.join(PKG, "csrc", "lfm_bunzip2.hip")).read()
    ws = lambda s: re.sub(r"\s+", "", s)  # noqa: E731
    m = re.search(r"const bool from_img =(.*?);", enc, re.S)
    assert m and sorted(ws(m.group(1)).split("&&")) == sorted([
        "((uintptr_t)d_img&15)==0", "(bs[0]*bpp)%16==0", "(dims[0]*bpp)%16==0", "((dims[0]%bs[0])*bpp)%16==0"])
    assert re.search(r"if \(!from_img\) hipLaunchKernelGGL\(gather_blocks, dim3\(%d, streams\), dim3\(%d\)"
                     % (G.GATHER_ROW_GROUPS, G.GATHER_ROW_THREADS), enc)
    m = re.search(r"bool v16 =(.*?);\s*if \(v16 && dims\[0\] % bs\[0\]\) v16 =(.*?);", dec, re.S)
    assert m and sorted(ws(m.group(1)).split("&&")) == sorted([
        "((uintptr_t)d_blocks&15)==0", "((uintptr_t)d_img&15)==0", "stride%16==0", "((size_t)dims[0]*bpp)%16==0",
        "((size_t)bs[0]*bpp)%16==0"])
    assert ws(m.group(2)) == "((size_t)(dims[0]%bs[0])*bpp)%16==0"
    assert re.search(r"scatter_blocks16, dim3\(8, count\), dim3\(256\)", dec) and G.SCATTER16_UNITS == 8 * 256
    assert re.search(r"scatter_blocks, dim3\(%d, count\), dim3\(%d\)" % (G.GATHER_ROW_GROUPS, G.GATHER_ROW_THREADS), dec)
    assert re.search(r"if \(x >= \(1u << 23\)\) return x / d;", enc) and G.FDIV_LIMIT == 1 << 23
    threads = int(re.search(r"constexpr \w+ kRleThreads = (\d+);", enc).group(1))
    chunk = int(re.search(r"constexpr \w+ kRleChunk = (\d+);", enc).group(1))
    assert re.search(r"kRleTile = kRleThreads \* kRleChunk;", enc) and threads * chunk == G.RLE_TILE
    assert re.search(r"glim = FROM_IMG \? L - 16 :", enc)  # fdiv_dividends: no offset past L - 16


def test_fourth_clause_is_implied():
    """((dims[0] % bs[0]) * bpp) % 16 == 0 whenever the bs and dims clauses
    hold: no geometry isolates it."""
    for bpp in (1, 2, 4, 8):
        for b0 in range(1, 130):
            for d0 in range(b0, 400):
                if (b0 * bpp) % 16 == 0 and (d0 * bpp) % 16 == 0:
                    assert ((d0 % b0) * bpp) % 16 == 0


@pytest.mark.parametrize("case", [c for c in CASES if c.hot], ids=[c.name for c in CASES if c.hot])
def test_hot_divisors_need_the_plus_one(case):
    """Each claimed divisor, at a dividend load16 forms for the named block:
    the raw float32 quotient is one too small, and first so at x == d."""
    assert case.from_img
    boxes = G.boxes(case)
    for label, d, bid in case.hot:
        size = boxes[bid][2]
        dd, xs = G.fdiv_dividends(size, case.bpp)[label]
        assert dd == d, (label, dd)
        xs = xs[xs < G.FDIV_LIMIT]
        raw = G.fdiv_raw(xs, d)
        wrong = xs[raw != xs // d]
        assert wrong.size, (label, d)
        assert int(wrong[0]) == d and int(G.fdiv_raw(d, d)) == 0
        assert np.array_equal(raw[raw != xs // d] + 1, wrong // d)  # +1 mends every one of them
    if len(case.hot) == 1:  # the single-divisor cases: the other three divisions are exact
        label = case.hot[0][0]
        for size in sizes(case):
            assert [k for k, v in G.fdiv_corrections(size, case.bpp).items() if v is not None and k != label] == []


@pytest.mark.parametrize("case", [c for c in CASES if c.cold], ids=[c.name for c in CASES if c.cold])
def test_cold_cases_never_correct(case):
    assert case.from_img and not case.hot
    for size in sizes(case):
        assert set(G.fdiv_corrections(size, case.bpp).values()) == {None}, size


def test_hot_and_cold_partition_the_single_block_image_cases():
    for c in CASES:
        if c.from_img and not c.multi:
            assert bool(c.hot) != c.cold, c.name
        if not c.from_img:
            assert not c.hot and not c.cold, c.name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_lengths_against_the_bzip2_block_limit(case):
    limit = bz2_parts.nblock_max(case.level)
    L = max(int(np.prod(s)) * case.bpp for s in sizes(case))
    assert L == case.block_bytes  # (the first block is a full one)
    if case.multi:
        assert L > limit
    else:
        assert L + L // 4 < limit  # RLE1 grows a text by at most 5/4
    if case.name == "huge":
        assert L >= G.FDIV_LIMIT and case.claims["over_fdiv_limit"]
    else:
        assert L < G.FDIV_LIMIT
    if case.from_img:  # rle1_crc clamps its loads to L - 16
        assert min(int(np.prod(s)) * case.bpp for s in sizes(case)) >= 16


def _cmp(op, a, b):
    return a > b if op == ">" else a < b


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_geometry_claims(case):
    """Every entry of case.claims by arithmetic on oracle.iter_blocks."""
    boxes, sz, bpp = G.boxes(case), sizes(case), case.bpp
    rows = [int(np.prod(s[1:])) for s in sz]
    rowb = [s[0] * bpp for s in sz]
    for key, val in case.claims.items():
        if key == "streams":
            assert len(boxes) == val
        elif key == "ragged_all":
            assert all(d % b for d, b in zip(case.dims, case.bs))
            assert sz[-1] == [d % b for d, b in zip(case.dims, case.bs)]
        elif key == "deep":
            assert sz[0][3] > 1 and sz[0][4] > 1
        elif key == "units_per_block":
            assert _cmp(val[0], rows[0] * rowb[0] // 16, val[1])
        elif key == "max_block_bytes":
            assert max(r * b for r, b in zip(rows, rowb)) == val == case.block_bytes
        elif key == "rle_tiles":
            assert -(-case.block_bytes // G.RLE_TILE) == val and val > 2
        elif key == "image_row_bytes":
            assert case.dims[0] * bpp == val
        elif key == "block_row_bytes":
            assert rowb[0] == val
        elif key == "rows_per_block":
            assert all(_cmp(val[0], r, val[1]) for r in rows) and max(rows) == val[2]
        elif key == "row_bytes":
            assert all(_cmp(val[0], b, val[1]) for b in rowb)
        elif key == "short_block":
            bid, r, b = val
            assert (rows[bid], rowb[bid]) == (r, b) and rows[bid] == min(rows) and rowb[bid] == min(rowb)
        elif key == "parts_of_block0":
            assert len(bz2_parts.parts(G.expected_blocks(case)[0], case.level)) == val
        elif key == "over_fdiv_limit":
            assert rows[0] * rowb[0] >= G.FDIV_LIMIT
        else:
            raise AssertionError("unchecked claim %r" % key)
    if case.name == "fdiv-all":  # rows of 752 and of 656 bytes
        assert set(rowb) == {752, 656}
    if case.name == "huge":  # the thin second stream: the narrowest an image-direct block can be
        assert rowb[1] == 16 and rows[1] == rows[0]


@pytest.mark.parametrize("case", [c for c in CASES if c.name != "huge"], ids=[c.name for c in CASES if c.name != "huge"])
def test_images_and_addresses(case):
    """make_image: the case's dtype and shape, bytes 0 .. 199, the same on every
    call, no stream a repetition of a shorter text; byte_address names the
    image byte a block byte came from."""
    img = G.make_image(case)
    assert img.dtype == case.dtype and list(img.shape) == list(case.dims[::-1])
    raw = img.view(np.uint8)
    assert raw.max() == 199 and np.array_equal(raw, G.make_image(case).view(np.uint8))
    blocks = G.expected_blocks(case, img)
    assert [len(b) for b in blocks] == [int(np.prod(s)) * case.bpp for s in sizes(case)]
    rng = np.random.default_rng(5)
    rows = raw.reshape(tuple(case.dims[:0:-1]) + (case.dims[0] * case.bpp,))
    for bid in {0, 1, case.total // 2, case.total - 1}:
        b = np.frombuffer(blocks[bid], dtype=np.uint8)
        for p in range(1, 64):  # not periodic with a short period
            assert not np.array_equal(b[p:], b[:-p]) or b.size <= p
        for k in [0, b.size - 1] + [int(v) for v in rng.integers(0, b.size, 8)]:
            a = G.byte_address(case, bid, k)
            x0 = G.boxes(case)[bid][1][0]
            assert rows[a["t"], a["c"], a["z"], a["y"], x0 * case.bpp + a["col"]] == b[k]
    scattered = G.scattered_image(case, img, 0xFF)
    first, count = case.span
    if count == case.total:
        assert np.array_equal(scattered, rows)
    else:  # 0xFF is no image byte: exactly the span's bytes are the image's
        assert int((scattered == rows).sum()) == sum(len(b) for b in blocks[first:first + count]) < rows.size
    other = bytearray(blocks[1])
    other[len(other) - 1] ^= 1
    d = G.first_difference(case, 1, bytes(other), blocks[1])
    assert d["byte"] == len(other) - 1 and d["block"] == 1 and G.first_difference(case, 1, blocks[1], blocks[1]) is None


def test_minus_one_branch_search():
    """FDiv's `q -= 1` branch, searched for below 2^23 where the float path
    runs: every multiple of 16 up to 65 536 as a row size and every d up to 4096
    as a row-index divisor, at the dividends just below and at each multiple
    of d.  RECORDED OUTCOME: the raw quotient is never above x // d (the branch
    is unreachable, so block_grid_cases has no case for it), and never more
    than one below it (one correction step is enough)."""
    ds = sorted(set(range(1, 4097)) | set(range(16, 65537, 16)))
    too_big, below, plus_one = [], 0, 0
    for d in ds:
        k = np.arange(1, (G.FDIV_LIMIT - 1) // d + 1, dtype=np.int64)
        for xs in (k * d - 1, k * d):
            xs = xs[xs < G.FDIV_LIMIT]
            diff = G.fdiv_raw(xs, d) - xs // d
            if (diff > 0).any():
                too_big.append((d, int(xs[diff > 0][0])))
            below = min(below, int(diff.min()))
            plus_one += int((diff < 0).sum())
    assert too_big == []
    assert below == -1 and plus_one > 0


def test_plus_one_divisors_the_issue_lists():
    """The row sizes and row-index divisors the case table draws on: of the
    multiples of 16 up to 4096, 38 row sizes need the +1 for some 16-byte
    offset below 900 000; of the divisors below 130, fifteen do."""
    xs = np.arange(0, 900000, 16, dtype=np.int64)
    hot = [d for d in range(16, 4097, 16) if (G.fdiv_raw(xs, d) != xs // d).any()]
    assert len(hot) == 38 and hot[:6] == [656, 752, 880, 976, 1312, 1328]
    xs = np.arange(0, 900000 // 16, dtype=np.int64)
    assert [d for d in range(1, 130) if (G.fdiv_raw(xs, d) != xs // d).any()] == \
        [41, 47, 55, 61, 82, 83, 94, 97, 107, 109, 110, 115, 121, 122, 123]
    for d in (192, 128, 48, 32, 4096):  # the row sizes of the rest of the suite: never
        assert not (G.fdiv_raw(np.arange(0, 900000, 16), d) != np.arange(0, 900000, 16) // d).any()


def test_scatter_wrapper_refuses_bad_ranges(lfmlib):
    """scatter_blocks_device checks the block range, the stride and the extents
    before anything is launched (the C entry does not)."""
    dims, bs = [88, 10, 5, 3, 3], [40, 4, 2, 2, 2]
    good = dict(stride=2560, first=0, count=108)
    for bad in (dict(first=108, count=1), dict(first=80, count=29), dict(count=0), dict(first=-1),
                dict(stride=2559), dict(stride=1 << 32)):
        kw = dict(good, **bad)
        with pytest.raises(ValueError):
            lfmlib.scatter_blocks_device(4096, kw["stride"], kw["first"], kw["count"], dims, bs, 2, 8192)
    for d, b, bpp in ((dims[:4], bs, 2), (dims, [40, 4, 2, 2, 0], 2), (dims, bs, 0)):
        with pytest.raises(ValueError):
            lfmlib.scatter_blocks_device(4096, 2560, 0, 1, d, b, bpp, 8192)
    assert "lfm_hip_scatter_blocks" in lfmlib.EXPORTS
