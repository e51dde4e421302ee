"""The GPU bzip2 encoder outside the BWT (rle1_crc, gather_blocks, mtf_last /
mtf_prefix / mtf_win, rle2, huff_init / huff_select_reg / huff_lengths_heap /
huff_final, emit_stream, place_parts / join_parts, scan_offsets /
compact_streams) against the reference bzip2, byte for byte, on inputs aimed
at the seams of those kernels: the case lists of tests/bz2_encode_cases.py,
whose premises tests/test_bz2_encode_seams_cpu.py proves against the
reference library's own streams.  Every row must come back with flags == 0
(none is periodic or reaches nblockMAX): a row handed to the host library
would hide a wrong kernel."""
import numpy as np
import pytest

import bz2_encode_cases as C
from test_bwt_induce_compact_gpu import encode, ref_bz2

pytestmark = pytest.mark.gpu

BATCH = 64
_expected = {}


def expected(oracle, raw, level):
    key = (raw, level)
    if key not in _expected:
        _expected[key] = ref_bz2(oracle, raw, level)
    return _expected[key]


def run_batch(lfmlib, torch, oracle, rows, level, multi):
    """The streams of `rows` (equal lengths) from one call, and whether RLE1
    read the image (rle1_crc<true, .>) or gather_blocks ran first.  multi: the
    multi entry at a geometry where a stream owns two slots, so that
    rle1_crc<., true>, place_parts, emit_stream<true> and join_parts run: rows
    shorter than MULTI_BLOCK are the border blocks of a grid whose whole blocks
    are MULTI_BLOCK run-free bytes."""
    n = len(rows[0])
    assert all(len(r) == n for r in rows) and len(rows) <= BATCH
    if not multi:
        if level == C.LEVEL:
            got, flags = encode(lfmlib, torch, [np.frombuffer(r, np.uint8) for r in rows])
        else:
            d = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy()).cuda()
            got, flags = lfmlib.bzip2_device(d, [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], 1, level=level)
        return got, flags, C.from_img(n, n)
    L = lfmlib.lib()
    if C.max_parts(n, level) >= 2:
        dims, bs, img, step = [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], b"".join(rows), 1
    else:
        bb = C.MULTI_BLOCK
        dims, bs, img, step = [bb + n, 1, len(rows), 1, 1], [bb, 1, 1, 1, 1], b"".join(C.multi_filler() + r for r in rows), 2
    assert C.max_parts(bs[0], level) == 2
    count = step * len(rows)
    assert L.lfm_hip_bzip2_workspace_bytes_multi(count, bs[0], level) > L.lfm_hip_bzip2_workspace_bytes(count, bs[0])
    d = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).cuda()
    assert d.data_ptr() % 16 == 0
    got, flags = lfmlib.bzip2_device(d, dims, bs, 1, level=level, multi=True)
    assert len(got) == count
    if step == 2:  # the whole blocks: one reference for all
        assert not any(flags[0::2]) and set(got[0::2]) == {expected(oracle, C.multi_filler(), level)}
    return got[step - 1::step], flags[step - 1::step], C.from_img(dims[0], bs[0])


def run_cases(lfmlib, torch, oracle, cases, level=C.LEVEL, multi=False):
    """Encode [(id, raw)] in batches of equal length; the ids that failed, and
    the set of load paths taken."""
    by_len = {}
    for cid, raw in cases:
        by_len.setdefault(len(raw), []).append((cid, raw))
    failed, paths = [], set()
    for n, group in by_len.items():
        for lo in range(0, len(group), BATCH):
            part = group[lo:lo + BATCH]
            got, flags, direct = run_batch(lfmlib, torch, oracle, [raw for _, raw in part], level, multi)
            paths.add(direct)
            for (cid, raw), g, f in zip(part, got, flags):
                if f != 0:
                    failed.append((cid, "flags %d" % f))
                elif g != expected(oracle, raw, level):
                    failed.append((cid, "bytes differ"))
    return failed, paths


def rows_of(groups):
    return [(cid, raw) for g in groups for cid, raw, _ in g]


def test_a_lengths(lfmlib, oracle, gpu):
    """List A: raw lengths 1..70 and around 128 .. 32 768, one call per length.
    A length of whole 16-byte units is read from the image, any other gathered."""
    failed, paths = run_cases(lfmlib, gpu, oracle, rows_of([C.length_cases()]))
    assert paths == {True, False}
    assert not failed, failed


@pytest.mark.parametrize("extra", [0, 1], ids=["from-image", "gathered"])
def test_b_rle1_seams(lfmlib, oracle, gpu, extra):
    """List B: runs placed on the chunk, wave and tile seams of rle1_crc, rows
    of whole 16-byte units (rle1_crc<true, false>) and the same one byte longer
    (gather_blocks, rle1_crc<false, false>)."""
    groups = C.rle1_cases(extra)
    for n in groups:
        assert C.from_img(n + extra, n + extra) == (extra == 0)
    failed, paths = run_cases(lfmlib, gpu, oracle, rows_of(groups.values()))
    assert paths == {extra == 0}
    assert not failed, failed


def test_b_rle1_whole_stream_runs(lfmlib, oracle, gpu):
    """List B: one value over a whole stream of 4 bytes and of three tiles and
    5 / 16 bytes, each a call of its own."""
    failed, paths = run_cases(lfmlib, gpu, oracle, rows_of([C.rle1_solo_cases()]))
    assert paths == {True, False}
    assert not failed, failed


def test_c_rle2(lfmlib, oracle, gpu):
    """List C: zero runs on the thread, wave and tile seams of rle2, final runs,
    no zero at all, values 1..4 only; the run of 40 000 in a call of its own."""
    failed, _ = run_cases(lfmlib, gpu, oracle, rows_of(C.rle2_cases().values()) + rows_of([C.rle2_solo_cases()]))
    assert not failed, failed


def test_d_mtf(lfmlib, oracle, gpu):
    failed, _ = run_cases(lfmlib, gpu, oracle, rows_of([C.mtf_cases()]))
    assert not failed, failed


def test_e_huffman(lfmlib, oracle, gpu):
    failed, _ = run_cases(lfmlib, gpu, oracle, rows_of([C.huffman_cases()]))
    assert not failed, failed


def test_f_emit_and_compaction(lfmlib, oracle, gpu):
    failed, _ = run_cases(lfmlib, gpu, oracle, rows_of([C.emit_cases()]))
    assert not failed, failed
    rows = C.compaction_batch()
    want = [expected(oracle, raw, C.LEVEL) for raw in rows]
    C.compaction_witness(want)
    got, flags, _ = run_batch(lfmlib, gpu, oracle, rows, C.LEVEL, False)
    assert flags == [0] * len(rows) and got == want


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_multi_entry_level1(lfmlib, oracle, gpu, which):
    """Lists A, B and C through lfm_hip_bzip2_blocks_multi at level 1 with two
    slots per stream: single-part streams through rle1_crc<., true>,
    place_parts, emit_stream<true> and join_parts.  The same bytes."""
    cases = {"A": lambda: rows_of([C.length_cases()]),
             "B": lambda: rows_of(C.rle1_cases(0).values()) + rows_of([C.rle1_solo_cases()]),
             "C": lambda: rows_of(C.rle2_cases().values()) + rows_of([C.rle2_solo_cases()])}[which]()
    failed, paths = run_cases(lfmlib, gpu, oracle, cases, level=1, multi=True)
    if which == "A":
        assert paths == {True, False}
    assert not failed, failed


def test_level9_tile_seams(lfmlib, oracle, gpu):
    """List B at the 16 384 seam and list C's rows with the 16 384 runs at level
    9: other capacities and write limits, the level digit in the bytes."""
    cases = rows_of([C.rle1_cases(0)[C.RLE1_ROW[16384]], C.rle2_cases()[C.RLE2_LARGE]])
    assert any(cid == "P16384-j224-R256" for cid, _ in cases) and any(cid == "pairs16384" for cid, _ in cases)
    failed, _ = run_cases(lfmlib, gpu, oracle, cases, level=9)
    assert not failed, failed
    cid, raw = cases[0]
    a, b = expected(oracle, raw, 9), expected(oracle, raw, C.LEVEL)
    assert a[:3] == b[:3] and a[3:4] == b"9" and a[4:] == b[4:]


def test_seam_cases_in_one_mixed_batch(lfmlib, oracle, gpu):
    """One call over a block grid with border blocks: streams of 36 864, 4 096,
    288 and 32 bytes, rows of every list, 2 to 6 coding tables, alphaSize 5 and
    258 side by side (the early-outs per stream, scan_offsets, compact_streams)."""
    torch = gpu
    rows = C.mixed_batch()
    img = C.place_blocks(C.MIXED_DIMS, C.MIXED_BS, [raw for _, raw in rows])
    d = torch.from_numpy(img.reshape(-1).copy()).cuda()
    got, flags = lfmlib.bzip2_device(d, C.MIXED_DIMS, C.MIXED_BS, 1, level=C.LEVEL)
    assert len(got) == len(rows)
    failed = [cid for (cid, raw), g, f in zip(rows, got, flags) if f != 0 or g != expected(oracle, raw, C.LEVEL)]
    assert not failed, failed
