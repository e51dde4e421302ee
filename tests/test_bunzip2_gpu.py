"""Edge cases of the GPU bzip2 decoder (csrc/lfm_bunzip2.hip: bzd_huff, bzd_tt,
bzd_walk, bzd_rle1) against libbzip2.  Every comparison is byte-exact: the
expected bytes are what the reference library compressed or, for streams
written by tests/bz2_craft.py, what it decompresses (test_bz2_craft_cpu.py
checks that, and that each case sits on its edge, on the host).

Flags of lfm.bunzip2_device: 0 decoded, 1 handed to the host library (output
None), 2 decoded but the block CRC does not match (output None)."""
import numpy as np
import pytest

import bz2_cases as K
import bz2_craft as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bz(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


def check_good(lfmlib, inputs, streams, out_stride, what):
    out, flags = lfmlib.bunzip2_device(streams, out_stride)
    bad = [(i, len(d), f) for i, (d, f) in enumerate(zip(inputs, flags)) if f != 0]
    assert not bad, (what, out_stride, "flagged (index, length, flag)", bad)
    wrong = [(i, len(d)) for i, (d, o) in enumerate(zip(inputs, out)) if o != d]
    assert not wrong, (what, out_stride, "wrong bytes (index, length)", wrong)


def test_size_and_alignment_sweep(lfmlib, bz, gpu):
    """Lengths around the 16-byte chunk, the 256-thread tile and the 4096-byte
    staged block of bzd_tt, random and 4-symbol bytes, one batch: every stream
    start alignment (WaveBits::init) and every group count 2..6, decoded at an
    out_stride that is not a multiple of 16 (bzd_rle1's `ab` differs from
    stream to stream) and at one that is."""
    inputs = K.sweep_inputs()
    streams = [bz.compress(d, 1) for d in inputs]
    starts = np.cumsum([0] + [len(s) for s in streams])[:-1]
    assert {int(o) % 4 for o in starts} == {0, 1, 2, 3}
    assert {C.parse(s)["ngroups"] for s in streams} == {2, 3, 4, 5, 6}
    for out_stride in (9001, 9008):
        check_good(lfmlib, inputs, streams, out_stride, "sweep")


@pytest.mark.parametrize("fill,out_stride", [(0, 1399), (360, 4243)])
def test_rle1_seams(lfmlib, bz, gpu, fill, out_stride):
    """Runs of 4 (count 0), 5, 8, 9, 255, 256, 259, 510 and a run ending the
    block, count bytes equal to their run's byte, behind k = 0..47 plain bytes:
    every state of bzd_rle1's machine crosses a lane-segment seam (segments of
    16 bytes with the text below 1024 bytes, where most lanes are empty, and of
    48 bytes at about 3000), at an odd out_stride."""
    inputs = K.rle_seam_inputs(fill)
    assert max(len(d) for d in inputs) <= out_stride
    check_good(lfmlib, inputs, [bz.compress(d, 1) for d in inputs], out_stride, "rle1 seams")


def test_walk_starts_on_a_marker(lfmlib, gpu):
    """bzd_walk with extra == false: the walk's start node v0 is a regular
    marker (row 128 m), for every m of blocks of 1 .. 4000 bytes; the chain
    then starts at marker v0 / 128, not at the extra walker."""
    cases = K.marker_cases()
    assert all(info["v0"] % 128 == 0 for _, _, info in cases)
    assert {info["v0"] // 128 for _, _, info in cases} == set(range(32))
    check_good(lfmlib, [t for t, _, _ in cases], [s for _, s, _ in cases], 4001, "marker")


def test_periodic_streams_go_to_the_host(lfmlib, bz, gpu):
    """An exactly periodic RLE1 text makes the LF permutation several cycles:
    bzd_walk cannot walk it as one (s_total == 0) and flags the stream for the
    host library.  The same texts with one more byte are not periodic and
    decode on the device, in the same batch.  Among them w w of at most 128
    bytes and w w w of 129 .. 256, from libbzip2 and with each origPtr that
    names one of the equal rows: there the walk has one walker per cycle, and
    a chain that went round the start's cycle two or three times would count
    every segment and byte (bz2_cases.chain_wraps) and leave the other
    segments' output offsets unwritten."""
    per = K.periodic_inputs()
    inputs, streams = [], []
    for d in per:
        inputs += [d, d + d[:1]]
        streams += [bz.compress(d, 1), bz.compress(d + d[:1], 1)]
    rep = K.repeated_cases()
    assert sum(w for _, _, w in rep) == 5
    for text, stream, _ in rep:
        inputs += [text, text, text + text[:1]]
        streams += [stream, bz.compress(text, 1), bz.compress(text + text[:1], 1)]
    want = [1, 0] * len(per) + [1, 1, 0] * len(rep)
    out, flags = lfmlib.bunzip2_device(streams, 12289)
    assert flags == want
    for d, o, f in zip(inputs, out, flags):
        assert o == (None if f else d), len(d)


def test_crafted_good(lfmlib, gpu):
    """Valid streams libbzip2's compressor never writes: 2..6 groups with
    cycling selectors and tables that differ, code lengths of 20 throughout
    (every symbol takes the limit walk), 17..20 (incomplete code), flat 9, EOB
    as the 50th symbol of the last group and alone in it, a RUNA/RUNB run over
    a group seam (the `rs` carry), 1, 2 and 256 bytes in use (move-to-front
    position 255), unused trailing selectors.

    Decoded on the device (flag 0, exact bytes): all of them but two.
    Handed to the host (flag 1), as read from the kernels:
      ninuse1_n5   the text 5 5 5 5 5 is constant, so periodic: bzd_walk, s_total == 0
      extra_sel5   EOB in a group that is not the last selector's: bzd_huff,
                   `if (__ballot(lane < 50 && symv == EOB)) flag = kHost`
    Never flag 0 with other bytes."""
    cases = K.crafted_good()
    out, flags = lfmlib.bunzip2_device([s for _, _, s, _, _ in cases], 2801)
    got = {name: f for (name, _, _, _, _), f in zip(cases, flags)}
    assert got == {name: 0 if on_device else 1 for name, _, _, _, on_device in cases}
    for (name, data, _, _, _), o, f in zip(cases, out, flags):
        assert o == (None if f else data), name


def test_bad_streams_are_flagged(lfmlib, bz, gpu):
    """Streams libbzip2 rejects, each caught by one check of
    csrc/lfm_bunzip2.hip, named by its condition (none of the checked values
    indexes anything before its check):
      trunc13          bzd_huff  b1 - b0 < 14
      trunc_symbols    bzd_huff  over() at the start of a group (words past the stream read as 0
                       through a clamped index); a bad code (zn > kMaxLen || idx < 0 || idx >= alphaSize),
                       a run of 2^21 (j >= 21) or the block capacity (nblock + total > cap), all before
                       any store, may come first
      block_magic      bzd_huff  m1 / m2
      randomised       bzd_huff  the randomised bit
      orig_eq_n, orig_max  bzd_huff  origPtr >= nblock (before bzd_walk reads tt[origPtr])
      ngroups1, ngroups7, nsel0  bzd_huff  nGroups < 2 || nGroups > kMaxGroups || nSel < 1
      selector_unary   bzd_huff  ++j >= nGroups (before `pos` is shifted by 4 * j)
      startlen0, startlen21  bzd_huff  curr < 1 || curr > kMaxLen (before slen / scnt are written)
      eos_magic        bzd_huff  e1 / e2
      combined_crc     bzd_huff  ccrc != bcrc
    all flag 1; and, decoded in full but with the wrong CRC, flag 2 (kCrcFail):
      crc_both         bzd_rle1  crc != D.crc[s]: both CRC fields changed alike
      orig_wrong       bzd_rle1  crc != D.crc[s]: an origPtr in range: another rotation of the text
    Good streams sit between them and decode exactly."""
    bad = K.crafted_bad()
    rng = np.random.default_rng(21)
    good = [rng.integers(0, 1 + 3 * (i % 5) ** 3, 200 + 37 * i, dtype=np.uint8).tobytes() for i in range(len(bad) + 1)]
    streams = [bz.compress(good[0], 1)]
    for (_, s, _), g in zip(bad, good[1:]):
        streams += [s, bz.compress(g, 1)]
    out, flags = lfmlib.bunzip2_device(streams, 1001)
    assert {name: f for (name, _, _), f in zip(bad, flags[1::2])} == {name: want for name, _, want in bad}
    assert all(o is None for o in out[1::2])
    assert flags[0::2] == [0] * len(good)
    assert out[0::2] == good


@pytest.mark.parametrize("out_stride,level", [(350000, 4), (900000, 9)])
def test_large_blocks(lfmlib, bz, gpu, out_stride, level):
    """Blocks of level 4 and up: bzd_walk<512, false> (marker tables in global
    memory), the large selector area of bzd_huff and bzd_tt beyond 200 064
    bytes.  One decode call per case."""
    rng = np.random.default_rng(out_stride)
    if level == 4:
        inputs = [rng.integers(0, 256, 350000, dtype=np.uint8).tobytes(), b"small block",
                  rng.integers(0, 4, 350000, dtype=np.uint8).tobytes(),
                  rng.integers(0, 9, 3000, dtype=np.uint8).tobytes()]
    else:
        low = rng.integers(0, 6, 900000, dtype=np.uint8)
        low[1000:9000] = 3  # one long run, so that the text after RLE1 stays one bzip2 block
        inputs = [low.tobytes(), rng.integers(0, 256, 120000, dtype=np.uint8).tobytes()]
    check_good(lfmlib, inputs, [bz.compress(d, level) for d in inputs], out_stride, "large")


def test_out_stride_limits(lfmlib, bz, gpu):
    """A stream decoding to exactly out_stride bytes is decoded, one byte more
    goes to the host (bzd_rle1: tot > cap) and writes nothing past its region:
    the next stream's region holds its own bytes.  A block longer than the
    batch's capacity (level 9 in a level-1 batch) goes to the host in bzd_huff."""
    rng = np.random.default_rng(5)
    base = (rng.integers(0, 3, 1002, dtype=np.uint8) * (rng.integers(0, 4, 1002) == 0)).astype(np.uint8).tobytes()
    assert len(C.rle1(base)) != len(base)
    inputs = [base[:1001], base, base[:500], rng.integers(0, 256, 150000, dtype=np.uint8).tobytes(), base[1:]]
    streams = [bz.compress(d, 1) for d in inputs[:3]] + [bz.compress(inputs[3], 9), bz.compress(inputs[4], 1)]
    out, flags = lfmlib.bunzip2_device(streams, 1001)
    assert flags == [0, 1, 0, 1, 0]
    assert out == [inputs[0], None, inputs[2], None, inputs[4]]


def test_engine_host_fallback_on_decode(lfmlib, oracle, bz, gpu):
    """A file whose blocks are half constant (0x0201: a period-2 text without
    runs, exactly periodic) and half noise: lfm.decode returns every pixel,
    and the same streams cut out of the file come back flagged 1 exactly on
    the constant blocks, so the file read went through the engine's host
    branch (decompress_one, then the copy into the slot) for those.  With
    both CRC fields of one noise block changed the file does not decode."""
    rng = np.random.default_rng(12)
    img = rng.integers(0, 65536, (16, 256, 256), dtype=np.uint16)
    bs = [64, 64, 8, 1, 1]
    const = []
    for bid, (x0, y0, z0, _, _), _ in oracle.iter_blocks([256, 256, 16, 1, 1], bs):
        const.append((x0 // 64 + y0 // 64 + z0 // 8) % 2 == 0)
        if const[-1]:
            img[z0:z0 + 8, y0:y0 + 64, x0:x0 + 64] = 0x0201
    buf = oracle.encode(img, header_version=8, nnum=13, block_size=bs)  # request 8: predictor 0 forced
    h = oracle.parse_header(buf)
    assert h["header_version"] == 0 and h["nb"] == 32 and sum(const) == 16
    assert np.array_equal(lfmlib.decode(buf)[0, 0], img)
    ends = [h["header_size"] + int(e) for e in h["offsets"]]
    begs = [h["header_size"]] + ends[:-1]
    streams = [buf[a:b] for a, b in zip(begs, ends)]
    out, flags = lfmlib.bunzip2_device(streams, 65536)
    assert flags == [1 if c else 0 for c in const]
    for (bid, coord, size), o, c in zip(oracle.iter_blocks([256, 256, 16, 1, 1], bs), out, const):
        assert o == (None if c else oracle.gather_block(img[None, None], coord, size)), bid
    victim = const.index(False)
    twin = C.set_crcs(streams[victim], C.parse(streams[victim])["crc"] ^ 1)
    assert len(twin) == len(streams[victim])
    assert lfmlib.bunzip2_device([twin], 65536)[1] == [2]
    with pytest.raises(lfmlib.LfmError):
        lfmlib.decode(buf[:begs[victim]] + twin + buf[ends[victim]:])
