"""GPU decode of bzip2 streams of several bzip2 blocks
(lfm_hip_bunzip2_blocks_multi, lfm.bunzip2_device(..., multi=True)) and the
readers that use it.  Expected bytes are the inputs the reference library
(oracle.bzip2(), BZ2_bzBuffToBuffCompress of bzip2-1.0.6) compressed, or the
oracle's pixels; the part counts and the bad streams' premises are checked on
the host by tests/test_bunzip2_multiblock_cpu.py.

Flags of lfm.bunzip2_device: 0 decoded, 1 handed to the host library (output
None), 2 decoded but a block CRC does not match (output None)."""
import ctypes

import numpy as np
import pytest

import bz2_multi_cases as M
import bz2_parts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bz(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


def check_exact(inputs, out, flags, what):
    bad = [(i, len(d), f) for i, (d, f) in enumerate(zip(inputs, flags)) if f != 0]
    assert not bad, (what, "flagged (index, length, flag)", bad)
    wrong = [(i, len(d)) for i, (d, o) in enumerate(zip(inputs, out)) if o != d]
    assert not wrong, (what, "wrong bytes (index, length)", wrong)


def test_cut_edges_level1(lfmlib, bz, gpu):
    """All 40 cut-rule edges of bz2_parts.level1_cases() in one call (1, 2, 3,
    5 and 6 parts; 9 slots per stream): a cut one byte early, exact and late,
    at the stream's last byte (a block of nblockMAX + 5), and inside a chain of
    255-byte pieces, where the next part begins with aaaa + count."""
    cases = bz2_parts.level1_cases()
    inputs = [d for _, d in cases]
    out, flags = lfmlib.bunzip2_device([bz.compress(d, 1) for d in inputs], 700000, multi=True, level=1)
    assert {n: f for (n, _), f in zip(cases, flags) if f} == {}
    assert [n for (n, d), o in zip(cases, out) if o != d] == []


@pytest.mark.parametrize("n,level,out_stride", [(450000, 2, 450001), (1000000, 9, 1000003)])
def test_levels_2_and_9(lfmlib, bz, gpu, n, level, out_stride):
    """3 parts at level 2 and 2 at level 9, each beside a short single-block
    stream, at an odd out_stride: the later parts' offsets and their `ab` in
    bzd_rle1 are unaligned."""
    inputs = [M.random_bytes(n, n), b"a short stream of one block " * 9 + b"."]  # (the dot: not periodic)
    out, flags = lfmlib.bunzip2_device([bz.compress(d, level) for d in inputs], out_stride, multi=True, level=level)
    check_exact(inputs, out, flags, "level %d" % level)


def test_mixed_batch(lfmlib, bz, gpu):
    """The encoder test's five rows (3, 1, 3, 4 and 3 parts): the one whose
    first part is periodic goes to the host whole, the others are exact."""
    rows = M.mixed_rows()
    out, flags = lfmlib.bunzip2_device([bz.compress(r, 1) for r in rows], 250000, multi=True, level=1)
    assert flags == [0, 0, 0, 0, 1] and out[4] is None
    assert [out[i] == rows[i] for i in range(4)] == [True] * 4


def test_bound_and_capacity(lfmlib, bz, gpu):
    """More blocks than slots (3 parts where level 2 gives 2 slots: bzd_huff,
    p + 1 == parts) and more bytes than out_stride (bzd_rle1 of the second
    part: base + tot > out_stride, nothing of it written) are flag 1, and the
    neighbours' regions hold their own bytes; one byte more of out_stride and
    the same stream fills its region exactly."""
    small = [M.random_bytes(3000, 1), bytes(5000) + M.random_bytes(100, 2)]
    three = M.random_bytes(250000, 4)
    streams = [bz.compress(small[0], 1), bz.compress(three, 1), bz.compress(small[1], 1)]
    out, flags = lfmlib.bunzip2_device(streams, 250000, multi=True, level=2)
    assert flags == [0, 1, 0] and out == [small[0], None, small[1]]
    # (at its own level the stream has its slots)
    out, flags = lfmlib.bunzip2_device(streams, 250000, multi=True, level=1)
    check_exact([small[0], three, small[1]], out, flags, "level 1")
    d = bz2_parts.run_free(120001)
    streams = [bz.compress(small[0], 1), bz.compress(d, 1), bz.compress(small[1], 1)]
    out, flags = lfmlib.bunzip2_device(streams, 120000, multi=True, level=1)
    assert flags == [0, 1, 0] and out == [small[0], None, small[1]]
    out, flags = lfmlib.bunzip2_device(streams, 120001, multi=True, level=1)
    check_exact([small[0], d, small[1]], out, flags, "exact fill")


def test_bad_two_part_streams_are_flagged(lfmlib, bz, gpu):
    """A 2-part stream with one field damaged (libbzip2 rejects each), good
    streams between them.  Flag 2: the second block's CRC field and the
    combined CRC changed alike (bzd_rle1 of the second slot: crc != D.crc[s]).
    Flag 1, all in bzd_huff: the combined CRC alone (ccrc != comb), the second
    block's magic or the end magic damaged (the 48 bits behind a block are
    neither magic), cut off inside the second block, and the second block's
    origPtr == its n (origPtr >= nblock).

    None reads or writes outside its slots.  bzd_huff writes ll only at
    ll + nblock .. behind the check nblock + total > cap of the slot it is in,
    and moves to the next slot only behind p + 1 == parts; words past a cut
    stream read as 0 (a clamped index) until over() at the next group, a bad
    code, nInUse == 0 or a start length of 0 ends it.  origPtr is checked
    before the slot's words are written, so bzd_walk never reads tt[origPtr]
    of a flagged stream: every slot of one carries its flag and n = 0, and
    bzd_tt, bzd_walk and bzd_rle1 leave such slots alone.  With a wrong CRC
    everything is decoded as for the good stream; only the comparison at the
    end differs.  test_multi_workspace_is_exactly_its_size covers the rest."""
    data, stream, _ = M.two_part(bz.compress)
    bad = M.bad_two_part(bz.compress)
    rng = np.random.default_rng(23)
    good = [data] + [rng.integers(0, 1 + 3 * (i % 5) ** 3, 200 + 37 * i, dtype=np.uint8).tobytes()
                     for i in range(len(bad))]
    streams = [stream]
    for (_, s, _), g in zip(bad, good[1:]):
        streams += [s, bz.compress(g, 1)]
    out, flags = lfmlib.bunzip2_device(streams, M.TWO_PART_STRIDE, multi=True, level=1)
    assert {name: f for (name, _, _), f in zip(bad, flags[1::2])} == {name: want for name, _, want in bad}
    assert all(o is None for o in out[1::2])
    assert flags[0::2] == [0] * len(good)
    assert out[0::2] == good


def test_multi_workspace_is_exactly_its_size(lfmlib, bz, gpu):
    """lfm_hip_bunzip2_blocks_multi with exactly its workspace and exactly its
    output between 4 KiB guards: one byte of workspace less is refused before
    anything runs, the exact size leaves the guards alone."""
    torch = gpu
    L = lfmlib.lib()
    GUARD, FILL = 4096, 0xA5
    n, count = 250000, 2
    inputs = [M.random_bytes(n, 6), np.random.default_rng(7).integers(0, 3, n, dtype=np.uint8).tobytes()]
    assert [len(bz2_parts.parts(d, 1)) for d in inputs] == [3, 3]
    streams = [bz.compress(d, 1) for d in inputs]
    offs = (ctypes.c_uint64 * (count + 1))(0, len(streams[0]), len(streams[0]) + len(streams[1]))
    pay = torch.frombuffer(bytearray(b"".join(streams) + bytes(64)), dtype=torch.uint8).cuda()
    ws_bytes = L.lfm_hip_bunzip2_workspace_bytes_multi(count, n, 1)
    assert ws_bytes > 3 * L.lfm_hip_bunzip2_workspace_bytes(count, 100000)
    ws = torch.full((GUARD + 256 + ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lo = GUARD + (-(ws.data_ptr() + GUARD)) % 256
    out = torch.full((GUARD + count * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(nbytes):
        lens, flags = (ctypes.c_uint32 * count)(), (ctypes.c_uint32 * count)()
        rc = L.lfm_hip_bunzip2_blocks_multi(pay.data_ptr(), offs, count, out.data_ptr() + GUARD, n, 1,
                                            ws.data_ptr() + lo, nbytes, lens, flags, None)
        torch.cuda.synchronize()
        return rc, list(lens), list(flags)

    rc, lens, flags = call(ws_bytes - 1)
    assert rc == 1  # LFM_HIP_EINVAL
    assert not any(lens) and bool((ws == FILL).all()) and bool((out == FILL).all())  # nothing ran
    rc, lens, flags = call(ws_bytes)
    assert rc == 0 and flags == [0, 0] and lens == [n, n]
    assert bool((ws[:lo] == FILL).all()), "guard before the workspace written"
    assert bool((ws[lo + ws_bytes:] == FILL).all()), "guard after the workspace written"
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + count * n:] == FILL).all()), "output guards written"
    host = out[GUARD:GUARD + count * n].cpu().numpy().tobytes()
    assert host[:n] == inputs[0] and host[n:] == inputs[1]
    assert L.lfm_hip_bunzip2_blocks_multi(pay.data_ptr(), offs, count, out.data_ptr() + GUARD, n, 0,
                                          ws.data_ptr() + lo, ws_bytes, (ctypes.c_uint32 * count)(),
                                          (ctypes.c_uint32 * count)(), None) == 1  # level 0


def test_single_entry_unchanged(lfmlib, bz, gpu):
    """The single-block entry still hands a 2-part stream to the host, and a
    batch with one slot per stream decodes alike through both entries."""
    data, stream, _ = M.two_part(bz.compress)
    short = M.random_bytes(700, 3)
    out, flags = lfmlib.bunzip2_device([stream, bz.compress(short, 1)], M.TWO_PART_STRIDE)
    assert flags == [1, 0] and out == [None, short]
    rng = np.random.default_rng(12)
    inputs = [rng.integers(0, 1 + 7 * i, 1000 + 811 * i, dtype=np.uint8).tobytes() for i in range(9)]
    streams = [bz.compress(d, 1) for d in inputs] + [stream]  # the last has a second block: flag 1
    assert lfmlib.bunzip2_max_parts(9001, 1) == 1
    single = lfmlib.bunzip2_device(streams, 9001)
    multi = lfmlib.bunzip2_device(streams, 9001, multi=True, level=1)
    assert multi == single == (inputs + [None], [0] * 9 + [1])


def test_engine_16bit_streams_of_several_blocks(lfmlib, oracle, gpu):
    """The oracle's .lfm of predicted 16-bit symbols in 1 MiB blocks (level 9,
    two streams of several bzip2 blocks each): device and host destinations
    and a region that is no box of blocks return the pixels with no block
    handed to the host library; with the switch off both streams go there."""
    X = Y = 256
    Z, T, k = 16, 13, 4
    img = oracle.synthetic_lf(X, Y, Z=Z, T=T, seed=0x905)
    bs = [256, 256, 8, 1, 1]
    b = oracle.encode(img, header_version=8 + k, nnum=T, family="tiles", block_size=bs)
    old = lfmlib.get_family()
    lfmlib.set_family("tiles")
    try:
        assert lfmlib.get_bunzip2_multiblock() is True
        dev, st = lfmlib.decode_device(b, return_stats=True)
        assert (st["path"], st["blocks"], st["host_blocks"]) == (0, 2, 0)
        assert np.array_equal(dev.cpu().numpy(), img)
        assert np.array_equal(lfmlib.decode(b), img)
        lb, ub = [3, 5, 2, 0, 0], [200, 130, 11, 0, 0]
        roi, st = lfmlib.decode_roi_device(b, lb, ub, return_stats=True)
        assert st["host_blocks"] == 0
        assert np.array_equal(roi.cpu().numpy(), img[:, :, 2:12, 5:131, 3:201])
        assert lfmlib.set_bunzip2_multiblock(False) is True
        dev, st = lfmlib.decode_device(b, return_stats=True)
        assert (st["path"], st["blocks"], st["host_blocks"]) == (0, 2, 2)
        assert np.array_equal(dev.cpu().numpy(), img)
    finally:
        lfmlib.set_bunzip2_multiblock(True)
        lfmlib.set_family(old)


def test_engine_8bit_growth_and_periodic(lfmlib, oracle, gpu):
    """Two 95 000-byte streams: one of two bzip2 blocks by RLE1 growth, now
    decoded on the device, one periodic, which stays with the host library."""
    runs4 = np.repeat(np.arange(190000 // 4, dtype=np.uint32) % 251, 4).astype(np.uint8)
    img = np.stack([runs4[:95000].reshape(1, 95000), np.tile(np.array([[3, 7]], np.uint8), (1, 47500))])
    img = img.reshape(1, 1, 2, 1, 95000)
    b = oracle.encode(img, data_type=0, header_version=8, nnum=13, block_size=[95000, 1, 1, 1, 1])
    try:
        dev, st = lfmlib.decode_device(b, return_stats=True)
        assert (st["path"], st["blocks"], st["host_blocks"]) == (0, 2, 1)
        assert np.array_equal(dev.cpu().numpy(), img)
        assert lfmlib.set_bunzip2_multiblock(False) is True
        dev, st = lfmlib.decode_device(b, return_stats=True)
        assert (st["path"], st["blocks"], st["host_blocks"]) == (0, 2, 2)
        assert np.array_equal(dev.cpu().numpy(), img)
    finally:
        lfmlib.set_bunzip2_multiblock(True)
