"""GPU bzip2 of streams that libbzip2 cuts into several bzip2 blocks
(lfm_hip_bzip2_blocks_multi): the device finds the cuts, compresses every part
and joins them at bit offsets; the bytes are BZ2_bzBuffToBuffCompress's.  The
cut rule and the expected part counts are tests/bz2_parts.py, checked against
the reference library on the CPU by tests/test_bz2_parts_cpu.py."""
import numpy as np
import pytest

import bz2_parts

pytestmark = pytest.mark.gpu

CASES = bz2_parts.level1_cases()


def ref_bz2(oracle, data, level):
    """BZ2_bzBuffToBuffCompress(level, 0, 30) of the reference's bzip2-1.0.6
    (oracle/_ref/libbz2_ref.so, as in tests/test_gpu.py)."""
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz.compress(bytes(data), level)


def one_stream(torch, lfmlib, data, level, multi=True):
    a = np.frombuffer(data, dtype=np.uint8)
    d = torch.from_numpy(a.copy()).cuda()
    return lfmlib.bzip2_device(d, [len(a), 1, 1, 1, 1], [len(a), 1, 1, 1, 1], 1, level=level, multi=multi)


@pytest.mark.parametrize("name,data", CASES, ids=[n for n, _ in CASES])
def test_cut_edges_level1(lfmlib, oracle, gpu, name, data):
    """One stream at level 1 (nblockMAX 99 981) around every edge of the cut
    rule: the limit reached one byte early / exactly / late, at the stream's
    last byte, inside a chain of 255-byte pieces, and several cuts."""
    got, flags = one_stream(gpu, lfmlib, data, 1)
    assert flags == [0]
    assert got[0] == ref_bz2(oracle, data, 1), (name, len(bz2_parts.parts(data, 1)))


@pytest.mark.parametrize("n,level,nparts", [(450000, 2, 3), (1000000, 9, 2)])
def test_levels_2_and_9(lfmlib, oracle, gpu, n, level, nparts):
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert len(bz2_parts.parts(data, level)) == nparts
    got, flags = one_stream(gpu, lfmlib, data, level)
    assert flags == [0]
    assert got[0] == ref_bz2(oracle, data, level)


def test_level9_single_part_control(lfmlib, oracle, gpu):
    """899 000 random bytes at level 9 through the single-block entry: one part
    of nearly nblockMAX bytes, the size of a level-9 part of a longer stream."""
    data = np.random.default_rng(9).integers(0, 256, 899000, dtype=np.uint8).tobytes()
    assert len(bz2_parts.parts(data, 9)) == 1
    got, flags = one_stream(gpu, lfmlib, data, 9, multi=False)
    assert flags == [0]
    assert got[0] == ref_bz2(oracle, data, 9)


def test_mixed_batch(lfmlib, oracle, gpu):
    """Five streams of one call: three parts, one part, low entropy, text grown
    to 5/4 by runs of exactly four, and one whose first part is periodic (33 327
    x "abc"): that one alone is flagged for the host."""
    torch = gpu
    n = 250000
    rng = np.random.default_rng(3)
    rows = [rng.integers(0, 256, n, dtype=np.uint8),
            np.zeros(n, np.uint8),
            rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), n),
            np.repeat(np.arange(n // 4, dtype=np.uint32) % 251, 4).astype(np.uint8),
            np.frombuffer((b"abc" * 83334)[:n], dtype=np.uint8)]
    assert [len(bz2_parts.parts(r.tobytes(), 1)) for r in rows] == [3, 1, 3, 4, 3]
    assert bz2_parts.parts(rows[4].tobytes(), 1)[0][2] == 3 * 33327
    img = np.stack(rows)
    d = torch.from_numpy(img.reshape(-1).copy()).cuda()
    got, flags = lfmlib.bzip2_device(d, [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], 1, level=1, multi=True)
    assert flags == [0, 0, 0, 0, 1] and got[4] is None
    equal = [got[i] == ref_bz2(oracle, rows[i].tobytes(), 1) for i in range(4)]
    assert equal == [True] * 4


def test_multi_workspace_is_exactly_its_size(lfmlib, oracle, gpu):
    """lfm_hip_bzip2_blocks_multi with exactly its workspace between two
    guards, one byte less refused before anything runs; with one part per
    stream the size is lfm_hip_bzip2_workspace_bytes's."""
    torch = gpu
    import ctypes
    L = lfmlib.lib()
    for bb, lv in ((4096, 1), (147456, 2), (192, 1)):
        for count in (1, 3):
            assert L.lfm_hip_bzip2_workspace_bytes_multi(count, bb, lv) == L.lfm_hip_bzip2_workspace_bytes(count, bb)
    GUARD, FILL = 4096, 0xA5
    n, count = 250000, 2
    rng = np.random.default_rng(6)
    img = np.stack([rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 3, n, dtype=np.uint8)])
    d = torch.from_numpy(img.reshape(-1).copy()).cuda()
    dims, bs = [n, 1, count, 1, 1], [n, 1, 1, 1, 1]
    ws_bytes = L.lfm_hip_bzip2_workspace_bytes_multi(count, n, 1)
    assert ws_bytes > L.lfm_hip_bzip2_workspace_bytes(count, n) // 4
    out_cap = L.lfm_hip_bzip2_out_cap(n)
    buf = torch.full((GUARD + 256 + ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lo = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    pay = torch.full((count * out_cap,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(nbytes):
        sizes, flags = (ctypes.c_uint64 * count)(), (ctypes.c_uint32 * count)()
        rc = L.lfm_hip_bzip2_blocks_multi(d.data_ptr(), (ctypes.c_uint32 * 5)(*dims), (ctypes.c_uint32 * 5)(*bs), 1, 0,
                                          count, 1, buf.data_ptr() + lo, nbytes, pay.data_ptr(), sizes, flags, None)
        torch.cuda.synchronize()
        return rc, list(sizes), list(flags)

    rc, sizes, flags = call(ws_bytes - 1)
    assert rc == 1  # LFM_HIP_EINVAL
    assert not any(sizes) and bool((buf == FILL).all()) and bool((pay == 0x5A).all())  # nothing ran
    rc, sizes, flags = call(ws_bytes)
    assert rc == 0 and not any(flags)
    assert bool((buf[:lo] == FILL).all()), "guard before the workspace written"
    assert bool((buf[lo + ws_bytes:] == FILL).all()), "guard after the workspace written"
    host = pay[:sum(sizes)].cpu().numpy().tobytes()
    assert host[:sizes[0]] == ref_bz2(oracle, img[0].tobytes(), 1)
    assert host[sizes[0]:] == ref_bz2(oracle, img[1].tobytes(), 1)


def test_encoder_8bit_counts_and_switch(lfmlib, oracle, gpu):
    """The image of test_gpu_bzip2_host_fallback_streams: the row whose RLE1
    text passes nblockMAX is now two bzip2 blocks from the GPU, the periodic
    row stays with the host; with the switch off both go to the host.  Same
    bytes either way."""
    torch = gpu
    runs4 = np.repeat(np.arange(190000 // 4, dtype=np.uint32) % 251, 4).astype(np.uint8)
    img = np.stack([runs4[:95000].reshape(1, 95000), np.tile(np.array([[3, 7]], np.uint8), (1, 47500))])
    img = img.reshape(1, 1, 2, 1, 95000)
    assert len(bz2_parts.parts(img[0, 0, 0].tobytes(), 1)) == 2
    kw = dict(header_version=8, nnum=13, block_size=[95000, 1, 1, 1, 1])
    want = oracle.encode(img, data_type=0, **kw)
    d = torch.from_numpy(img.copy()).cuda()
    enc = lfmlib.Encoder(device=0)
    try:
        b, _ = enc.encode(d, **kw)
        assert b == want
        assert enc.stream_counts() == {"streams": 2, "host_streams": 1, "bzip2_blocks": 2}
        assert lfmlib.set_bzip2_multiblock(False) is True
        b, _ = enc.encode(d, **kw)
        assert b == want
        assert enc.stream_counts() == {"streams": 2, "host_streams": 2, "bzip2_blocks": 0}
    finally:
        lfmlib.set_bzip2_multiblock(True)
        enc.close()


@pytest.mark.parametrize("fam", ["tiles", "angle"])
def test_encoder_16bit_blocks_over_900k(lfmlib, oracle, gpu, fam):
    """1 MiB blocks (level 9) of predicted 16-bit symbols: every stream is
    several bzip2 blocks, none goes to the host, and the reader (which still
    takes multi-block streams to the host library) returns the image."""
    torch = gpu
    X = Y = 256
    Z, T, k = 16, 13, 4
    img = oracle.synthetic_lf(X, Y, Z=Z, T=T, seed=0x900 + len(fam))
    bs = [256, 256, 8, 1, 1]
    old = lfmlib.get_family()
    lfmlib.set_family(fam)
    enc = lfmlib.Encoder(device=0)
    try:
        d = torch.from_numpy(img[0, 0].view(np.int16).copy()).cuda()
        b, _ = enc.encode(d, header_version=8 + k, nnum=T, block_size=bs)
        counts = enc.stream_counts()
        back = lfmlib.decode(b)  # (the family is a process setting, not in the file)
    finally:
        enc.close()
        lfmlib.set_family(old)
    assert b == oracle.encode(img, header_version=8 + k, nnum=T, family=fam, block_size=bs)
    sym = oracle.predict_volume(img[0, 0], T, fam, k, 0)
    nparts = [len(bz2_parts.parts(oracle.gather_block(sym[None, None], coord, size), 9))
              for _, coord, size in oracle.iter_blocks([X, Y, Z, 1, 1], bs)]
    assert len(nparts) == 2 and sum(nparts) > 2
    assert counts == {"streams": 2, "host_streams": 0, "bzip2_blocks": sum(nparts)}
    assert np.array_equal(back, img)
