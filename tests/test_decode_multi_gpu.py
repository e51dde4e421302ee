"""Multi-GPU reader (lfm.decode_multi, lfm.decode_device_sharded, the drop-in
readers with a decode device list): one .lfm cut into ranges of whole block
layers, one worker per range.  On a one-GPU box the workers are [0] * n, every
one with its own thread, streams and buffers, so the path is the one an 8-GPU
node runs.  The files come from the CPU oracle; every result must equal the
input array and the single-device lfm.decode, and the shards' stats must show
that every block was decoded once, straight into place."""
import ctypes
import threading
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VBS = [64, 32, 3, 1, 1]


@pytest.fixture(autouse=True)
def restore(lfmlib):
    lfmlib.set_decode_devices(None)
    yield
    lfmlib.set_decode_devices(None)
    lfmlib.release_decoders()
    lfmlib.set_family("tiles")


def zlib_file(oracle, img, bs):
    """An unpredicted uint16 ZLIB file (the oracle writes NONE and BZIP2 only)."""
    xyzct = [img.shape[4], img.shape[3], img.shape[2], img.shape[1], img.shape[0]]
    blobs = [zlib.compress(oracle.gather_block(img, coord, size)) for _, coord, size in oracle.iter_blocks(xyzct, bs)]
    offsets = np.cumsum([len(b) for b in blobs]).astype(np.uint64)
    return oracle.header_bytes(0, 13, xyzct, [1.0] * 5, 1, 2, None, bs, offsets) + b"".join(blobs)


@pytest.fixture(scope="module")
def files(lfmlib, oracle, gpu):
    """{name: (family, image [t, c, z, y, x], .lfm bytes, lfm.decode's image)}:
    the plan tests' shapes over the three families (temporal prediction is
    invertible for tiles only, so the video files are tiles), a uint8 file, a
    half-constant file, and the files that are not farmed.  The single-device
    decode is taken once, here, with no device list."""
    lfmlib.set_decode_devices(None)
    vid = oracle.synthetic_lf(200, 96, Z=20, T=13, seed=0x4C464D0A)
    dflt = oracle.synthetic_lf(300, 200, Z=20, T=15, seed=0x4C464D0B)
    t3c2 = oracle.synthetic_lf(128, 100, Z=5, C=2, Tn=3, T=13, seed=0x4C464D0C)
    t1c3 = oracle.synthetic_lf(128, 100, Z=5, C=3, Tn=1, T=13, seed=0x4C464D0C)
    rng = np.random.default_rng(31)
    u8 = rng.integers(0, 7, (1, 1, 7, 33, 50), dtype=np.uint8)
    half = rng.integers(0, 65536, (1, 1, 16, 256, 256), dtype=np.uint16)
    for _, (x0, y0, z0, _, _), _ in oracle.iter_blocks([256, 256, 16, 1, 1], [64, 64, 8, 1, 1]):
        if (x0 // 64 + y0 // 64 + z0 // 8) % 2 == 0:
            half[0, 0, z0:z0 + 8, y0:y0 + 64, x0:x0 + 64] = 0x0201  # (periodic: the host library's)
    small = oracle.synthetic_lf(80, 80, Z=4, T=13, seed=0x4C464D24)
    B = [64, 64, 2, 1, 1]
    spec = {
        "video": ("tiles", vid, dict(header_version=0x80 | 12, nnum=13, block_size=VBS)),
        "still_angle": ("angle", vid, dict(header_version=12, nnum=13, block_size=VBS)),
        "still_space": ("space", vid, dict(header_version=12, nnum=13, block_size=VBS)),
        "default_tiles": ("tiles", dflt, dict(header_version=12, nnum=15)),
        "default_angle": ("angle", dflt, dict(header_version=12, nnum=15)),
        "t3c2_video": ("tiles", t3c2, dict(header_version=0x80 | 12, nnum=13, block_size=B)),
        "t3c2_space": ("space", t3c2, dict(header_version=12, nnum=13, block_size=B)),
        "t1c3_video": ("tiles", t1c3, dict(header_version=0x80 | 12, nnum=13, block_size=B)),
        "uint8": ("tiles", u8, dict(data_type=0, block_size=[16, 16, 2, 1, 1])),
        "half_constant": ("tiles", half, dict(header_version=8, nnum=13, block_size=[64, 64, 8, 1, 1])),
        # not farmed
        "none": ("tiles", small, dict(header_version=12, nnum=13, compression=0, block_size=[32, 32, 1, 1, 1])),
        "nnum40": ("tiles", small, dict(header_version=12, nnum=40, block_size=[32, 32, 1, 1, 1])),
        "one_unit": ("tiles", small, dict(header_version=12, nnum=13, block_size=[32, 32, 4, 1, 1])),
    }
    out = {}
    try:
        for name, (fam, img, kw) in spec.items():
            buf = oracle.encode(img, family=fam, **kw)
            lfmlib.set_family(fam)
            out[name] = (fam, img, buf, lfmlib.decode(buf))
        lfmlib.set_family("tiles")
        buf = zlib_file(oracle, small, [32, 32, 1, 1, 1])
        out["zlib"] = ("tiles", small, buf, lfmlib.decode(buf))
    finally:
        lfmlib.set_family("tiles")
    for name, (_, img, _, single) in out.items():
        assert np.array_equal(single, img), name
    return out


FARMED = ["video", "still_angle", "still_space", "default_tiles", "default_angle", "t3c2_video", "t3c2_space",
          "t1c3_video", "uint8", "half_constant"]


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("name", FARMED)
def test_exact_and_stats(lfmlib, oracle, files, name, n):
    """decode_multi equals the input and lfm.decode; workers, axis and the
    shards are the plan's; the shards' blocks sum to the header's block count
    (nothing decoded twice); every shard went through the pipeline on device 0
    straight into place (nothing staged) and the image came down once."""
    fam, img, buf, single = files[name]
    h = oracle.parse_header(buf)
    axis, plan = lfmlib.decode_shard_plan(buf, n)
    assert len(plan) >= 2, (name, n)
    lfmlib.set_family(fam)
    lfmlib.set_decode_devices([0] * n)
    got, st = lfmlib.decode_multi(buf, return_stats=True)
    print(name, n, st)
    assert got.dtype == img.dtype and np.array_equal(got, img)
    assert np.array_equal(got, single)
    assert st["workers"] == len(plan) and st["axis"] == axis, st
    shards = st["shards"]
    assert [(s["first"], s["count"]) for s in shards] == plan, st
    assert sum(s["stats"]["blocks"] for s in shards) == h["nb"] == st["blocks"], st
    for s in shards:
        assert s["rc"] == 0 and s["device"] == 0, st
        assert s["stats"]["staged_bytes"] == 0 and s["stats"]["path"] == 0 and s["stats"]["chunks"] >= 1, st
        assert s["stats"]["total_ms"] > 0, st
    assert st["d2h_bytes"] == img.nbytes == sum(s["stats"]["d2h_bytes"] for s in shards), st
    assert st["host_blocks"] == sum(s["stats"]["host_blocks"] for s in shards) <= st["blocks"], st
    if name == "half_constant":
        assert st["host_blocks"] == 16 and all(s["stats"]["host_blocks"] == 8 for s in shards), st


def host(t):
    import torch
    t = t.cpu()
    if t.dtype in (torch.uint16, torch.int16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


@pytest.mark.parametrize("name,n", [("video", 2), ("video", 5), ("t3c2_video", 3), ("t1c3_video", 2), ("uint8", 3),
                                    ("still_angle", 5)])
def test_device_destination(lfmlib, oracle, gpu, files, name, n):
    """decode_device_sharded: one CUDA tensor per shard, equal to the image's
    slice along the axis; no image byte comes down."""
    fam, img, buf, _ = files[name]
    axis, plan = lfmlib.decode_shard_plan(buf, n)
    lfmlib.set_family(fam)
    got_axis, parts, st = lfmlib.decode_device_sharded(buf, devices=[0] * n, return_stats=True)
    assert got_axis == axis and [f for f, _ in parts] == [f for f, _ in plan]
    assert st["workers"] == len(plan) >= 2 and st["d2h_bytes"] == 0, st
    assert st["blocks"] == oracle.parse_header(buf)["nb"], st
    for (first, t), (_, count), s in zip(parts, plan, st["shards"]):
        assert t.is_cuda and t.shape[4 - axis] == count
        sl = [slice(None)] * 5
        sl[4 - axis] = slice(first, first + count)
        assert np.array_equal(host(t), img[tuple(sl)]), (name, first)
        assert s["rc"] == 0 and s["device"] == 0 and s["stats"]["path"] == 0, st
        assert s["stats"]["staged_bytes"] == 0 and s["stats"]["d2h_bytes"] == 0, st
    # the same into tensors of the caller's (int16 stands in for uint16), full of 0x55
    outs = [gpu.full(tuple(t.shape), 0x55, dtype=gpu.int16 if t.dtype == gpu.uint16 else t.dtype, device="cuda")
            for _, t in parts]
    _, again = lfmlib.decode_device_sharded(buf, outs=outs)
    for (_, t), (_, want), o in zip(again, parts, outs):
        assert t.data_ptr() == o.data_ptr() and np.array_equal(host(t), host(want))


def test_device_destination_refusals(lfmlib, gpu, files):
    """A buffer one byte short returns 3; so does an nshards that is not the
    plan's count for that many workers (3 workers get 2 shards of this file)."""
    torch = gpu
    _, img, buf, _ = files["video"]
    assert lfmlib.decode_shard_plan(buf, 3) == (2, [(0, 12), (12, 8)])
    fn = lfmlib.lib().lfm_decode_memory_multi_device
    frame = img.shape[3] * img.shape[4] * 2
    bufs = [torch.empty(12 * frame, dtype=torch.uint8, device="cuda"), torch.empty(8 * frame, dtype=torch.uint8, device="cuda"),
            torch.empty(8 * frame, dtype=torch.uint8, device="cuda")]
    ptrs = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs])

    def call(nshards, sizes):
        return fn(buf, len(buf), ptrs, (ctypes.c_uint64 * 3)(*sizes), nshards, -1, None, None, 0)

    full = [12 * frame, 8 * frame, 8 * frame]
    assert call(3, full) == 3
    assert call(2, [full[0], full[1] - 1, 0]) == 3
    assert call(2, [full[0] - 1, full[1], 0]) == 3
    assert call(2, full) == 0
    got = np.concatenate([host(b[:s].view(torch.int16)) for b, s in zip(bufs[:2], full)])
    assert np.array_equal(got, img.reshape(-1))
    with pytest.raises(ValueError):
        lfmlib.decode_device_sharded(buf, outs=bufs)  # three tensors, two shards
    host_buf = np.empty(12 * frame, np.uint8)
    ptrs[0] = host_buf.ctypes.data
    assert call(2, full) == 3  # a host pointer


@pytest.mark.parametrize("name", ["none", "zlib", "nnum40", "one_unit"])
def test_not_farmed(lfmlib, oracle, files, name):
    """Three workers set, but the pipelined decode does not take the file (or it
    is one block layer): one plain decode, exact, workers == 1."""
    _, img, buf, _ = files[name]
    assert (len(lfmlib.decode_shard_plan(buf, 3)[1]) == 1) == (name == "one_unit")
    lfmlib.set_decode_devices([0, 0, 0])
    got, st = lfmlib.decode_multi(buf, return_stats=True)
    assert np.array_equal(got, img)
    assert st["workers"] == 1 and len(st["shards"]) == 1, st
    sh = st["shards"][0]
    assert (sh["first"], sh["count"], sh["rc"]) == (0, img.shape[2], 0), st
    assert sh["stats"]["path"] == (0 if name == "one_unit" else 1), st
    assert st["blocks"] == oracle.parse_header(buf)["nb"], st
    assert np.array_equal(lfmlib.decode(buf), img)  # the drop-in reader with the list set: the same rule


def test_corrupt_block_in_second_shard(lfmlib, oracle, files):
    """One bit of the stored block CRC (stream bytes 10-13) of a block of the
    second shard flipped: the Huffman decode runs normally, the comparison
    fails.  decode_multi fails with lfm.decode's status; the next decode on
    the same workers is exact."""
    _, img, buf, _ = files["video"]
    h = oracle.parse_header(buf)
    ends = [h["header_size"] + int(e) for e in h["offsets"]]
    begs = [h["header_size"]] + ends[:-1]
    victim = next(bid for bid, coord, _ in oracle.iter_blocks(h["xyzct"], h["block_size"]) if coord[2] == 15)
    bad = bytearray(buf)
    bad[begs[victim] + 12] ^= 0x10
    bad = bytes(bad)
    with pytest.raises(lfmlib.LfmError) as single:
        lfmlib.decode(bad)
    lfmlib.set_decode_devices([0, 0])
    assert lfmlib.decode_shard_plan(bad, 2)[1] == [(0, 12), (12, 8)]
    with pytest.raises(lfmlib.LfmError) as multi:
        lfmlib.decode_multi(bad)
    code = str(single.value).rsplit(" ", 1)[1]
    assert code != "0" and str(multi.value).rsplit(" ", 1)[1] == code, (single.value, multi.value)
    L = lfmlib.lib()
    out = np.empty(img.shape, np.uint16)
    st = lfmlib.DecodeMultiStats()
    sh = (lfmlib.DecodeShard * 2)()
    assert L.lfm_decode_memory_multi(bad, len(bad), out.ctypes.data, -1, ctypes.byref(st), sh, 2) == int(code)
    assert (sh[0].rc, sh[1].rc) == (0, int(code)) and st.workers == 2
    assert np.array_equal(out[0, 0, :12], img[0, 0, :12])  # the good shard is whole
    got, st = lfmlib.decode_multi(buf, return_stats=True)
    assert np.array_equal(got, img) and st["workers"] == 2


def test_readers_opt_in_through_env(lfmlib, files, tmp_path, monkeypatch):
    """LFM_DECODE_GPUS names three workers: the file readers and
    lfm_decode_memory farm, exactly; without it the list is empty again."""
    _, img, buf, _ = files["video"]
    p = tmp_path / "v.lfm"
    p.write_bytes(buf)
    monkeypatch.setenv("LFM_DECODE_GPUS", "0,0,0")
    try:
        assert lfmlib.get_decode_devices() == [0, 0, 0]
        got, hv, nnum = lfmlib.read_lfm(str(p))
        assert np.array_equal(got, img) and hv == 0x80 | 4 and nnum == 13
        assert np.array_equal(lfmlib.decode(buf), img)
        inplace = np.empty(img.shape, np.uint16)
        dt = ctypes.c_int()
        assert lfmlib.lib().readKLBstackInPlace(str(p).encode(), inplace.ctypes.data, ctypes.byref(dt), -1) == 0
        assert np.array_equal(inplace, img)
        _, st = lfmlib.decode_multi(buf, return_stats=True)
        assert st["workers"] == 2, st  # (3 workers: 2 shards of pairs of layers)
    finally:
        monkeypatch.delenv("LFM_DECODE_GPUS")
    assert lfmlib.get_decode_devices() == []
    assert lfmlib.decode_multi(buf, return_stats=True)[1]["workers"] == 1


def test_concurrent_calls(lfmlib, files):
    """Two threads call decode_multi at once, one on the list [0, 0] and one on
    [0, 0, 0] (they share two of the workers): both exact.  The list is
    process-wide and read when a call comes in: the first thread calls with
    [0, 0] in place, the second sets [0, 0, 0] and calls.  Which of the two
    lists the first call saw is not pinned, only that it ran one of them."""
    _, img, buf, _ = files["default_tiles"]
    counts = {len(lfmlib.decode_shard_plan(buf, n)[1]) for n in (2, 3)}
    assert counts == {2, 3}
    results = {}

    def run(key, devs):
        barrier.wait()
        if devs:
            lfmlib.set_decode_devices(devs)
        got, st = lfmlib.decode_multi(buf, return_stats=True)
        results[key] = (st["workers"], np.array_equal(got, img))

    for _ in range(4):
        lfmlib.set_decode_devices([0, 0])
        barrier = threading.Barrier(2)
        ts = [threading.Thread(target=run, args=("a", None)), threading.Thread(target=run, args=("b", [0, 0, 0]))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert results["a"][1] and results["b"][1], results
        assert results["a"][0] in counts and results["b"][0] == 3, results
        results.clear()


def test_buffers_are_reused(lfmlib, gpu, files):
    """The workers keep their device buffers: the device's free memory after
    the third decode on one list is not lower than after the second."""
    _, img, buf, _ = files["default_tiles"]
    lfmlib.set_decode_devices([0, 0, 0])
    free = []
    for _ in range(3):
        assert np.array_equal(lfmlib.decode_multi(buf), img)
        free.append(gpu.cuda.mem_get_info(0)[0])
    assert free[2] >= free[1], free
    lfmlib.release_decoders()
    assert gpu.cuda.mem_get_info(0)[0] > free[2], (free, "release_decoders frees the workers' buffers")
