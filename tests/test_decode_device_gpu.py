"""Device-destination decode (lfm.decode_device, lfm.decode_roi_device,
lfm.crop_device; lfm_decode_memory_device / lfm_decode_memory_roi_device /
lfm_hip_crop_region): .lfm bytes -> torch CUDA tensor, bit-exact against the
input, with the lfm_decode_stats of every call checked (path 0: the pipelined
GPU decode wrote the tensor and no image byte came down; path 1: host decode
and one upload)."""
import ctypes

import numpy as np
import pytest

import bz2_craft as C

pytestmark = pytest.mark.gpu

FAMS = ("tiles", "angle", "space")


def dev(torch, a):
    """numpy uint16 -> CUDA int16 tensor (torch has no uint16 arithmetic)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def host(t):
    """CUDA tensor -> numpy, uint16 for the 2-byte integer types."""
    import torch
    t = t.cpu()
    if t.dtype in (torch.uint16, torch.int16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def pipelined(st, chunks_at_least=1):
    assert st["path"] == 0 and st["d2h_bytes"] == 0 and st["chunks"] >= chunks_at_least, st
    assert st["total_ms"] > 0 and st["host_blocks"] <= st["blocks"], st


@pytest.fixture(scope="module")
def files(lfmlib, oracle, gpu):
    """The stacks of cases 1 and 2 and their .lfm bytes, encoded once from CUDA
    tensors: {name: (family, numpy [1, 1, z, y, x], device tensor, bytes, block size)}."""
    torch = gpu
    out = {}
    stack = oracle.synthetic_lf(150, 110, Z=6, T=13, seed=0x4C464D21)
    bs = [32, 24, 2, 1, 1]
    enc = lfmlib.Encoder(device=torch.cuda.current_device())
    try:
        for fam in FAMS:
            lfmlib.set_family(fam)
            d = dev(torch, stack)
            b, _ = enc.encode(d, header_version=8 + 4, nnum=13, block_size=bs)
            out[fam] = (fam, stack, d, b, bs)
        # tiles video stack: 5 slabs of 9 blocks in chunks of 3 + 2, so chunk 1
        # starts at the temporal frame 3
        lfmlib.set_family("tiles")
        vid = oracle.synthetic_lf(70, 90, Z=5, T=2, seed=0x4C464D22)
        d = dev(torch, vid)
        vbs = [32, 32, 1, 1, 1]
        b, _ = enc.encode(d, header_version=0x80 | (8 + 4), nnum=2, block_size=vbs)
        out["video"] = ("tiles", vid, d, b, vbs)
    finally:
        enc.close()
        lfmlib.set_family("tiles")
    return out


@pytest.mark.parametrize("fam", FAMS)
def test_roundtrip_on_device(lfmlib, oracle, gpu, files, fam):
    """Device stack -> .lfm -> device stack for the three families: equal to
    the input tensor, decoded by the pipeline in two chunks (3 z-slabs of 25
    blocks) with nothing copied down; the bytes are the oracle's and the host
    reader gives the same pixels."""
    torch = gpu
    _, stack, d, buf, bs = files[fam]
    lfmlib.set_family(fam)
    try:
        got, st = lfmlib.decode_device(buf, return_stats=True)
        assert got.dtype == torch.uint16 and tuple(got.shape) == stack.shape and got.is_cuda
        assert torch.equal(got.view(torch.int16), d)
        pipelined(st, 2)
        assert st["blocks"] == 75 and st["staged_bytes"] == 0, st
        assert buf == oracle.encode(stack, header_version=8 + 4, nnum=13, family=fam, block_size=bs)
        assert np.array_equal(lfmlib.decode(buf), host(d))
    finally:
        lfmlib.set_family("tiles")


def test_temporal_frame_at_chunk_start(lfmlib, oracle, gpu, files):
    """The first frame of chunk 1 (frame 3, temporal) reads frame 2 from the
    caller's buffer: exact, into a fresh tensor and into a preallocated int16
    tensor full of 0x5555."""
    torch = gpu
    _, vid, d, buf, _ = files["video"]
    h = oracle.parse_header(buf)
    assert h["header_version"] == 0x80 | 4 and h["nb"] == 45
    got, st = lfmlib.decode_device(buf, return_stats=True)
    assert torch.equal(got.view(torch.int16), d)
    pipelined(st, 2)
    assert st["chunks"] == 2 and st["blocks"] == 45, st
    out = torch.full(vid.shape, 0x5555, dtype=torch.int16, device="cuda")
    ret, st = lfmlib.decode_device(buf, out=out, return_stats=True)
    assert ret.data_ptr() == out.data_ptr() and ret.dtype == torch.int16
    assert torch.equal(out, d)
    pipelined(st, 2)


def test_unpredicted_and_host_library_blocks(lfmlib, oracle, gpu):
    """Half constant (0x0201, periodic: flagged for the host library), half
    noise, predictor 0: the scatter writes the caller's tensor; 16 of the 32
    streams go through decompress_one.  Both CRC fields of a noise block
    changed: rc 2."""
    torch = gpu
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
    got, st = lfmlib.decode_device(buf, return_stats=True)
    assert np.array_equal(host(got)[0, 0], img)
    pipelined(st, 2)
    assert st["host_blocks"] == 16 and st["blocks"] == 32, st
    ends = [h["header_size"] + int(e) for e in h["offsets"]]
    begs = [h["header_size"]] + ends[:-1]
    victim = const.index(False)
    stream = buf[begs[victim]:ends[victim]]
    twin = C.set_crcs(stream, C.parse(stream)["crc"] ^ 1)
    assert len(twin) == len(stream)
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.decode_device(buf[:begs[victim]] + twin + buf[ends[victim]:])


def test_auto_predictor_5d(lfmlib, oracle, gpu):
    """[t=2, c=1, z=4, y=64, x=96], auto-selected predictor, Nnum 15, angle."""
    torch = gpu
    img = oracle.synthetic_lf(96, 64, Z=4, C=1, Tn=2, T=15, seed=0x4C464D23)
    assert img.shape == (2, 1, 4, 64, 96)
    lfmlib.set_family("angle")
    enc = lfmlib.Encoder(device=torch.cuda.current_device())
    try:
        d = dev(torch, img)
        buf, est = enc.encode(d, header_version=0, nnum=15)
        assert est["chosen"] != 0  # (a predicted file: the inverse predictor writes the tensor)
        got, st = lfmlib.decode_device(buf, return_stats=True)
        assert tuple(got.shape) == img.shape and torch.equal(got.view(torch.int16), d)
        pipelined(st)
    finally:
        enc.close()
        lfmlib.set_family("tiles")


@pytest.fixture(scope="module")
def fallback_files(lfmlib, oracle, gpu):
    """{name: (numpy [z, y, x], .lfm bytes, expected path)}; the ZLIB files come
    from the library's own writer (the oracle writes NONE and BZIP2)."""
    rng = np.random.default_rng(31)
    u16 = oracle.synthetic_lf(80, 80, Z=2, T=13, seed=0x4C464D24)[0, 0]
    u8 = rng.integers(0, 7, (3, 33, 50), dtype=np.uint8)
    f32 = rng.standard_normal((2, 17, 40)).astype(np.float32)
    enc = lfmlib.Encoder(device=gpu.cuda.current_device())
    try:
        zlib16 = enc.encode(u16, header_version=8 + 4, nnum=13, compression=2)[0]
        zlib8 = enc.encode(u8, compression=2, block_size=[16, 16, 2, 1, 1])[0]
    finally:
        enc.close()
    assert oracle.parse_header(zlib16)["compression"] == 2 and oracle.parse_header(zlib8)["data_type"] == 0
    return {
        "none": (u16, oracle.encode(u16, header_version=8 + 4, nnum=13, compression=0), 1),
        "zlib": (u16, zlib16, 1),
        "uint8": (u8, zlib8, 1),
        "float32": (f32, oracle.encode(f32, compression=0, data_type=8, block_size=[16, 16, 1, 1, 1]), 1),
        "nnum40": (u16, oracle.encode(u16, header_version=8 + 4, nnum=40, block_size=[32, 32, 1, 1, 1]), 1),
        # the same two types as bzip2 files are the pipeline's (unpredicted: the scatter writes the tensor)
        "uint8_bzip2": (u8, oracle.encode(u8, data_type=0, block_size=[16, 16, 2, 1, 1]), 0),
        "float32_bzip2": (f32, oracle.encode(f32, data_type=8, block_size=[16, 16, 1, 1, 1]), 0),
    }


@pytest.mark.parametrize("name", ["none", "zlib", "uint8", "float32", "nnum40", "uint8_bzip2", "float32_bzip2"])
def test_fallback_path(lfmlib, gpu, fallback_files, name):
    """Files the pipelined decode does not take are decoded on the host and
    uploaded with one copy (path 1), exactly; tensors come in the file's dtype."""
    img, buf, path = fallback_files[name]
    got, st = lfmlib.decode_device(buf, return_stats=True)
    assert str(got.dtype) == "torch." + str(img.dtype)
    assert tuple(got.shape) == (1, 1) + img.shape
    assert np.array_equal(host(got)[0, 0], img)
    assert st["path"] == path and st["staged_bytes"] == 0, st
    if path == 0:
        pipelined(st)
    else:
        assert st["chunks"] == 0 and st["blocks"] == st["host_blocks"] > 0, st


@pytest.mark.parametrize("name", ["tiles", "angle", "space", "video"])
def test_regions(lfmlib, oracle, gpu, files, name):
    """decode_roi_device equals the slice of the input tensor: six random
    regions per file, the whole image, one pixel, an exact block box (decoded
    straight into the tensor: nothing staged) and, on the video file, a region
    that starts at an odd z.  Nothing comes down; a buffer one byte short is
    refused with 3."""
    torch = gpu
    fam, stack, d, buf, bs = files[name]
    dims = [stack.shape[4], stack.shape[3], stack.shape[2], 1, 1]
    rng = np.random.default_rng(77 + len(name))
    regions = []
    for _ in range(6):
        lb, ub = [], []
        for n in dims:
            a, b = sorted(int(v) for v in rng.integers(0, n, size=2))
            lb.append(a)
            ub.append(b)
        regions.append((lb, ub, None))
    regions.append(([0] * 5, [n - 1 for n in dims], None))
    regions.append(([dims[0] // 2 + 1, dims[1] // 3, dims[2] - 1, 0, 0], [dims[0] // 2 + 1, dims[1] // 3, dims[2] - 1, 0, 0],
                    None))
    regions.append(([0, 0, 2, 0, 0], [bs[0] - 1, bs[1] - 1, 2 + bs[2] - 1, 0, 0], True))  # blocks (0, 0, 2 / bs[2])
    if name == "video":
        regions.append(([5, 40, 3, 0, 0], [60, 77, 4, 0, 0], False))
    lfmlib.set_family(fam)
    try:
        for lb, ub, exact in regions:
            got, st = lfmlib.decode_roi_device(buf, lb, ub, return_stats=True)
            want = d[lb[4]:ub[4] + 1, lb[3]:ub[3] + 1, lb[2]:ub[2] + 1, lb[1]:ub[1] + 1, lb[0]:ub[0] + 1]
            assert got.shape == want.shape and torch.equal(got.view(torch.int16), want), (name, lb, ub)
            pipelined(st)
            if exact is True:
                assert st["staged_bytes"] == 0, (name, lb, ub, st)
            if exact is False:
                assert st["staged_bytes"] > 0, (name, lb, ub, st)
        lb, ub = [3, 2, 1, 0, 0], [40, 30, 2, 0, 0]
        need = 38 * 29 * 2 * 2
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        fn = lfmlib.lib().lfm_decode_memory_roi_device
        u5 = ctypes.c_uint32 * 5
        assert fn(buf, len(buf), u5(*lb), u5(*ub), out.data_ptr(), need - 1, -1, None) == 3
        assert fn(buf, len(buf), u5(*lb), u5(*ub), out.data_ptr(), need, -1, None) == 0
        want = d[0:1, 0:1, 1:3, 2:31, 3:41].contiguous()
        assert torch.equal(out.view(torch.int16).view(want.shape), want)
    finally:
        lfmlib.set_family("tiles")


@pytest.fixture(scope="module")
def crop_sources(gpu):
    """Random bytes as [t=2, c=2, z=3, y=7, x=67 * bpp] for each bpp (one draw,
    cut to size) and one long row source, x = 70000 at bpp 1."""
    torch = gpu
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (2, 2, 3, 7, 67 * 8), dtype=np.uint8)
    long_ = rng.integers(0, 256, (1, 2, 1, 2, 70000), dtype=np.uint8)
    return small, long_, torch.from_numpy(long_).cuda()


def run_crop(lfmlib, torch, src_bytes, d_src, bpp, lb, n):
    """crop_device on the uint8 array [t, c, z, y, x * bpp] against the numpy slice."""
    t, c, z, y, xb = src_bytes.shape
    dims = [xb // bpp, y, z, c, t]
    typed = src_bytes.view("<u%d" % bpp)
    want = typed[lb[4]:lb[4] + n[4], lb[3]:lb[3] + n[3], lb[2]:lb[2] + n[2], lb[1]:lb[1] + n[1], lb[0]:lb[0] + n[0]]
    dst = torch.full((int(np.prod(n)) * bpp + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    lfmlib.crop_device(d_src, dims, lb, n, bpp, dst[16:])
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:16] == 0xA5).all() and (got[-16:] == 0xA5).all(), (bpp, lb, n, "wrote outside the destination")
    assert np.array_equal(got[16:-16].view("<u%d" % bpp).reshape(want.shape), want), (bpp, lb, n)


@pytest.mark.parametrize("bpp", [1, 2, 4, 8])
def test_crop_device(lfmlib, gpu, crop_sources, bpp):
    """lfm_hip_crop_region alone: an odd lb[0], n[0] == 1, the identity box, a
    box whose rows start on 16-byte boundaries on both sides at every bpp, and
    at bpp 1 a source row longer than 4096 * 16 bytes cropped from lb[0] = 3
    (byte accesses), from lb[0] = 16 (16-byte accesses, several slices per row)
    and with a ragged end.  A box that leaves the image raises."""
    torch = gpu
    small, long_, d_long = crop_sources
    src = np.ascontiguousarray(small[..., :67 * bpp])
    d_src = torch.from_numpy(src).cuda()
    for lb, n in (([5, 1, 1, 0, 1], [33, 4, 2, 2, 1]),
                  ([66, 0, 0, 0, 0], [1, 7, 3, 2, 2]),
                  ([0, 0, 0, 0, 0], [67, 7, 3, 2, 2]),
                  ([16, 2, 0, 1, 0], [32, 5, 3, 1, 2]),
                  ([3, 6, 2, 1, 1], [64, 1, 1, 1, 1])):
        run_crop(lfmlib, torch, src, d_src, bpp, lb, n)
    if bpp == 1:
        for lb0, n0 in ((3, 69990), (16, 69984), (16, 69971), (0, 70000)):
            run_crop(lfmlib, torch, long_, d_long, 1, [lb0, 0, 0, 0, 0], [n0, 2, 1, 2, 1])
    dst = torch.empty(67 * 8 * 7 * 3 * 2 * 2, dtype=torch.uint8, device="cuda")
    for lb, n in (([60, 0, 0, 0, 0], [8, 1, 1, 1, 1]), ([0, 0, 3, 0, 0], [1, 1, 1, 1, 1]),
                  ([0, 0, 0, 0, 0], [0, 1, 1, 1, 1]), ([0, 0, 0, 0, 1], [1, 1, 1, 1, 2])):
        with pytest.raises(lfmlib.LfmError):
            lfmlib.crop_device(d_src, [67, 7, 3, 2, 2], lb, n, bpp, dst)
    with pytest.raises(lfmlib.LfmError):
        lfmlib.crop_device(d_src, [67, 7, 3, 2, 2], [0] * 5, [1] * 5, 3, dst)


@pytest.mark.parametrize("predicted", [True, False])
def test_ordering(lfmlib, oracle, gpu, files, predicted):
    """`out` is still being written on the null stream (a 256 MB tensor bumped
    200 times, then copied into it) when decode_device is called, with no
    synchronisation; a second non-blocking stream reads it as soon as the call
    returns.  The library's writes must come after the fill and be complete on
    return: the reader sees the decoded image.  Predicted file: the first
    writer is the inverse predictor; unpredicted: the scatter on the slot
    stream.  (A build without the waits loses the image to the fill here when
    the slot streams and the null stream sit on different hardware queues;
    measured 11 ms of fill against a 2.8 ms decode.)"""
    torch = gpu
    _, stack, d, buf, bs = files["tiles"]
    if not predicted:
        buf = oracle.encode(stack, header_version=8, nnum=13, block_size=bs)  # request 8: predictor 0 forced
        assert oracle.parse_header(buf)["header_version"] == 0
    out = torch.empty(stack.shape, dtype=torch.int16, device="cuda")
    big = torch.full((128 << 20,), 0x5555, dtype=torch.int16, device="cuda")
    assert big.numel() * big.element_size() >= 256 << 20
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(200):
        big.add_(1)
    out.copy_(big[:out.numel()].view(out.shape))
    ret, st = lfmlib.decode_device(buf, out=out, return_stats=True)
    with torch.cuda.stream(side):
        seen = out.clone()
    side.synchronize()
    pipelined(st, 2)
    assert torch.equal(seen, d)
    torch.cuda.synchronize()
    assert torch.equal(out, d) and int(big[0]) == 0x5555 + 200


def test_errors(lfmlib, oracle, gpu, files):
    """Bad destinations and buffers raise ValueError / LfmError; a host pointer
    handed to the C function returns 3."""
    torch = gpu
    _, stack, d, buf, _ = files["tiles"]
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_device(buf, out=np.empty(stack.shape, np.uint16))
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_device(buf, out=torch.empty(stack.size - 1, dtype=torch.int16, device="cuda"))
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_device(buf, out=torch.empty(stack.shape, dtype=torch.float16, device="cuda"))
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_device(buf, out=torch.empty(stack.shape, dtype=torch.int16, device="cuda").transpose(3, 4))
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_device(buf[:10])
    with pytest.raises((ValueError, lfmlib.LfmError)):
        lfmlib.decode_roi_device(buf, [0] * 5, [150, 0, 0, 0, 0])
    himg = np.empty(stack.shape, np.uint16)
    st = lfmlib.DecodeStats()
    fn = lfmlib.lib().lfm_decode_memory_device
    assert fn(buf, len(buf), himg.ctypes.data, himg.nbytes, -1, ctypes.byref(st)) == 3
    pinned = torch.empty(stack.shape, dtype=torch.int16).pin_memory()
    assert fn(buf, len(buf), pinned.data_ptr(), himg.nbytes, -1, None) == 3
    good = torch.empty(stack.shape, dtype=torch.int16, device="cuda")
    assert fn(buf, len(buf), good.data_ptr(), himg.nbytes - 1, -1, None) == 3
    assert fn(buf, len(buf), good.data_ptr(), himg.nbytes, -1, None) == 0
    assert torch.equal(good, d)


@pytest.mark.parametrize("env,path", [("LFM_GPU_BUNZIP2=0", 1), ("LFM_GPU_DECODE=0", 1), ("LFM_DECODE_KEEP=0", 0),
                                      ("LFM_DECODE_CHUNK_BLOCKS=1 LFM_DECODE_SLOTS=3", 0)])
def test_switches(lfmlib, gpu, files, tmp_path, env, path):
    """The decode's switches with a device destination: the GPU stages off ->
    host decode + upload (path 1); buffers released after every call (the
    region read's sub-image must outlive its decode) and one slab per chunk on
    three slots -> path 0.  Whole video stack and a region of it that is no
    block box, exact either way.  The switches are read once per process: each
    variant runs in its own child process (one GPU process at a time)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import PKG
    _, vid, d, buf, _ = files["video"]
    p = tmp_path / "sw.lfm"
    p.write_bytes(buf)
    code = ("import sys, json; sys.path.insert(0, %r); import torch, lfm; buf = open(%r, 'rb').read(); "
            "a, sa = lfm.decode_device(buf, return_stats=True); "
            "b, sb = lfm.decode_roi_device(buf, [5, 40, 3, 0, 0], [60, 77, 4, 0, 0], return_stats=True); "
            "b2 = lfm.decode_roi_device(buf, [5, 40, 3, 0, 0], [60, 77, 4, 0, 0]); "
            "torch.save([t.view(torch.int16).cpu() for t in (a, b, b2)], %r); print(json.dumps([sa, sb]))"
            % (PKG, str(p), str(tmp_path / "out.pt")))
    child_env = dict(os.environ)
    child_env.update(kv.split("=", 1) for kv in env.split())
    r = subprocess.run([sys.executable, "-c", code], env=child_env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    sa, sb = json.loads(r.stdout.strip().splitlines()[-1])
    a, b, b2 = gpu.load(str(tmp_path / "out.pt"))
    want = d.cpu()
    assert gpu.equal(a.view(gpu.int16), want), env
    for got in (b, b2):
        assert gpu.equal(got.view(gpu.int16), want[:, :, 3:5, 40:78, 5:61]), env
    assert sa["path"] == path and sb["path"] == path, (env, sa, sb)
    assert sa["staged_bytes"] == 0 and sb["staged_bytes"] > 0, (env, sa, sb)
    if path == 0:
        assert sa["d2h_bytes"] == 0 and sb["d2h_bytes"] == 0, (env, sa, sb)
    if "CHUNK_BLOCKS=1" in env:
        assert sa["chunks"] == 5, (env, sa)


def test_read_lfm_device(lfmlib, gpu, files, tmp_path):
    torch = gpu
    _, stack, d, buf, _ = files["tiles"]
    p = tmp_path / "dev.lfm"
    p.write_bytes(buf)
    got = lfmlib.read_lfm_device(str(p), device="cuda:0")
    assert torch.equal(got.view(torch.int16), d)
