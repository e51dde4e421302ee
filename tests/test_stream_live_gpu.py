"""Checkpoints, recovery and the live reader on the GPU: files of predicted
stacks appended from CUDA tensors and never closed are recovered to the bytes
of the one-shot encode of their complete layers, with every stream verified by
the GPU bzip2 decoder, and are read into device memory while the writer runs.
A "crashed" file is the copy of a flushed, still-open writer's file (see
test_stream_live_cpu.py); the stack is that of test_stream_gpu.py."""
import shutil
import struct

import numpy as np
import pytest

import bz2_parts
from test_stream_gpu import BS, NNUM, dev, host, read_file, stack  # noqa: F401  (stack: a fixture)

pytestmark = pytest.mark.gpu

FIXED = 320


def crashed(lfm, path, pieces, shape, committed, **kw):
    """A writer of `shape` takes `pieces`, is flushed (`committed` indices must
    be on file then) and aborted; what its file held is left at `path`."""
    live = path + ".open"
    w = lfm.Writer(live, shape, **kw)
    try:
        for p in pieces:
            w.append(p)
        assert w.flush() == committed
        shutil.copyfile(live, path)
    finally:
        w.abort()
    return path


def encode(lfm, torch, d, **kw):
    enc = lfm.Encoder(device=torch.cuda.current_device())
    try:
        return enc.encode(d[None, None], **kw)
    finally:
        enc.close()


@pytest.mark.parametrize("fam", ["tiles", "angle", "space"])
def test_recovery_per_family(lfmlib, gpu, stack, tmp_path, fam):
    """Auto selection, nine frames appended from the device, eight committed:
    the recovered file is Encoder.encode of those eight, all eight streams
    verified on the GPU."""
    a, d = stack
    lfmlib.set_family(fam)
    try:
        ref, ref_st = encode(lfmlib, gpu, d[:8], header_version=0, nnum=NNUM, block_size=BS)
        src = crashed(lfmlib, str(tmp_path / "c.lfm"), [d[:9]], a.shape, 8, predictor_request=0, nnum=NNUM,
                      block_size=BS)
        out = str(tmp_path / "o.lfm")
        st = lfmlib.recover(src, out=out, verify=True)
        assert read_file(out) == ref
        assert st["kept"] == 8 and st["dropped_layers"] == 0 and st["committed_blocks"] == 8, st
        assert st["verified_streams"] == 8 and st["host_streams"] == 0, st
        assert st["header_version"] == ref_st["header_version"] and ref_st["chosen"] != 0, (st, ref_st)
        back = lfmlib.read_lfm_device(out)
        assert np.array_equal(host(back)[0, 0], a[:8])
    finally:
        lfmlib.set_family("tiles")


def test_recovery_video_odd_extent(lfmlib, oracle, gpu, tmp_path):
    """Video stack, block depth 3, one frame per append: nine of ten frames are
    committed, and the ranges behind the first start at temporal frames."""
    a = oracle.synthetic_lf(64, 48, Z=10, T=NNUM, seed=0x4C464D43)[0, 0]
    d = dev(gpu, a)
    bs = [32, 32, 3, 1, 1]
    ref, ref_st = encode(lfmlib, gpu, d[:9], header_version=0x80, nnum=NNUM, block_size=bs)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [d[z] for z in range(10)], a.shape, 9, predictor_request=0,
                  video=1, nnum=NNUM, block_size=bs)
    st = lfmlib.recover(src, verify=True)
    assert read_file(src) == ref
    assert st["kept"] == 9 and st["header_version"] == ref_st["header_version"] >= 0x80, st
    assert st["verified_streams"] == 12 and st["host_streams"] == 0, st


def test_zeroed_stream_is_caught_on_the_gpu(lfmlib, gpu, stack, tmp_path):
    """The last stream of the second layer is zeros under an intact table:
    verification drops that layer without the host library's help."""
    a, d = stack
    ref4, _ = encode(lfmlib, gpu, d[:4], header_version=0, nnum=NNUM, block_size=BS)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [d[:8]], a.shape, 8, predictor_request=0, nnum=NNUM, block_size=BS)
    buf = bytearray(read_file(src))
    table = struct.unpack_from("<8Q", buf, FIXED)
    base = FIXED + 8 * 20
    buf[base + table[6]:base + table[7]] = bytes(table[7] - table[6])
    with open(src, "wb") as f:
        f.write(buf)
    st = lfmlib.recover(src, verify=True)
    assert st["kept"] == 4 and st["dropped_layers"] == 1 and st["host_streams"] == 0, st
    assert st["verified_streams"] == 8 and read_file(src) == ref4, st


def test_live_reads_into_device_memory(lfmlib, gpu, stack, tmp_path):
    """Append, flush, refresh and read alternate in one thread: each new layer
    lands in a device tensor through the pipelined GPU decode."""
    torch = gpu
    a, d = stack
    p = str(tmp_path / "live.lfm")
    w = lfmlib.Writer(p, a.shape, predictor_request=0, nnum=NNUM, block_size=BS)
    try:
        r = lfmlib.Reader(p, live=True)
        assert r.shape == (1, 1, 0, 48, 64)
        for k in (4, 8, 12):
            w.append(d[k - 4:k])
            assert w.flush() == k and r.refresh() == (1, 1, k, 48, 64)
            assert r.header_version & 0x7F != 0 and r.nnum == NNUM
            out = torch.empty((1, 1, 4, 48, 64), dtype=torch.int16, device="cuda")
            got, st = r.read([0, 0, k - 4, 0, 0], [63, 47, k - 1, 0, 0], out=out, return_stats=True)
            assert got.data_ptr() == out.data_ptr() and np.array_equal(host(got)[0, 0], a[k - 4:k])
            assert st["path"] == 0 and st["d2h_bytes"] == 0 and st["blocks"] == 4, st
        # x 20 .. 40 and y 30 .. 40 cross the block edge at 32, z 3 .. 9 two layer edges
        box, st = r.read([20, 30, 3, 0, 0], [40, 40, 9, 0, 0], device="cuda", return_stats=True)
        assert np.array_equal(host(box)[0, 0], a[3:10, 30:41, 20:41]) and st["path"] == 0, st
        with pytest.raises(lfmlib.LfmError, match="code 3"):
            r.read([0, 0, 12, 0, 0], [63, 47, 12, 0, 0], device="cuda")
        r.close()
    finally:
        w.abort()


def test_recovery_verifies_multiblock_streams(lfmlib, gpu, tmp_path):
    """95 000-byte rows of runs of four (test_bzip2_multiblock_gpu.py): every
    stream is two bzip2 blocks, written and verified on the device."""
    torch = gpu
    assert lfmlib.get_bzip2_multiblock() and lfmlib.get_bunzip2_multiblock()
    runs4 = np.repeat(np.arange(190000 // 4, dtype=np.uint32) % 251, 4)[:95000]
    img = np.stack([((runs4 + 7 * z) % 251).astype(np.uint8).reshape(1, 95000) for z in range(3)])
    assert all(len(bz2_parts.parts(img[z].tobytes(), 1)) == 2 for z in range(3))
    d = torch.from_numpy(img.copy()).cuda()
    bs = [95000, 1, 1, 1, 1]
    ref, _ = encode(lfmlib, torch, d[:2], header_version=8, nnum=13, block_size=bs)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [d[:2]], img.shape, 2, dtype=np.uint8, predictor_request=8,
                  block_size=bs)
    st = lfmlib.recover(src, verify=True)
    assert read_file(src) == ref
    assert st["kept"] == 2 and st["verified_streams"] == 2 and st["host_streams"] == 0, st
