"""Streaming on the GPU (lfm.Writer / lfm.Reader): predicted stacks appended
piece by piece from CUDA tensors or host arrays give the bytes of the one-shot
encode of the whole stack, and region reads of the file land in device memory
with only the needed streams fetched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 4, 3, 8, 1)
NNUM = 5
BS = [32, 32, 4, 1, 1]


def dev(torch, a):
    """numpy uint16 -> CUDA int16 tensor (torch has no uint16 arithmetic)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().view(__import__("torch").int16).numpy().view(np.uint16)


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def stream_z(lfm, path, frames, counts, hv, bs, capacity=None, zero_after=False, nnum=NNUM):
    """frames [z, y, x] (CUDA tensor or numpy) appended in `counts`; (bytes, stats)."""
    z, y, x = frames.shape
    w = lfm.Writer(path, (capacity or z, y, x), predictor_request=hv & 0x7F, video=hv >> 7, nnum=nnum, block_size=bs)
    at = 0
    for n in counts:
        piece = frames[at] if n == 1 else frames[at:at + n]
        if zero_after:
            piece = piece.clone()
        w.append(piece)
        if zero_after:
            piece.zero_()  # queued behind nothing the library still needs: append has finished reading
        at += n
    assert at == z
    st = w.close()
    return read_file(path), st


@pytest.fixture(scope="module")
def stack(oracle, gpu):
    """64 x 48 x 19 light field, lenslets of 5: (numpy [19, 48, 64], CUDA tensor)."""
    a = oracle.synthetic_lf(64, 48, Z=19, T=NNUM, seed=0x4C464D41)[0, 0]
    return a, dev(gpu, a)


@pytest.fixture(scope="module")
def one_shot(lfmlib, gpu, stack):
    """{family: (bytes, stats)} of Encoder.encode of the whole device stack, auto selection."""
    out = {}
    enc = lfmlib.Encoder(device=gpu.cuda.current_device())
    try:
        for fam in ("tiles", "angle", "space"):
            lfmlib.set_family(fam)
            out[fam] = enc.encode(stack[1][None, None], header_version=0, nnum=NNUM, block_size=BS)
    finally:
        enc.close()
        lfmlib.set_family("tiles")
    return out


@pytest.mark.parametrize("fam", ["tiles", "angle", "space"])
@pytest.mark.parametrize("where", ["device", "host"])
def test_predicted_auto_selection(lfmlib, gpu, stack, one_shot, tmp_path, fam, where):
    """Auto selection, appended as 1, 2, 4, 3, 8, 1: the one-shot's bytes and
    predictor.  Device appends are compressed on the GPU (host_streams == 0).
    Host appends of this size are not: the encoder hands a host image of at
    most 1 MiB to the host library by design (each range here is 12 to 24 KiB),
    as the one-shot encode of a host stack this small does; every stream is
    then a host stream."""
    ref, ref_st = one_shot[fam]
    lfmlib.set_family(fam)
    try:
        frames = stack[1] if where == "device" else stack[0]
        got, st = stream_z(lfmlib, str(tmp_path / "s.lfm"), frames, COUNTS, 0, BS)
    finally:
        lfmlib.set_family("tiles")
    assert got == ref
    assert st["chosen"] == ref_st["chosen"] and st["chosen"] != 0, (st, ref_st)
    assert st["header_version"] == ref_st["header_version"]
    assert np.allclose(st["entropy"], ref_st["entropy"], rtol=1e-6)
    assert st["ranges"] == 4 and st["streams"] == 2 * 2 * 5 and st["appended"] == 19, st
    assert st["staged_peak_bytes"] <= 3 * 64 * 48 * 2 and st["moved_bytes"] == 0, st
    if where == "device":
        assert st["host_streams"] == 0 and st["bzip2_blocks"] >= st["streams"], st
    else:
        assert st["host_streams"] == st["streams"], st


def test_capacity_not_reached_on_device(lfmlib, gpu, stack, one_shot, tmp_path):
    got, st = stream_z(lfmlib, str(tmp_path / "s.lfm"), stack[1], COUNTS, 0, BS, capacity=40)
    assert got == one_shot["tiles"][0]
    assert st["moved_bytes"] == len(got) - 320 - 8 * 20 and st["host_streams"] == 0, st


def test_selection_comes_from_frame_0_only(lfmlib, oracle, gpu, stack, tmp_path):
    """Frames 0-3 are the light field, frames 4-7 noise: frame 4 alone selects
    another predictor than frame 0 alone, and the second range (frames 4-7)
    must still be coded with frame 0's."""
    torch = gpu
    a = stack[0][:8].copy()
    a[4:] = np.random.default_rng(0x4C464D42).integers(0, 65535, size=a[4:].shape, dtype=np.uint16, endpoint=True)
    d = dev(torch, a)
    enc = lfmlib.Encoder(device=torch.cuda.current_device())
    try:
        _, st0 = enc.encode(d[0][None, None, None], header_version=0, nnum=NNUM, block_size=BS)
        _, st4 = enc.encode(d[4][None, None, None], header_version=0, nnum=NNUM, block_size=BS)
        assert st0["chosen"] != st4["chosen"], (st0["chosen"], st4["chosen"])
        ref, ref_st = enc.encode(d[None, None], header_version=0, nnum=NNUM, block_size=BS)
    finally:
        enc.close()
    assert ref_st["chosen"] == st0["chosen"]
    got, st = stream_z(lfmlib, str(tmp_path / "s.lfm"), d, (4, 4), 0, BS)
    assert got == ref and st["chosen"] == st0["chosen"] and st["ranges"] == 2


def test_video_odd_block_depth(lfmlib, oracle, gpu, tmp_path):
    """Video stack, block depth 3, one frame per append: the ranges start at
    z0 = 3 and 9 (temporal frames, predicted from the raw frame the writer
    kept) and at 6."""
    torch = gpu
    a = oracle.synthetic_lf(64, 48, Z=10, T=NNUM, seed=0x4C464D43)[0, 0]
    d = dev(torch, a)
    bs = [32, 32, 3, 1, 1]
    enc = lfmlib.Encoder(device=torch.cuda.current_device())
    try:
        ref, ref_st = enc.encode(d[None, None], header_version=0x80, nnum=NNUM, block_size=bs)
    finally:
        enc.close()
    assert ref_st["chosen"] != 0
    got, st = stream_z(lfmlib, str(tmp_path / "s.lfm"), d, (1,) * 10, 0x80, bs)
    assert got == ref
    assert st["ranges"] == 4 and st["header_version"] == ref_st["header_version"] and st["host_streams"] == 0, st
    assert st["staged_peak_bytes"] == 2 * 64 * 48 * 2
    assert np.array_equal(lfmlib.decode(got)[0, 0], a)
    got_h, _ = stream_z(lfmlib, str(tmp_path / "h.lfm"), a, (1,) * 10, 0x80, bs)
    assert got_h == ref


@pytest.fixture(scope="module")
def volumes(lfmlib, oracle, gpu, tmp_path_factory):
    """64 x 48 x 4 x 1 x 3 video stack streamed per volume from the device:
    (numpy [3, 1, 4, 48, 64], path of the streamed file, writer stats, write_lfm bytes)."""
    d = tmp_path_factory.mktemp("stream_t")
    a = oracle.synthetic_lf(64, 48, Z=4, Tn=3, T=NNUM, seed=0x4C464D44)
    lfmlib.set_family("tiles")
    lfmlib.write_lfm(str(d / "ref.lfm"), a, predictor_request=0, nnum=NNUM, video=1, block_size=BS)
    path = str(d / "s.lfm")
    dv = dev(gpu, a)
    with lfmlib.Writer(path, a.shape, predictor_request=0, video=1, nnum=NNUM, block_size=BS) as w:
        assert w.axis == 4
        for t in range(3):
            w.append(dv[t])
    return a, path, w.stats, read_file(str(d / "ref.lfm"))


def test_t_axis_per_volume(lfmlib, volumes):
    a, path, st, ref = volumes
    assert read_file(path) == ref
    assert st["ranges"] == 3 and st["chosen"] != 0 and st["host_streams"] == 0 and st["staged_peak_bytes"] == 0, st


def test_input_is_reusable_on_return(lfmlib, gpu, stack, one_shot, tmp_path):
    got, _ = stream_z(lfmlib, str(tmp_path / "s.lfm"), stack[1], COUNTS, 0, BS, zero_after=True)
    assert got == one_shot["tiles"][0]


def test_mixing_host_and_device_appends(lfmlib, gpu, stack, tmp_path):
    path = str(tmp_path / "s.lfm")
    w = lfmlib.Writer(path, stack[0].shape, predictor_request=0, nnum=NNUM, block_size=BS)
    w.append(stack[1][:4])
    with pytest.raises(lfmlib.LfmError, match="code 3"):
        w.append(stack[0][4:8])
    w.abort()
    w = lfmlib.Writer(path, stack[0].shape, predictor_request=0, nnum=NNUM, block_size=BS)
    w.append(stack[0][:4])
    with pytest.raises(lfmlib.LfmError, match="code 3"):
        w.append(stack[1][4:8])
    w.abort()


def test_reader_to_device(lfmlib, gpu, volumes):
    torch = gpu
    a, path, _, ref = volumes
    whole = lfmlib.decode_device(ref)
    assert np.array_equal(host(whole), a)
    hbytes = 320 + 8 * (2 * 2 * 1 * 1 * 3)
    with lfmlib.Reader(path) as r:
        assert r.shape == a.shape and r.header_version & 0x80 and r.nnum == NNUM and r.file_bytes == len(ref)
        assert r.bytes_read == hbytes
        last, st = r.read([0, 0, 0, 0, 2], [63, 47, 3, 0, 2], device="cuda", return_stats=True)
        assert last.is_cuda and torch.equal(last.view(torch.int16), whole[2:3].view(torch.int16))
        assert st["d2h_bytes"] == 0 and st["path"] == 0 and st["blocks"] == 4, st
        assert 0 < r.bytes_read - hbytes < r.file_bytes - hbytes
        ends = np.frombuffer(ref, dtype="<u8", count=12, offset=320)
        assert r.bytes_read - hbytes == int(ends[11] - ends[7])
        # x 20 .. 40 and y 30 .. 40 cross the block edge at 32; z 1 .. 2 starts at a temporal frame
        lb, ub = [20, 30, 1, 0, 1], [40, 40, 2, 0, 2]
        out = torch.empty((2, 1, 2, 11, 21), dtype=torch.int16, device="cuda")
        box, st = r.read(lb, ub, out=out, return_stats=True)
        want = whole[1:3, :, 1:3, 30:41, 20:41].view(torch.int16)
        assert box.data_ptr() == out.data_ptr() and torch.equal(box.view(torch.int16), want)
        assert st["d2h_bytes"] == 0 and st["staged_bytes"] > 0, st
        assert np.array_equal(r.read(lb, ub), host(want))
        assert np.array_equal(r.read([0, 0, 0, 0, 2], [63, 47, 3, 0, 2]), a[2:3])
