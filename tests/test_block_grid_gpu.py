"""The block grid on the GPU: gather_blocks and the image-direct rle1_crc of
the bzip2 encoder, scatter_blocks / scatter_blocks16 of the decoder, over the
geometries of tests/block_grid_cases.py (5-D blocks ragged in every dimension,
FDiv divisors that need their correction, row and unit counts on both sides of
the kernels' loop strides, multi-block streams, sub-ranges of the grid).

The encoder's streams must be the reference library's for the blocks
oracle.gather_block cuts, with no stream handed to the host; the scatter must
rebuild the image and touch nothing else.  No test sees which kernel ran:
test_block_grid_cases_cpu.py pins the launchers' predicates, and here both
sides of each give the same bytes."""
import functools
import time

import numpy as np
import pytest

import block_grid_cases as G

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
# bytes kept behind an image the encoder reads (part of the allocation, so a
# row index one too large still reads memory that is there)
SLACK = 65536
SINGLE = [c for c in G.CASES if not c.multi]
NOT_HUGE = [c for c in G.CASES if c.name != "huge"]


def ref_bz2(oracle, data, level):
    """BZ2_bzBuffToBuffCompress(level, 0, 30) of the reference's bzip2-1.0.6
    (oracle/_ref/libbz2_ref.so, as in tests/test_gpu.py)."""
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz.compress(bytes(data), level)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(image, every block's bytes) of a case, built once for all tests."""
    case = G.BY_NAME[name]
    img = G.make_image(case)
    img.setflags(write=False)
    return img, G.expected_blocks(case, img)


def place(torch, nbytes, off, fill, head=GUARD, tail=GUARD):
    """A device byte buffer and the offset lo in it of a region of nbytes that
    starts `off` bytes past a 256-byte aligned address, with at least `head`
    bytes in front and `tail` behind, everything set to `fill`."""
    buf = torch.full((head + 256 + off + nbytes + tail,), fill, dtype=torch.uint8, device="cuda")
    lo = head + (-(buf.data_ptr() + head)) % 256 + off
    assert (buf.data_ptr() + lo - off) % 256 == 0 and lo + nbytes + tail <= buf.numel()
    return buf, lo


def upload(torch, case, img):
    """The image on the device at the case's base offset: (keep-alive, view)."""
    raw = np.ascontiguousarray(img).view(np.uint8).reshape(-1)
    buf, lo = place(torch, raw.size, case.base_off, 0, head=0, tail=SLACK)
    view = buf[lo:lo + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 256 == case.base_off
    return buf, view


def explain(oracle, case, bid, got, want_raw):
    """Why stream bid is not the reference's: the address of the first byte its
    decoded block differs in."""
    try:
        raw = oracle.bzip2().decompress(got, case.block_bytes + 64)
    except RuntimeError as e:
        return "%s: stream of block %d does not decode (%s)" % (case.name, bid, e)
    d = G.first_difference(case, bid, raw, want_raw)
    if d is None:
        return "%s: stream of block %d decodes to the right block but is not the reference's stream" % (case.name, bid)
    return ("%(name)s: block %(block)d differs first at byte %(byte)d = row %(row)d, column %(col)d "
            "(t %(t)d, c %(c)d, z %(z)d, y %(y)d, x %(x)d): got %(got)s, want %(want)s; %(got_len)d bytes, want "
            "%(want_len)d" % dict(d, name=case.name))


def encode_and_compare(torch, lfmlib, oracle, case):
    img, blocks = case_data(case.name)
    first, count = case.span
    keep, d_img = upload(torch, case, img)
    assert G.from_img(case, d_img.data_ptr()) == case.from_img
    got, flags = lfmlib.bzip2_device(d_img, list(case.dims), list(case.bs), case.bpp, level=case.level,
                                     first=first, count=count, multi=case.multi)
    assert len(got) == count
    assert not any(flags), "%s: streams %s handed to the host" % (case.name, [first + i for i, f in enumerate(flags) if f])
    for i in range(count):
        if got[i] != ref_bz2(oracle, blocks[first + i], case.level):
            pytest.fail(explain(oracle, case, first + i, got[i], blocks[first + i]))
    del keep
    return got


@pytest.mark.parametrize("case", NOT_HUGE, ids=[c.name for c in NOT_HUGE])
def test_encoder_streams(lfmlib, oracle, gpu, case):
    """bzip2_device over the case's span: every stream is the reference
    library's for the block the oracle gathers, none goes to the host."""
    encode_and_compare(gpu, lfmlib, oracle, case)


def test_encoder_huge_block(lfmlib, oracle, gpu):
    """A block of 8 848 784 bytes (>= 2^23: FDiv divides by integer division
    for its upper offsets, by float below them with row bytes 656 and extents
    41 and 47, which all need the +1) and a second stream of 16-byte rows, at
    level 9 through the multi-block entry.  Wall time on an MI355X: 0.6 s,
    the reference compressor on the host included."""
    t0 = time.perf_counter()
    encode_and_compare(gpu, lfmlib, oracle, G.BY_NAME["huge"])
    print("huge: %.2f s" % (time.perf_counter() - t0))


def scatter_and_check(torch, lfmlib, case, blocks, boff=0, ioff=0, spad=0):
    """Scatter `blocks` (the bytes of the span's blocks) at stride block_bytes +
    spad from a buffer boff bytes off alignment into an image ioff bytes further
    off than the case's own base_off; the image and both guards are checked."""
    img, _ = case_data(case.name)
    first, count = case.span
    assert len(blocks) == count
    stride = case.block_bytes + spad
    host = np.full(count * stride, 0x3C, dtype=np.uint8)
    for i, b in enumerate(blocks):
        host[i * stride:i * stride + len(b)] = np.frombuffer(b, dtype=np.uint8)
    bbuf, blo = place(torch, host.size, boff, 0x3C, head=0, tail=0)
    bbuf[blo:blo + host.size].copy_(torch.from_numpy(host))
    n = case.image_bytes
    ibuf, ilo = place(torch, n, case.base_off + ioff, FILL)
    p_blocks, p_img = bbuf.data_ptr() + blo, ibuf.data_ptr() + ilo
    assert G.v16(case, p_blocks, p_img, stride) == (case.v16 and not (boff or ioff or spad))
    lfmlib.scatter_blocks_device(p_blocks, stride, first, count, list(case.dims), list(case.bs), case.bpp, p_img)
    torch.cuda.synchronize()
    back = ibuf.cpu().numpy()
    assert (back[:ilo] == FILL).all(), "%s: bytes in front of the image written" % case.name
    assert (back[ilo + n:] == FILL).all(), "%s: bytes behind the image written" % case.name
    want = G.scattered_image(case, img, FILL)
    got = back[ilo:ilo + n].reshape(want.shape)
    if not np.array_equal(got, want):
        t, c, z, y, col = [int(v[0]) for v in np.nonzero(got != want)]
        pytest.fail("%s: image differs first at t %d, c %d, z %d, y %d, byte %d of the row: got %d, want %d; "
                    "%d bytes differ" % (case.name, t, c, z, y, col, got[t, c, z, y, col], want[t, c, z, y, col],
                                         int((got != want).sum())))


@pytest.mark.parametrize("case", SINGLE, ids=[c.name for c in SINGLE])
def test_scatter(lfmlib, gpu, case):
    """scatter_blocks_device of the expected blocks into an image of 0xA5
    between two 4 KiB guards: the image is make_image's (outside a sub-range
    still 0xA5), the guards are untouched."""
    _, blocks = case_data(case.name)
    first, count = case.span
    scatter_and_check(gpu, lfmlib, case, blocks[first:first + count])


@pytest.mark.parametrize("boff,ioff,spad", [(8, 0, 0), (0, 2, 0), (0, 0, 8)], ids=["blocks+8", "image+2", "stride+8"])
def test_scatter_byte_kernel_reasons(lfmlib, gpu, boff, ioff, spad):
    """img-5d, which scatters in 16-byte units, with the one thing changed that
    sends it to the byte kernel: the same image."""
    case = G.BY_NAME["img-5d"]
    assert case.v16
    scatter_and_check(gpu, lfmlib, case, case_data(case.name)[1], boff, ioff, spad)


@pytest.mark.parametrize("name", ["img-5d", "gather-dims"])
def test_encode_decode_scatter_round_trip(lfmlib, oracle, gpu, name):
    """The GPU's own streams decoded by bunzip2_device and scattered back give
    the input image."""
    case = G.BY_NAME[name]
    streams = encode_and_compare(gpu, lfmlib, oracle, case)
    raws, flags = lfmlib.bunzip2_device(streams, case.block_bytes)
    assert not any(flags)
    scatter_and_check(gpu, lfmlib, case, raws)


# ------------------------------------ whole files with blocks deep in c and t --
DEEP_SHAPE = (3, 3, 4, 52, 104)  # [t, c, z, y, x]
DEEP = {"u16": dict(header_version=8 + 4, nnum=13, block_size=[56, 26, 2, 2, 2]),  # predictor 4 forced; image-direct rows
        "u8": dict(header_version=8, nnum=13, block_size=[48, 26, 2, 2, 2])}        # unpredicted; 104-byte rows: gathered


@pytest.fixture(scope="module")
def deep_files(lfmlib, oracle, gpu):
    """{kind: (image, device tensor, .lfm bytes of Encoder.encode, stream counts, the oracle's .lfm)}"""
    torch = gpu
    t, c, z, y, x = DEEP_SHAPE
    imgs = {"u16": oracle.synthetic_lf(x, y, Z=z, C=c, Tn=t, T=13, seed=0x5D),
            "u8": np.random.default_rng(0x5D).integers(0, 200, DEEP_SHAPE, dtype=np.uint8)}
    old = lfmlib.get_family()
    lfmlib.set_family("tiles")
    enc = lfmlib.Encoder(device=0)
    out = {}
    try:
        for kind, img in imgs.items():
            d = torch.from_numpy(img.view(np.int16) if kind == "u16" else img).cuda()
            b, _ = enc.encode(d, **DEEP[kind])
            want = oracle.encode(img, family="tiles", data_type=1 if kind == "u16" else 0, **DEEP[kind])
            out[kind] = (img, d, b, enc.stream_counts(), want)
    finally:
        enc.close()
        lfmlib.set_family(old)
    return out


def to_numpy(torch, t, kind):
    return t.cpu().view(torch.int16).numpy().view(np.uint16) if kind == "u16" else t.cpu().numpy()


@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_deep_file_encode(deep_files, kind):
    """Encoder.encode of a device tensor with blocks two channels and two time
    points deep: the oracle's bytes, every stream compressed on the GPU."""
    img, _, b, counts, want = deep_files[kind]
    nb = [-(-d // s) for d, s in zip(DEEP_SHAPE[::-1], DEEP[kind]["block_size"])]
    assert nb == [2 if kind == "u16" else 3, 2, 2, 2, 2]
    assert counts["streams"] == int(np.prod(nb)) and counts["host_streams"] == 0, counts
    assert b == want


@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_deep_file_decode(lfmlib, gpu, deep_files, kind):
    """decode_device returns the input through the host reader (the pipelined
    GPU decode declines blocks deeper than one channel / time point), and a
    region that crosses a block border in every dimension, c and t included,
    is the numpy slice."""
    img, _, b, _, _ = deep_files[kind]
    old = lfmlib.get_family()
    lfmlib.set_family("tiles")
    try:
        got, st = lfmlib.decode_device(b, return_stats=True)
        lb, ub = [40, 20, 1, 1, 1], [60, 30, 2, 2, 2]
        roi = lfmlib.decode_roi_device(b, lb, ub)
    finally:
        lfmlib.set_family(old)
    assert tuple(got.shape) == DEEP_SHAPE and np.array_equal(to_numpy(gpu, got, kind), img)
    assert st["path"] == 1 and st["staged_bytes"] == 0, st
    assert st["chunks"] == 0 and st["blocks"] == st["host_blocks"] > 0, st
    bs = DEEP[kind]["block_size"]
    assert all(l // s != u // s for l, u, s in zip(lb, ub, bs))
    assert np.array_equal(to_numpy(gpu, roi, kind), img[1:3, 1:3, 1:3, 20:31, 40:61])
