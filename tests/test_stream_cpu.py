"""Streaming without a GPU (lfm.Writer / lfm_writer_*, lfm.Reader /
lfm_reader_*): a stack appended piece by piece gives the bytes lfm.write_lfm
gives for the whole array, and a region read fetches exactly the streams of
the blocks it touches.  Predictor request 8 (off) and the host libbz2
everywhere, uint16 noise unless said."""
import os
import struct

import numpy as np
import pytest

Z_COUNTS = (1, 2, 4, 3, 8, 1)


def noise(shape, dtype=np.uint16, seed=0x4C464D31):
    r = np.random.default_rng(seed)
    return r.integers(0, np.iinfo(dtype).max, size=shape, dtype=dtype, endpoint=True)


def one_shot(lfm, path, img, **kw):
    lfm.write_lfm(path, img, predictor_request=8, **kw)
    with open(path, "rb") as f:
        return f.read()


def streamed(lfm, path, img, counts, capacity, axis_tczyx, **kw):
    """img appended along tczyx axis `axis_tczyx` in pieces of `counts`;
    returns (file bytes, stats)."""
    shape = list(img.shape)
    shape[axis_tczyx] = capacity
    w = lfm.Writer(path, shape, dtype=img.dtype, predictor_request=8, **kw)
    at = 0
    for n in counts:
        sl = [slice(None)] * img.ndim
        sl[axis_tczyx] = slice(at, at + n)
        piece = img[tuple(sl)]
        # the count leads: [n, (dims below the axis)]
        piece = np.moveaxis(piece, axis_tczyx, 0).reshape((n,) + img.shape[axis_tczyx + 1:])
        w.append(piece[0] if n == 1 else piece)
        at += n
    assert at == img.shape[axis_tczyx]
    st = w.close()
    with open(path, "rb") as f:
        return f.read(), st


@pytest.fixture(scope="module")
def case1(lfmlib, tmp_path_factory):
    """40 x 24 x 19, block 16 x 16 x 4: (array, block size, one-shot bytes, path of the streamed file)."""
    d = tmp_path_factory.mktemp("stream1")
    img = noise((1, 1, 19, 24, 40))
    bs = [16, 16, 4, 1, 1]
    ref = one_shot(lfmlib, str(d / "ref.lfm"), img, block_size=bs)
    return img, bs, ref, d


@pytest.fixture(scope="module")
def case3(lfmlib, tmp_path_factory):
    """24 x 16 x 5 x 1 x 3, block 16 x 16 x 4 x 1 x 1."""
    d = tmp_path_factory.mktemp("stream3")
    img = noise((3, 1, 5, 16, 24), seed=0x4C464D33)
    bs = [16, 16, 4, 1, 1]
    ref = one_shot(lfmlib, str(d / "ref.lfm"), img, block_size=bs)
    return img, bs, ref, d


def test_z_axis_capacity_reached(lfmlib, case1):
    img, bs, ref, d = case1
    got, st = streamed(lfmlib, str(d / "cap19.lfm"), img, Z_COUNTS, 19, 2, block_size=bs)
    assert got == ref
    assert st["moved_bytes"] == 0 and st["appended"] == 19 and st["bytes_written"] == len(ref)
    assert st["staged_peak_bytes"] <= 3 * 40 * 24 * 2, st
    # layers complete at the appends that reach z = 4, 8 (with 10 taken), 16 (with 18); the tail at close
    assert st["ranges"] == 4 and st["streams"] == st["host_streams"] == 3 * 2 * 5, st
    assert st["chosen"] == 0 and st["header_version"] == 0


def test_z_axis_capacity_not_reached(lfmlib, case1):
    img, bs, ref, d = case1
    got, st = streamed(lfmlib, str(d / "cap64.lfm"), img, Z_COUNTS, 64, 2, block_size=bs)
    assert got == ref
    table_gap = 8 * (3 * 2 * 16 - 3 * 2 * 5)
    assert st["moved_bytes"] == len(ref) - 320 - 8 * 30 > 0 and table_gap > 0
    assert st["staged_peak_bytes"] <= 3 * 40 * 24 * 2, st


def test_final_extent_below_block_depth(lfmlib, tmp_path):
    """96 x 96 x 3 in a writer opened for 64 frames of block depth 8: the
    one-shot writer clamps the block to depth 3, whose 55 296 bytes are coded
    at bzip2 level 1; a nominal 96 x 96 x 8 block is coded at level 2."""
    bs = [96, 96, 8, 1, 1]
    deep = noise((1, 1, 8, 96, 96), seed=0x4C464D32)
    ref8 = one_shot(lfmlib, str(tmp_path / "ref8.lfm"), deep, block_size=bs)
    assert ref8[320 + 8:320 + 8 + 4] == b"BZh2"
    img = deep[:, :, :3]
    ref = one_shot(lfmlib, str(tmp_path / "ref3.lfm"), img, block_size=bs)
    assert ref[320 + 8:320 + 8 + 4] == b"BZh1" and struct.unpack_from("<5I", ref, 300)[2] == 3
    got, st = streamed(lfmlib, str(tmp_path / "s.lfm"), img, (1, 2), 64, 2, block_size=bs)
    assert got == ref
    assert st["ranges"] == 1 and st["moved_bytes"] > 0, st


@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1)])
def test_t_axis(lfmlib, case3, counts):
    img, bs, ref, d = case3
    got, st = streamed(lfmlib, str(d / ("t%d.lfm" % len(counts))), img, counts, 3, 0, block_size=bs)
    assert got == ref
    assert st["ranges"] == len(counts) and st["staged_peak_bytes"] == 0 and st["moved_bytes"] == 0, st


def test_c_axis(lfmlib, tmp_path):
    img = noise((1, 2, 5, 16, 24), seed=0x4C464D34)
    bs = [16, 16, 4, 1, 1]
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), img, block_size=bs)
    w = lfmlib.Writer(str(tmp_path / "s.lfm"), img.shape, predictor_request=8, block_size=bs)
    assert w.axis == 3
    w.abort()
    got, st = streamed(lfmlib, str(tmp_path / "s.lfm"), img, (1, 1), 2, 1, block_size=bs)
    assert got == ref and st["ranges"] == 2


@pytest.mark.parametrize("kind", ["uint8", "none"])
def test_other_types(lfmlib, tmp_path, kind):
    """A uint8 stack, and a uint16 stack stored uncompressed, of case 1's shape."""
    img = noise((1, 1, 19, 24, 40), np.uint8 if kind == "uint8" else np.uint16, seed=0x4C464D35)
    kw = dict(block_size=[16, 16, 4, 1, 1], compression=1 if kind == "uint8" else 0,
              pixel_size=[0.5, 0.5, 2.0, 1.0, 1.0], metadata="streamed")
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), img, **kw)
    for cap in (19, 40):
        got, _ = streamed(lfmlib, str(tmp_path / "s.lfm"), img, Z_COUNTS, cap, 2, **kw)
        assert got == ref


def test_errors(lfmlib, case1, tmp_path):
    img, bs, _, _ = case1
    short = img[:, :, :6]
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), short, block_size=bs)
    # past the capacity: code 3, nothing taken, and the close still gives the shorter file
    p = str(tmp_path / "a.lfm")
    w = lfmlib.Writer(p, (6, 24, 40), predictor_request=8, block_size=bs)
    assert w.axis == 2
    w.append(short[0, 0, :5])
    with pytest.raises(lfmlib.LfmError, match="code 3"):
        w.append(img[0, 0, 5:7])
    w.append(short[0, 0, 5])
    st = w.close()
    assert st["appended"] == 6 and open(p, "rb").read() == ref
    # nothing appended: close returns 3 and leaves no file
    p = str(tmp_path / "b.lfm")
    w = lfmlib.Writer(p, (6, 24, 40), predictor_request=8, block_size=bs)
    assert os.path.exists(p)
    with pytest.raises(lfmlib.LfmError, match="code 3"):
        w.close()
    assert not os.path.exists(p)
    # abort leaves no file; so does an exception inside a with block
    p = str(tmp_path / "c.lfm")
    w = lfmlib.Writer(p, (6, 24, 40), predictor_request=8, block_size=bs)
    w.append(short[0, 0, :5])
    w.abort()
    assert not os.path.exists(p)
    with pytest.raises(KeyError):
        with lfmlib.Writer(p, (6, 24, 40), predictor_request=8, block_size=bs) as w:
            w.append(short[0, 0, :4])
            raise KeyError("stop")
    assert not os.path.exists(p)
    with lfmlib.Writer(p, (6, 24, 40), predictor_request=8, block_size=bs) as w:
        w.append(short[0, 0])
    assert open(p, "rb").read() == ref and w.stats["appended"] == 6


def test_unclosed_file_is_rejected(lfmlib, case1, tmp_path):
    """A file whose writer never closed it has a zero table: the reader refuses it."""
    img, bs, _, _ = case1
    p = str(tmp_path / "open.lfm")
    w = lfmlib.Writer(p, (19, 24, 40), predictor_request=8, block_size=bs)
    w.append(img[0, 0, :8])
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.Reader(p)
    w.abort()


# ------------------------------------------------------------------ reader --
def parse(buf):
    """(xyzct, block size, header bytes, [compressed size per block]) of a .lfm."""
    xyzct = struct.unpack_from("<5I", buf, 2)
    bs = struct.unpack_from("<5I", buf, 300)
    nb = [-(-d // b) for d, b in zip(xyzct, bs)]
    n = int(np.prod(nb))
    ends = np.frombuffer(buf, dtype="<u8", count=n, offset=320)
    sizes = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    return xyzct, bs, 320 + 8 * n, nb, sizes


def touched_bytes(buf, lb, ub):
    """Sum of the compressed sizes of the blocks that intersect lb .. ub."""
    _, bs, _, nb, sizes = parse(buf)
    rng = [range(lo // b, hi // b + 1) for lo, hi, b in zip(lb, ub, bs)]
    total = 0
    for t in rng[4]:
        for c in rng[3]:
            for z in rng[2]:
                for y in rng[1]:
                    for x in rng[0]:
                        total += int(sizes[x + nb[0] * (y + nb[1] * (z + nb[2] * (c + nb[3] * t)))])
    return total


def crop(img, lb, ub):
    return img[lb[4]:ub[4] + 1, lb[3]:ub[3] + 1, lb[2]:ub[2] + 1, lb[1]:ub[1] + 1, lb[0]:ub[0] + 1]


@pytest.mark.parametrize("which", ["z", "t"])
def test_reader_fetches_only_the_blocks_it_needs(lfmlib, case1, case3, which):
    img, bs, ref, d = case1 if which == "z" else case3
    path = str(d / "read.lfm")
    axis = 2 if which == "z" else 0
    counts = Z_COUNTS if which == "z" else (1, 1, 1)
    got, _ = streamed(lfmlib, path, img, counts, img.shape[axis], axis, block_size=bs)
    assert got == ref
    xyzct, _, hbytes, _, sizes = parse(ref)
    hi = [v - 1 for v in xyzct]
    with lfmlib.Reader(path) as r:
        assert r.shape == img.shape and r.dtype == img.dtype and r.block_size == list(bs)
        assert r.header_version == 0 and r.nnum == 13 and r.file_bytes == len(ref)
        assert r.bytes_read == hbytes
        regions = {
            "whole": ([0, 0, 0, 0, 0], hi),
            "plane": ([0, 0, 2, 0, hi[4]], [hi[0], hi[1], 2, 0, hi[4]]),
            "volume": ([0, 0, 0, 0, hi[4]], hi),
            # x 10 .. 20 and y 12 .. 18 cross the block edge at 16 (the t file is one block high
            # in y: 16), z 3 .. 4 the one at 4
            "box": ([10, 12, 3, 0, 0], [20, min(18, hi[1]), 4, 0, hi[4] // 2]),
        }
        for name, (lb, ub) in regions.items():
            before = r.bytes_read
            out, st = r.read(lb, ub, return_stats=True)
            assert np.array_equal(out, crop(img, lb, ub)), name
            grown = r.bytes_read - before
            assert grown == touched_bytes(ref, lb, ub), name
            assert st["blocks"] > 0 and st["total_ms"] > 0, (name, st)
            if name == "whole":
                assert grown == int(sizes.sum()) == len(ref) - hbytes
            if name == "plane":
                assert grown < r.file_bytes / 2
        # a caller's buffer, and the codes of lfm_decode_memory_roi
        buf = np.empty(crop(img, *regions["box"]).size, dtype=img.dtype)
        out = r.read(*regions["box"], out=buf)
        assert np.shares_memory(out, buf) and np.array_equal(out, crop(img, *regions["box"]))
        with pytest.raises(ValueError):
            r.read([0, 0, 0, 0, 0], [xyzct[0], 0, 0, 0, 0])
        assert np.array_equal(lfmlib.decode_roi(ref, *regions["box"]), out)
