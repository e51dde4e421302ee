"""Checkpoints, recovery and the live reader without a GPU (lfm.Writer.flush,
lfm.recover, lfm.Reader(live=True)): the writer puts a finished layer's table
entries into the file behind its payload, so a file that is never closed still
yields the .lfm of its complete layers, byte for byte the one-shot writer's, and
can be read while it grows.  Predictor request 8 (off) and host arrays; the
stacks are those of test_stream_cpu.py.  Everything runs without a GPU, on the
host libbz2; where a device is visible, recovery verifies the bzip2 streams on
it (host_streams tells), with the same results.

A "crashed" file is made without a crash: after flush() the still-open writer's
file is copied and the writer aborted -- the copy is what a killed process
leaves.  One test does it with a real child process that leaves through
os._exit."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_stream_cpu import crop, noise, one_shot, touched_bytes

BS = [16, 16, 4, 1, 1]
FIXED = 320
LAYER = 3 * 2  # blocks of one z-layer of the 40 x 24 stack


def host_verified(lfm, n):
    """stats.host_streams after n bzip2 streams were verified: all of them without a device, none with one."""
    return n if lfm.device_count() <= 0 else 0


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def table_of(buf, nb):
    return list(struct.unpack_from("<%dQ" % nb, buf, FIXED))


def crashed(lfm, path, pieces, shape, committed, **kw):
    """A writer of `shape` takes `pieces`, is flushed (`committed` indices must
    be on file then) and aborted; what its file held is left at `path`."""
    live = path + ".open"
    w = lfm.Writer(live, shape, predictor_request=8, **kw)
    try:
        for p in pieces:
            w.append(p)
        assert w.flush() == committed
        shutil.copyfile(live, path)
    finally:
        w.abort()
    assert not os.path.exists(live)
    return path


@pytest.fixture(scope="module")
def case1(lfmlib, tmp_path_factory):
    """40 x 24 x 19, block 16 x 16 x 4: (array, directory, {k: one-shot bytes of the first k frames})."""
    d = tmp_path_factory.mktemp("live1")
    img = noise((1, 1, 19, 24, 40))
    refs = {k: one_shot(lfmlib, str(d / ("ref%d.lfm" % k)), img[:, :, :k], block_size=BS) for k in (4, 8, 12, 16, 19)}
    return img, d, refs


@pytest.fixture(scope="module")
def torn(lfmlib, case1):
    """Bytes of a crashed file of capacity 19 with two layers (8 frames) committed, 10 appended."""
    img, d, _ = case1
    return read_file(crashed(lfmlib, str(d / "torn.lfm"), [img[0, 0, :10]], (19, 24, 40), 8, block_size=BS))


# ------------------------------------------------------------- checkpoints --
def test_checkpoint_contents(lfmlib, case1, tmp_path):
    """Appends of 1, 2, 4 frames complete one layer: after flush its six
    entries, and no others, are in the capacity-sized table with the values
    close writes, and byte 0 is the header byte the ranges produced (0), no
    longer the request (8)."""
    img, _, refs = case1
    p = str(tmp_path / "open.lfm")
    w = lfmlib.Writer(p, (19, 24, 40), predictor_request=8, block_size=BS)
    try:
        assert read_file(p)[0] == 8 and not any(table_of(read_file(p), 30))
        at = 0
        for n in (1, 2, 4):
            w.append(img[0, 0, at:at + n])
            at += n
        assert w.flush() == 4
        buf = read_file(p)
        table = table_of(buf, 30)
        assert all(table[:LAYER]) and not any(table[LAYER:])
        assert table[:LAYER] == table_of(refs[19], 30)[:LAYER]
        assert buf[0] == refs[19][0] == 0
        assert struct.unpack_from("<5I", buf, 2)[2] == 19  # the capacity until close
        # the payload lies behind the capacity-sized table
        assert buf[FIXED + 8 * 30:FIXED + 8 * 30 + table[5]] == refs[19][FIXED + 8 * 30:FIXED + 8 * 30 + table[5]]
        assert w.flush(sync=True) == 4  # nothing new: the three frames held back are not covered
    finally:
        w.abort()


@pytest.mark.parametrize("capacity", [19, 64])
def test_closed_file_identity_with_flushes(lfmlib, case1, tmp_path, capacity):
    """A flush after every append changes nothing in the closed file."""
    img, _, refs = case1
    p = str(tmp_path / "s.lfm")
    w = lfmlib.Writer(p, (capacity, 24, 40), predictor_request=8, block_size=BS)
    at, seen = 0, []
    for n in (1, 2, 4, 3, 8, 1):
        w.append(img[0, 0, at:at + n])
        at += n
        seen.append(w.flush(sync=(n == 3)))
    assert seen == [0, 0, 4, 8, 16, 16]
    st = w.close()
    assert read_file(p) == refs[19]
    assert st["committed"] == st["appended"] == 19 and st["ranges"] == 4
    assert (st["moved_bytes"] > 0) == (capacity == 64)


# ---------------------------------------------------------------- recovery --
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in_place"])
@pytest.mark.parametrize("k", [4, 8, 16])
def test_recovery_gives_the_one_shot_file(lfmlib, case1, tmp_path, k, in_place):
    """k committed frames (one more appended and held back): the recovered
    file is the one-shot writer's of img[:k]."""
    img, _, refs = case1
    src = crashed(lfmlib, str(tmp_path / "crash.lfm"), [img[0, 0, :k + 1]], (19, 24, 40), k, block_size=BS)
    before = read_file(src)
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.Reader(src)
    if in_place:
        st = lfmlib.recover(src)
        got = read_file(src)
    else:
        out = str(tmp_path / "out.lfm")
        st = lfmlib.recover(src, out=out)
        got = read_file(out)
        assert read_file(src) == before
    assert got == refs[k]
    assert st["kept"] == k and st["capacity"] == 19 and st["axis"] == 2 and st["already_valid"] == 0, st
    assert st["dropped_layers"] == 0 and st["moved_bytes"] == len(got) - FIXED - 8 * LAYER * (k // 4) > 0, st
    assert st["committed_blocks"] == LAYER * (k // 4) and st["bytes_written"] == len(got), st
    assert st["verified_streams"] == LAYER * (k // 4) and st["header_version"] == 0, st
    assert st["host_streams"] == host_verified(lfmlib, LAYER * (k // 4)), st
    assert np.array_equal(lfmlib.decode(got), img[:, :, :k])


def test_recovery_without_verification(lfmlib, case1, torn, tmp_path):
    _, _, refs = case1
    src, out = str(tmp_path / "c.lfm"), str(tmp_path / "o.lfm")
    with open(src, "wb") as f:
        f.write(torn)
    st = lfmlib.recover(src, out=out, verify=False)
    assert read_file(out) == refs[8] and st["kept"] == 8 and st["verified_streams"] == 0, st


def test_recovery_t_axis(lfmlib, tmp_path):
    """24 x 16 x 5 x 1 x 3 by volumes: two of three committed."""
    img = noise((3, 1, 5, 16, 24), seed=0x4C464D33)
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), img[:2], block_size=BS)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [img[0], img[1]], img.shape, 2, block_size=BS)
    st = lfmlib.recover(src)
    assert read_file(src) == ref
    assert st["axis"] == 4 and st["kept"] == 2 and st["capacity"] == 3 and st["committed_blocks"] == 8, st


def test_recovery_c_axis(lfmlib, tmp_path):
    img = noise((1, 2, 5, 16, 24), seed=0x4C464D34)
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), img[:, :1], block_size=BS)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [img[0, 0]], img.shape, 1, block_size=BS)
    st = lfmlib.recover(src)
    assert read_file(src) == ref and st["axis"] == 3 and st["kept"] == 1, st


@pytest.mark.parametrize("kind", ["uint8", "none"])
def test_recovery_other_types(lfmlib, tmp_path, kind):
    """A uint8 stack, and a uint16 stack stored uncompressed (of which only the
    stored sizes can be verified)."""
    img = noise((1, 1, 19, 24, 40), np.uint8 if kind == "uint8" else np.uint16, seed=0x4C464D35)
    kw = dict(block_size=BS, compression=1 if kind == "uint8" else 0, pixel_size=[0.5, 0.5, 2.0, 1.0, 1.0],
              metadata="streamed")
    ref = one_shot(lfmlib, str(tmp_path / "ref.lfm"), img[:, :, :8], **kw)
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [img[0, 0, :11]], (40, 24, 40), 8, dtype=img.dtype, **kw)
    st = lfmlib.recover(src)
    assert read_file(src) == ref and st["kept"] == 8 and st["verified_streams"] == 2 * LAYER, st
    assert st["host_streams"] == (host_verified(lfmlib, 2 * LAYER) if kind == "uint8" else 0), st


# -------------------------------------------------------------- torn files --
def put(path, buf):
    with open(path, "wb") as f:
        f.write(buf)
    return path


@pytest.mark.parametrize("verify", [True, False])
def test_truncated_in_the_second_layer(lfmlib, case1, torn, tmp_path, verify):
    """The file ends in the middle of layer 2's payload: its entries point past
    the end, so one layer is kept with or without verification."""
    _, _, refs = case1
    table = table_of(torn, 30)
    assert all(table[:2 * LAYER]) and not any(table[2 * LAYER:])
    cut = FIXED + 8 * 30 + (table[LAYER - 1] + table[2 * LAYER - 1]) // 2
    src = put(str(tmp_path / "c.lfm"), torn[:cut])
    st = lfmlib.recover(src, verify=verify)
    assert read_file(src) == refs[4]
    assert st["kept"] == 4 and LAYER <= st["committed_blocks"] < 2 * LAYER and st["dropped_layers"] == 1, st


def test_zeroed_second_layer(lfmlib, case1, torn, tmp_path):
    """Layer 2's payload bytes are zeros under intact table entries (entries
    that reached the disk before their payload): verify=True keeps one layer;
    verify=False trusts the table and keeps both -- a file whose second layer
    does not decode, which is why verify=False is for process crashes only."""
    _, _, refs = case1
    table = table_of(torn, 30)
    base = FIXED + 8 * 30
    bad = bytearray(torn)
    bad[base + table[LAYER - 1]:base + table[2 * LAYER - 1]] = bytes(table[2 * LAYER - 1] - table[LAYER - 1])
    src = put(str(tmp_path / "c.lfm"), bytes(bad))
    st = lfmlib.recover(src, out=str(tmp_path / "v.lfm"), verify=True)
    assert read_file(str(tmp_path / "v.lfm")) == refs[4]
    assert st["kept"] == 4 and st["dropped_layers"] == 1 and st["committed_blocks"] == 2 * LAYER, st
    st = lfmlib.recover(src, out=str(tmp_path / "t.lfm"), verify=False)
    got = read_file(str(tmp_path / "t.lfm"))
    assert st["kept"] == 8 and st["dropped_layers"] == 0 and len(got) == len(refs[8]), st
    assert got[:FIXED + 8 * 2 * LAYER] == refs[8][:FIXED + 8 * 2 * LAYER] and got != refs[8]
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.decode(got)
    # one damaged byte in one stream of layer 2 is enough for the bzip2 CRC
    bad = bytearray(torn)
    bad[base + table[LAYER + 2] - 20] ^= 0x10
    st = lfmlib.recover(put(src, bytes(bad)), verify=True)
    assert st["kept"] == 4 and st["dropped_layers"] == 1 and read_file(src) == refs[4], st


def test_decreasing_entry_ends_the_prefix(lfmlib, case1, torn, tmp_path):
    _, _, refs = case1
    table = table_of(torn, 30)
    bad = bytearray(torn)
    struct.pack_into("<Q", bad, FIXED + 8 * (LAYER + 1), table[LAYER] - 1)
    src = put(str(tmp_path / "c.lfm"), bytes(bad))
    st = lfmlib.recover(src, verify=False)
    assert st["committed_blocks"] == LAYER + 1 and st["kept"] == 4 and st["dropped_layers"] == 1, st
    assert read_file(src) == refs[4]


@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in_place"])
def test_nothing_committed(lfmlib, case1, tmp_path, in_place):
    """Three frames appended, none committed: code 3, the input untouched, no output."""
    img, _, _ = case1
    src = crashed(lfmlib, str(tmp_path / "c.lfm"), [img[0, 0, :3]], (19, 24, 40), 0, block_size=BS)
    before = read_file(src)
    out = None if in_place else str(tmp_path / "o.lfm")
    with pytest.raises(lfmlib.LfmError, match="code 3"):
        lfmlib.recover(src, out=out)
    assert read_file(src) == before and sorted(os.listdir(str(tmp_path))) == ["c.lfm"]
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.recover(str(tmp_path / "missing.lfm"))
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.recover(put(str(tmp_path / "short.lfm"), before[:FIXED + 8 * 29]))


def test_closed_file_is_left_alone(lfmlib, case1, tmp_path):
    _, _, refs = case1
    src = put(str(tmp_path / "closed.lfm"), refs[19])
    for out in (None, str(tmp_path / "o.lfm")):
        st = lfmlib.recover(src, out=out)
        assert st["already_valid"] == 1 and st["kept"] == st["capacity"] == 19 and st["bytes_written"] == 0, st
        assert read_file(src) == refs[19] and os.listdir(str(tmp_path)) == ["closed.lfm"]


def test_killed_child_process(lfmlib, case1, tmp_path):
    """A fresh process appends nine frames, flushes, reports what is committed
    and leaves through os._exit without closing; the parent recovers eight."""
    img, _, refs = case1
    p = str(tmp_path / "child.lfm")
    code = "\n".join([
        "import os, sys",
        "sys.path.insert(0, %r)" % lfmlib.PKG_DIR,
        "import numpy as np",
        "import lfm",
        "r = np.random.default_rng(0x4C464D31)",
        "img = r.integers(0, 65535, size=(1, 1, 19, 24, 40), dtype=np.uint16, endpoint=True)",
        "w = lfm.Writer(%r, (19, 24, 40), predictor_request=8, block_size=%r)" % (p, BS),
        "w.append(img[0, 0, :9])",
        "print('committed', w.flush(sync=True), flush=True)",
        "os._exit(0)",
    ])
    run = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout.decode().split()[-2:] == ["committed", "8"], run.stdout
    assert os.path.exists(p)
    with pytest.raises(lfmlib.LfmError, match="code 2"):
        lfmlib.Reader(p)
    st = lfmlib.recover(p)
    assert st["kept"] == 8 and read_file(p) == refs[8], st


# ------------------------------------------------------------- live reader --
def test_live_reader_follows_the_writer(lfmlib, case1, tmp_path):
    """Capacity 64, 19 appended: the extent grows by whole layers with each
    flush + refresh, a region read fetches exactly its streams from behind the
    capacity-sized table, and after close (a shorter table, the payload moved)
    refresh re-parses the file."""
    img, _, refs = case1
    p = str(tmp_path / "live.lfm")
    nb_cap = LAYER * 16
    head = FIXED + 8 * nb_cap
    w = lfmlib.Writer(p, (64, 24, 40), predictor_request=8, block_size=BS)
    try:
        r = lfmlib.Reader(p, live=True)
        assert r.shape == (1, 1, 0, 24, 40) and r.bytes_read == head and r.block_size == BS
        with pytest.raises(lfmlib.LfmError, match="code 3"):
            r.read([0, 0, 0, 0, 0], [39, 23, 0, 0, 0])
        w.append(img[0, 0, :3])
        assert w.flush() == 0 and r.refresh() == (1, 1, 0, 24, 40)
        assert r.bytes_read == 2 * head
        at, known = 3, 0
        for n, k in ((2, 4), (8, 12), (3, 16)):
            w.append(img[0, 0, at:at + n])
            at += n
            assert w.flush() == k
            assert r.shape[2] == known // LAYER * 4  # nothing moves without refresh
            before = r.bytes_read
            assert r.refresh() == r.shape == (1, 1, k, 24, 40)
            assert r.bytes_read - before == FIXED + 8 * (nb_cap - known)
            known = LAYER * (k // 4)
            assert r.header_version == 0 and r.file_bytes == os.path.getsize(p)
            regions = {
                "extent": ([0, 0, 0, 0, 0], [39, 23, k - 1, 0, 0]),
                "last layer": ([0, 0, k - 4, 0, 0], [39, 23, k - 1, 0, 0]),
                # x 10 .. 20 and y 12 .. 18 cross the block edge at 16, z 3 .. 4 the one at 4
                "box": ([10, 12, 3, 0, 0], [20, 18, min(4, k - 1), 0, 0]),
            }
            for name, (lb, ub) in regions.items():
                before = r.bytes_read
                out, st = r.read(lb, ub, return_stats=True)
                assert np.array_equal(out, crop(img, lb, ub)), (k, name)
                assert r.bytes_read - before == touched_bytes(refs[k], lb, ub), (k, name)
                assert st["blocks"] > 0, (k, name, st)
            with pytest.raises(lfmlib.LfmError, match="code 3"):
                r.read([0, 0, k, 0, 0], [39, 23, k, 0, 0])
            with pytest.raises(lfmlib.LfmError, match="code 2"):
                lfmlib.Reader(p)
        w.append(img[0, 0, at:])
        st = w.close()
        assert st["moved_bytes"] > 0 and read_file(p) == refs[19]
        assert r.refresh() == (1, 1, 19, 24, 40) and r.file_bytes == len(refs[19])
        whole = ([0, 0, 0, 0, 0], [39, 23, 18, 0, 0])
        before = r.bytes_read
        assert np.array_equal(r.read(*whole), img)
        assert r.bytes_read - before == len(refs[19]) - FIXED - 8 * 30
        assert r.refresh() == (1, 1, 19, 24, 40)  # closed: nothing more to look for
        r.close()
    finally:
        w.abort()


def test_live_reader_when_the_capacity_is_reached(lfmlib, case1, tmp_path):
    """Capacity 19 reached: close completes the table in place, refresh finds
    it complete; a live reader of a closed file is the plain reader."""
    img, _, refs = case1
    p = str(tmp_path / "live.lfm")
    with lfmlib.Writer(p, (19, 24, 40), predictor_request=8, block_size=BS) as w:
        w.append(img[0, 0, :17])
        assert w.flush() == 16
        r = lfmlib.Reader(p, live=True)
        assert r.shape == (1, 1, 16, 24, 40)
        assert np.array_equal(r.read([0, 0, 8, 0, 0], [39, 23, 15, 0, 0]), img[:, :, 8:16])
        w.append(img[0, 0, 17:])
    assert read_file(p) == refs[19]
    assert r.refresh() == (1, 1, 19, 24, 40)
    assert np.array_equal(r.read([0, 0, 16, 0, 0], [39, 23, 18, 0, 0]), img[:, :, 16:])
    r.close()
    with lfmlib.Reader(p, live=True) as r2, lfmlib.Reader(p) as r1:
        assert r2.shape == r1.shape == img.shape and r2.bytes_read == r1.bytes_read == FIXED + 8 * 30
        assert r2.refresh() == img.shape and r2.bytes_read == r1.bytes_read
        with pytest.raises(ValueError):
            r1.read([0, 0, 19, 0, 0], [39, 23, 19, 0, 0])
