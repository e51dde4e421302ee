"""GPU decode of bzip2 blocks whose text after RLE1 is exactly periodic
(lfm_set_bunzip2_periodic, bzd_walk of csrc/lfm_bunzip2.hip): with the switch
on such streams come back with flag 0 and libbzip2's bytes, with it off (the
default) they are flagged for the host library as ever.  Every comparison is
byte-exact, against what the reference library compressed or, for streams
written by tests/bz2_craft.py, the crafted text (test_bunzip2_periodic_cpu.py
checks on the host that libbzip2 decompresses those to it).

Flags of lfm.bunzip2_device: 0 decoded, 1 handed to the host library (output
None), 2 decoded but the block CRC does not match (output None)."""
import numpy as np
import pytest

import bz2_cases as K
import bz2_multi_cases as M
import bz2_periodic_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bz(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


class switched:
    """with switched(lfm, on): the switch set, and put back to 0 whatever happens."""

    def __init__(self, lfmlib, on):
        self.lfm, self.on = lfmlib, on

    def __enter__(self):
        assert self.lfm.get_bunzip2_periodic() is False  # the default, and what every test leaves
        self.lfm.set_bunzip2_periodic(self.on)

    def __exit__(self, *exc):
        self.lfm.set_bunzip2_periodic(False)


def test_the_host_batch_decodes_on_the_device(lfmlib, bz, gpu):
    """The batch of test_bunzip2_gpu.test_periodic_streams_go_to_the_host:
    periodic texts of period 2, 2, 4 and 251 from libbzip2, w w (at most 128
    bytes, one walker per cycle) and w w w with each origPtr that names one of
    the equal rows and from libbzip2, each next to its neighbour of one more
    byte, which is not periodic.  Switch on: everything decodes.  Switch off,
    the same batch: the flags of today."""
    per = K.periodic_inputs()
    inputs, streams = [], []
    for d in per:
        inputs += [d, d + d[:1]]
        streams += [bz.compress(d, 1), bz.compress(d + d[:1], 1)]
    rep = K.repeated_cases()
    for text, stream, _ in rep:
        inputs += [text, text, text + text[:1]]
        streams += [stream, bz.compress(text, 1), bz.compress(text + text[:1], 1)]
    with switched(lfmlib, True):
        out, flags = lfmlib.bunzip2_device(streams, 12289)
    assert flags == [0] * len(streams)
    assert [i for i, (d, o) in enumerate(zip(inputs, out)) if o != d] == []
    with switched(lfmlib, False):
        out, flags = lfmlib.bunzip2_device(streams, 12289)
    assert flags == [1, 0] * len(per) + [1, 1, 0] * len(rep)
    for d, o, f in zip(inputs, out, flags):
        assert o == (None if f else d), len(d)


def test_seams(lfmlib, gpu):
    """Periods m = 2 .. 1300 repeated 2, 3 and 7 times: the fill's aligned
    16-byte pieces start inside, at and behind a piece's edge and the last one
    ends anywhere; periods around kMark (the start's cycle with no, one and a
    few regular markers) and kWalkKeep (kept bytes alone, and the re-walk of a
    longer segment: m1300_r2_o1 is one segment of 1300 bytes, long_segment has
    one above 512 between shorter ones); w w w from each of its three equal
    rows; 4 500 cycles of 2 rows, where all but one walker are off the start's
    cycle; q = 1.  One batch, flag 0 and the exact bytes for every stream."""
    cases = P.seam_cases()
    with switched(lfmlib, True):
        out, flags = lfmlib.bunzip2_device([s for _, _, s in cases], P.SEAM_STRIDE)
    assert {name: f for (name, _, _), f in zip(cases, flags) if f} == {}
    assert [name for (name, data, _), o in zip(cases, out) if o != data] == []


def test_wrong_start_row(lfmlib, bz, gpu):
    """A periodic text whose origPtr names a row of another rotation: decoded
    like any other (n steps from origPtr), and the CRC says no: flag 2 with
    the switch on, the host library's with it off, never flag 0.  A good
    stream on either side decodes."""
    text, stream, _ = P.wrong_start()
    good = K.noruns(300, 9, 50)
    streams = [bz.compress(good, 1), stream, bz.compress(good[::-1], 1)]
    with switched(lfmlib, True):
        assert lfmlib.bunzip2_device(streams, 401) == ([good, None, good[::-1]], [0, 2, 0])
    with switched(lfmlib, False):
        assert lfmlib.bunzip2_device(streams, 401) == ([good, None, good[::-1]], [0, 1, 0])


def test_multi_entries(lfmlib, bz, gpu):
    """The _multi entries: 83 334 x "abc" cut to 250 000 bytes is three bzip2
    blocks at level 1, the first two 33 327 x "abc" (q = 3, n = 99 981: the
    fill writes all but three bytes of the text), next to a 3-part stream of
    random bytes."""
    rows = M.mixed_rows()
    inputs = [rows[4], rows[0]]
    streams = [bz.compress(d, 1) for d in inputs]
    with switched(lfmlib, True):
        out, flags = lfmlib.bunzip2_device(streams, 250000, multi=True, level=1)
    assert flags == [0, 0] and out == inputs
    with switched(lfmlib, False):
        out, flags = lfmlib.bunzip2_device(streams, 250000, multi=True, level=1)
    assert flags == [1, 0] and out == [None, inputs[1]]


def engine_files(oracle):
    """[(image, .lfm, block size, constant blocks, region)]: unpredicted files,
    half of their blocks constant (periodic) and half noise; the region cuts
    through blocks of both kinds."""
    rng = np.random.default_rng(12)
    u16 = rng.integers(0, 65536, (1, 1, 16, 256, 256), dtype=np.uint16)
    u8 = rng.integers(0, 256, (1, 1, 8, 64, 144), dtype=np.uint8)
    pattern = np.tile(np.array([3, 7, 11], np.uint8), 16)  # a block's row of 48 bytes
    out = []
    for img, bs, region in ((u16, [64, 64, 8, 1, 1], ([3, 5, 2, 0, 0], [200, 130, 11, 0, 0])),
                            (u8, [48, 32, 4, 1, 1], ([5, 3, 1, 0, 0], [100, 40, 6, 0, 0]))):
        xyzct = list(img.shape[::-1])
        const = 0
        for _, (x0, y0, z0, _, _), _ in oracle.iter_blocks(xyzct, bs):
            if (x0 // bs[0] + y0 // bs[1] + z0 // bs[2]) % 2 == 0:
                const += 1
                img[0, 0, z0:z0 + bs[2], y0:y0 + bs[1], x0:x0 + bs[0]] = 0x0201 if img.dtype == np.uint16 else pattern
        buf = oracle.encode(img, data_type=0 if img.dtype == np.uint8 else 1, header_version=8, nnum=13,
                            block_size=bs)  # request 8: predictor 0 forced
        h = oracle.parse_header(buf)
        assert h["header_version"] == 0 and h["nb"] == 2 * const
        out.append((img, buf, const, region))
    assert [c for _, _, c, _ in out] == [16, 6]
    return out


def test_engine(lfmlib, oracle, gpu):
    """Every reader that decodes on the GPU, on a uint16 file whose constant
    blocks are 0x0201 (period 2) and a uint8 file whose constant blocks repeat
    3 7 11: host and device destinations, a region, two workers on device 0.
    Switch on: the pixels, and no block handed to the host library.  Switch
    off: the pixels, and the constant blocks decoded there."""
    files = engine_files(oracle)
    try:
        for on in (True, False):
            with switched(lfmlib, on):
                for img, buf, const, (lb, ub) in files:
                    want = 0 if on else const
                    assert np.array_equal(lfmlib.decode(buf), img)
                    dev, st = lfmlib.decode_device(buf, return_stats=True)
                    assert (st["path"], st["blocks"], st["host_blocks"]) == (0, 2 * const, want), (on, st)
                    assert np.array_equal(dev.cpu().numpy(), img)
                    roi, st = lfmlib.decode_roi_device(buf, lb, ub, return_stats=True)
                    assert st["host_blocks"] == 0 if on else 0 < st["host_blocks"] <= const, (on, st)
                    assert np.array_equal(roi.cpu().numpy(),
                                          img[:, :, lb[2]:ub[2] + 1, lb[1]:ub[1] + 1, lb[0]:ub[0] + 1])
                    lfmlib.set_decode_devices([0, 0])
                    got, st = lfmlib.decode_multi(buf, return_stats=True)
                    lfmlib.set_decode_devices(None)
                    assert st["workers"] == 2 and st["host_blocks"] == want, (on, st)
                    assert np.array_equal(got, img)
    finally:
        lfmlib.set_decode_devices(None)
        lfmlib.release_decoders()
