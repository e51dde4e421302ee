"""The bzip2 block-cut rule of tests/bz2_parts.py against the reference
library, on the CPU: for every cut-edge input of the GPU multi-block tests the
rule's parts have the block CRCs and the combined CRC found in
BZ2_bzBuffToBuffCompress's stream.  Also the stream counts of an encoder that
has no GPU."""
import numpy as np
import pytest

import bz2_parts
from bz2_craft import rle1

CASES = bz2_parts.level1_cases()
EXTRA = [  # levels 2 and 9 (the GPU tests' sizes), and a final block of exactly nblockMAX + 5
    ("random-450000-l2", np.random.default_rng(7).integers(0, 256, 450000, dtype=np.uint8).tobytes(), 2),
    ("random-1000000-l9", np.random.default_rng(8).integers(0, 256, 1000000, dtype=np.uint8).tobytes(), 9),
    ("runs4-l1", np.repeat(np.arange(250000 // 4, dtype=np.uint32) % 251, 4).astype(np.uint8).tobytes(), 1),
]


def _ref(oracle, data, level):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz.compress(bytes(data), level)


@pytest.mark.parametrize("name,data,level", [(n, d, 1) for n, d in CASES] + EXTRA,
                         ids=[n for n, _ in CASES] + [e[0] for e in EXTRA])
def test_cut_rule_matches_reference_crcs(oracle, name, data, level):
    parts = bz2_parts.parts(data, level)
    # the parts tile the input and the uncut RLE1 text
    assert parts[0][0] == 0 and sum(p[1] for p in parts) == len(data)
    assert all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert sum(p[2] for p in parts) == len(rle1(data))
    nmax = bz2_parts.nblock_max(level)
    assert all(nmax <= p[2] <= nmax + 4 for p in parts[:-1]) and parts[-1][2] <= nmax + 5
    crcs, comb = bz2_parts.part_crcs(data, level)
    assert (crcs, comb) == bz2_parts.stream_crcs(_ref(oracle, data, level))


def test_expected_part_counts():
    """The counts the GPU tests rely on."""
    n = {name: len(bz2_parts.parts(d, 1)) for name, d in CASES}
    assert n["runfree-99980"] == 1 and n["runfree-99982"] == 1 and n["runfree-99983"] == 2
    assert n["runfree-199963"] == 2 and n["runfree-199964"] == 3
    assert n["draw-00012"] == 6 and n["random-250000"] == 3
    assert [len(bz2_parts.parts(d, lv)) for _, d, lv in EXTRA] == [3, 2, 4]
    assert max(bz2_parts.parts(d, 1)[-1][2] for name, d in CASES if name.startswith("last1")) == 99981 + 5


def test_stream_counts_without_gpu(lfmlib, oracle):
    """No GPU bzip2 ran: every stream was compressed by the host library."""
    no_gpu = lfmlib.device_count() <= 0  # (the GPU suite checks the counts of GPU encodes)
    img = np.random.default_rng(4).integers(0, 5, (1, 1, 3, 48, 64), dtype=np.uint8)  # 8-bit: no predictor stage
    kw = dict(header_version=8, nnum=13, block_size=[32, 24, 2, 1, 1])
    enc = lfmlib.Encoder()
    try:
        assert enc.stream_counts() == {"streams": 0, "host_streams": 0, "bzip2_blocks": 0}
        b, _ = enc.encode(img, **kw)
        c = enc.stream_counts()
    finally:
        enc.close()
    assert b == oracle.encode(img, data_type=0, **kw)
    assert c["streams"] == 2 * 2 * 2
    if no_gpu:
        assert c["host_streams"] == c["streams"] and c["bzip2_blocks"] == 0
    assert lfmlib.get_bzip2_multiblock() is True
    assert lfmlib.set_bzip2_multiblock(False) is True and lfmlib.get_bzip2_multiblock() is False
    assert lfmlib.set_bzip2_multiblock(True) is False
