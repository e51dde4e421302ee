"""Inputs of the multi-block GPU bzip2 decoder tests, shared by
test_bunzip2_multiblock_cpu.py (their premises, against libbzip2 on the host)
and test_bunzip2_multiblock_gpu.py.  TEST INFRASTRUCTURE ONLY.

`compress(data, level)` is the reference library's BZ2_bzBuffToBuffCompress
(oracle.bzip2().compress) everywhere."""
import numpy as np

import bz2_parts
from bz2_craft import BLOCK_MAGIC, EOS_MAGIC, get_bits, patch_bits


def find_magic(stream, magic):
    """Bit positions of a 48-bit magic in a stream, at any bit offset (the
    search of bz2_parts.stream_crcs, returning the positions)."""
    big, nbits = int.from_bytes(stream, "big"), 8 * len(stream)
    pat, hits = magic.to_bytes(6, "big"), []
    for sh in range(8):  # the stream shifted left by sh bits: a magic at bit 8 k + sh is at byte k
        s = ((big << sh) & ((1 << nbits) - 1)).to_bytes(len(stream), "big")
        k = s.find(pat)
        while k >= 0:
            hits.append(8 * k + sh)
            k = s.find(pat, k + 1)
    return sorted(hits)


def rotl1(x):
    return ((x << 1) | (x >> 31)) & 0xFFFFFFFF


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def mixed_rows():
    """The five 250 000-byte rows of test_bzip2_multiblock_gpu.test_mixed_batch:
    3, 1, 3, 4 and 3 parts at level 1, the last one's first part periodic."""
    n = 250000
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            bytes(n),
            rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), n).tobytes(),
            np.repeat(np.arange(n // 4, dtype=np.uint32) % 251, 4).astype(np.uint8).tobytes(),
            (b"abc" * 83334)[:n]]


TWO_PART_LEN = 100500  # run_free bytes at level 1: parts of 99 981 and 519 bytes (RLE1 leaves them alone)
TWO_PART_STRIDE = 100501


def two_part(compress):
    """(data, stream, facts) of the 2-part level-1 stream the bad streams are
    patched from; facts: the bit positions of its two block magics and its end
    magic, the two block CRCs and the second block's length."""
    data = bz2_parts.run_free(TWO_PART_LEN, seed=8)
    stream = compress(data, 1)
    blocks, ends = find_magic(stream, BLOCK_MAGIC), find_magic(stream, EOS_MAGIC)
    assert len(blocks) == 2 and len(ends) == 1 and blocks[0] == 32
    crcs = [get_bits(stream, p + 48, 32) for p in blocks]
    parts = bz2_parts.parts(data, 1)
    assert [t for _, _, t in parts] == [bz2_parts.nblock_max(1), TWO_PART_LEN - bz2_parts.nblock_max(1)]
    assert get_bits(stream, ends[0] + 48, 32) == rotl1(rotl1(0) ^ crcs[0]) ^ crcs[1]
    return data, stream, dict(block=blocks, eos=ends[0], crc=crcs, n2=parts[1][2])


def bad_two_part(compress):
    """[(name, stream, flag)]: the 2-part stream with one field damaged; flag
    is what the GPU decoder must answer (1: host library, 2: CRC mismatch).
    libbzip2 rejects every one of them."""
    _, s, f = two_part(compress)
    b2, eos, (c1, c2) = f["block"][1], f["eos"], f["crc"]
    c2x = c2 ^ 0x00010000
    orig2 = b2 + 48 + 32 + 1  # behind the magic, the block CRC and the randomised bit
    return [
        ("crc2_and_combined", patch_bits(patch_bits(s, b2 + 48, 32, c2x), eos + 48, 32, rotl1(c1) ^ c2x), 2),
        ("combined_alone", patch_bits(s, eos + 48, 32, (rotl1(c1) ^ c2) ^ 1), 1),
        ("block2_magic", patch_bits(s, b2, 48, BLOCK_MAGIC ^ 1), 1),
        ("eos_magic", patch_bits(s, eos, 48, EOS_MAGIC ^ 1), 1),
        ("trunc_in_block2", s[:(b2 + (eos - b2) * 3 // 4) // 8], 1),
        ("orig2_eq_n2", patch_bits(s, orig2, 24, f["n2"]), 1),
    ]
