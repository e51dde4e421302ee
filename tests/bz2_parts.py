"""Where libbzip2 1.0.6 cuts a stream into bzip2 blocks, restated from bzlib.c
(ADD_CHAR_TO_BLOCK, copy_input_until_stop, handle_compress) for
BZ2_bzBuffToBuffCompress, i.e. one BZ_FINISH call.  TEST INFRASTRUCTURE ONLY.

RLE1 works in pieces: a maximal run of equal bytes, cut every 255 bytes.  A
piece of l bytes adds min(l, 4) + (l >= 4) bytes to the block's text when the
next input byte arrives.  nblock >= nblockMAX (100000 * level - 19) is tested
before each input byte is read, so a block ends in front of the first piece
whose text position has reached nblockMAX past the block's start -- unless
that piece is the stream's last byte: libbzip2 has read it by then and it
joins the block.  The run state is not reset at a cut, so the parts' texts are
consecutive ranges of the uncut RLE1 text.

    parts(data, level) -> [(raw_start, raw_len, text_len), ...]

Python's bz2.compress is NOT this function (BZ_RUN, then BZ_FINISH: it cuts
differently when the limit is reached at the last byte).
"""
import numpy as np

from bz2_craft import BLOCK_MAGIC, crc32, get_bits


def nblock_max(level):
    return 100000 * level - 19


def pieces(data):
    """(raw start, length) of every RLE1 piece, as two int64 arrays."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if a.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    run_start = np.concatenate(([0], np.flatnonzero(a[1:] != a[:-1]) + 1)).astype(np.int64)
    run_len = np.diff(np.concatenate((run_start, [a.size])))
    npiece = (run_len + 254) // 255
    first = np.repeat(run_start, npiece)
    k = np.arange(int(npiece.sum()), dtype=np.int64) - np.repeat(np.cumsum(npiece) - npiece, npiece)
    start = first + 255 * k
    length = np.minimum(255, np.repeat(run_start + run_len, npiece) - start)
    return start, length


def parts(data, level):
    start, length = pieces(data)
    if start.size == 0:
        return []
    L, limit = len(data), nblock_max(level)
    text_before = np.concatenate(([0], np.cumsum(np.minimum(length, 4) + (length >= 4))))
    out, p = [], 0
    while True:
        j = int(np.searchsorted(text_before, text_before[p] + limit, side="left"))
        if j >= start.size or start[j] == L - 1:  # no piece left to trigger the test, or it is the last byte
            out.append((int(start[p]), L - int(start[p]), int(text_before[-1] - text_before[p])))
            return out
        out.append((int(start[p]), int(start[j] - start[p]), int(text_before[j] - text_before[p])))
        p = j


def part_crcs(data, level):
    """([block CRC per part], combined CRC) by the rule above."""
    crcs = [crc32(bytes(data[a:a + n])) for a, n, _ in parts(data, level)]
    comb = 0
    for c in crcs:
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ c
    return crcs, comb


def stream_crcs(stream):
    """([block CRC per bzip2 block], combined CRC) read out of a bzip2 stream:
    the 48-bit block magic is looked for at every bit offset (blocks are not
    byte aligned); the combined CRC is the stream's last 32 bits before the
    padding, found behind the end magic."""
    from bz2_craft import EOS_MAGIC
    big = int.from_bytes(stream, "big")
    nbits = 8 * len(stream)

    def find_all(magic):
        pat, hits = magic.to_bytes(6, "big"), []
        for sh in range(8):  # the stream shifted left by sh bits: a magic at bit 8 k + sh is at byte k
            s = ((big << sh) & ((1 << nbits) - 1)).to_bytes(len(stream), "big")
            k = s.find(pat)
            while k >= 0:
                hits.append(8 * k + sh)
                k = s.find(pat, k + 1)
        return sorted(hits)

    blocks = [get_bits(stream, p + 48, 32) for p in find_all(BLOCK_MAGIC)]
    end = find_all(EOS_MAGIC)[-1]
    return blocks, get_bits(stream, end + 48, 32)


# ---------------------------------------------------------------- the cases --
def run_free(n, seed=1):
    """n bytes in which no byte equals its neighbour (RLE1 leaves them alone)."""
    # random non-zero steps mod 240: values 5..244, so never 3, 4 or 0xFC,
    # the bytes the cases put next to it
    rng = np.random.default_rng(seed)
    return (5 + np.cumsum(rng.integers(1, 240, n, dtype=np.int64)) % 240).astype(np.uint8).tobytes()


def level1_cases():
    """[(id, bytes)]: the cut edges at level 1 (nblockMAX 99 981)."""
    rng = np.random.default_rng(2)
    c = []
    for n in (99980, 99981, 99982, 99983, 99984, 199962, 199963, 199964):
        c.append(("runfree-%d" % n, run_free(n)))
    for pre in range(99973, 99984):  # a chain of 255-byte pieces straddling the cut
        c.append(("chain-%d" % pre, run_free(pre) + bytes([0xFC]) * 1000 + run_free(5000, seed=3)))
    for pre in range(99973, 99982):  # the last-byte edge: the block reaches nblockMAX + 5
        c.append(("last1-%d" % pre, run_free(pre) + bytes([0xFC]) * 6 + bytes([3])))
        c.append(("last2-%d" % pre, run_free(pre) + bytes([0xFC]) * 6 + bytes([3, 4])))
    c.append(("draw-00012", rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), 600000).tobytes()))
    c.append(("zeros-then-0to3", bytes(300000) + rng.integers(0, 4, 400000, dtype=np.uint8).tobytes()))
    c.append(("random-250000", rng.integers(0, 256, 250000, dtype=np.uint8).tobytes()))
    return c
