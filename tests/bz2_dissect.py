"""A pure-Python reader of single-block bzip2 streams, written from the file
format: it takes a stream apart into what each stage of a compressor wrote,
so that the encoder tests can check a claim such as "this input puts a zero
run on value 16 384" against the stream the reference library wrote, never
against the encoder under test.  TEST INFRASTRUCTURE ONLY (the counterpart of
bz2_craft.py, which writes such streams).

    d = dissect(stream)

d: level, crc (block CRC), ccrc (combined CRC), orig (origPtr), used (sorted
byte values in use), alpha (len(used) + 2), ngroups, nsel, selectors,
sel_mtf (the selectors' move-to-front values as written), lengths (one code
length table per group), syms (the symbol stream: RUNA 0, RUNB 1, value v as
v + 1, EOB alpha - 1, EOB included), hdr_bits (bit offset of the first
symbol), data_end (bit offset of the end magic) and nbits (bit offset of the
stream's end before the padding).

    vals, runs = mvals(d["syms"])   the move-to-front values before the second
                                    run-length step (zeros expanded, EOB
                                    dropped); runs: [(start, length)] of the
                                    zero runs
    col = bwt_column(vals, d["used"])   the inverse move-to-front: the last
                                    column of the sorted rotations
    assemble(d)                     the stream written back from d
"""
import numpy as np

from bz2_craft import BLOCK_MAGIC, EOS_MAGIC, assign_codes

RUNA, RUNB = 0, 1
GROUP = 50


def _bits(stream):
    return bin(int.from_bytes(b"\x01" + bytes(stream), "big"))[3:]


def dissect(stream):
    stream = bytes(stream)
    s = _bits(stream)
    assert stream[:3] == b"BZh" and 1 <= stream[3] - 48 <= 9, "not a bzip2 stream"
    pos = 32

    def take(n):
        nonlocal pos
        v = int(s[pos:pos + n], 2)
        pos += n
        return v

    assert take(48) == BLOCK_MAGIC, "no block magic"
    d = dict(level=stream[3] - 48, crc=take(32))
    assert take(1) == 0, "randomised block"
    d["orig"] = take(24)
    in16 = take(16)
    used = []
    for i in range(16):
        if in16 >> (15 - i) & 1:
            row = take(16)
            used += [16 * i + j for j in range(16) if row >> (15 - j) & 1]
    alpha = len(used) + 2
    d.update(used=used, alpha=alpha, ngroups=take(3), nsel=take(15))
    assert 2 <= d["ngroups"] <= 6 and d["nsel"] >= 1
    order, sel, sel_mtf = list(range(d["ngroups"])), [], []
    for _ in range(d["nsel"]):
        j = 0
        while s[pos] == "1":
            pos, j = pos + 1, j + 1
        pos += 1
        assert j < d["ngroups"]
        sel_mtf.append(j)
        order.insert(0, order.pop(j))
        sel.append(order[0])
    d.update(selectors=sel, sel_mtf=sel_mtf)
    lengths = []
    for _ in range(d["ngroups"]):
        curr, ln = take(5), []
        for _ in range(alpha):
            while s[pos] == "1":
                curr += 1 if s[pos + 1] == "0" else -1
                pos += 2
            pos += 1
            assert 1 <= curr <= 20
            ln.append(curr)
        lengths.append(ln)
    d.update(lengths=lengths, hdr_bits=pos)
    tables = []
    for ln in lengths:
        codes = assign_codes(ln)
        tables.append((min(ln), max(ln), {format(c, "0%db" % l): k for k, (c, l) in enumerate(zip(codes, ln))}))
    syms, eob = [], alpha - 1
    while True:
        assert len(syms) // GROUP < d["nsel"], "symbols past the last selector"
        lo, hi, tab = tables[sel[len(syms) // GROUP]]
        for l in range(lo, hi + 1):
            k = tab.get(s[pos:pos + l])
            if k is not None:
                break
        else:
            raise AssertionError("no code at bit %d" % pos)
        pos += l
        syms.append(k)
        if k == eob:
            break
    assert d["nsel"] == (len(syms) + GROUP - 1) // GROUP
    d.update(syms=syms, data_end=pos)
    assert take(48) == EOS_MAGIC, "no end magic"
    d["ccrc"] = take(32)
    d["nbits"] = pos
    assert len(stream) == (pos + 7) // 8 and "1" not in s[pos:]
    return d


def mvals(syms):
    """(values, zero runs) of a symbol stream that ends in EOB."""
    out, runs, run, w = [], [], 0, 1
    for k in syms[:-1]:
        if k <= RUNB:
            run += w << k  # RUNA adds w, RUNB 2 w
            w <<= 1
            continue
        if run:
            runs.append((len(out), run))
            out += [0] * run
            run, w = 0, 1
        out.append(k - 1)
    if run:
        runs.append((len(out), run))
        out += [0] * run
    return np.array(out, dtype=np.int32), runs


def bwt_column(vals, used):
    """The inverse move-to-front of vals over the sorted byte values `used`
    (an int n stands for range(n)), as a uint8 array."""
    order = list(range(used)) if isinstance(used, int) else list(used)
    out = bytearray()
    for v in vals.tolist():
        if v:
            order.insert(0, order.pop(v))
        out.append(order[0])
    return np.frombuffer(bytes(out), dtype=np.uint8)


def assemble(d):
    """The stream written back from its parts: the header fields, the selectors'
    move-to-front values, the length tables and the symbols as d holds them."""
    out = [format(0x425A6830 + d["level"], "032b"), format(BLOCK_MAGIC, "048b"), format(d["crc"], "032b"), "0",
           format(d["orig"], "024b")]
    rows = [sum(1 << (15 - j) for j in range(16) if 16 * i + j in set(d["used"])) for i in range(16)]
    out.append(format(sum(1 << (15 - i) for i in range(16) if rows[i]), "016b"))
    out += [format(r, "016b") for r in rows if r]
    out += [format(d["ngroups"], "03b"), format(d["nsel"], "015b")]
    out += ["1" * j + "0" for j in d["sel_mtf"]]
    for ln in d["lengths"]:
        curr = ln[0]
        out.append(format(curr, "05b"))
        for l in ln:
            out.append(("10" if l > curr else "11") * abs(l - curr) + "0")
            curr = l
    codes = [[format(c, "0%db" % l) for c, l in zip(assign_codes(ln), ln)] for ln in d["lengths"]]
    out += [codes[d["selectors"][k // GROUP]][sym] for k, sym in enumerate(d["syms"])]
    out += [format(EOS_MAGIC, "048b"), format(d["ccrc"], "032b")]
    s = "".join(out)
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")
