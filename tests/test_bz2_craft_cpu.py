"""The premises of tests/test_bunzip2_gpu.py, checked on the host: every
crafted stream declared good decompresses to its input with libbzip2 (the
reference's bzip2-1.0.6 when oracle/_ref is built, else the system library),
every one declared bad is rejected, and each case still sits on the edge it
was made for."""
import numpy as np
import pytest

import bz2_cases as K
import bz2_craft as C


@pytest.fixture(scope="module")
def bz(oracle):
    return oracle.bzip2()


def test_writer_parts():
    assert C.crc32(b"123456789") == 0xFC891918  # CRC-32/BZIP2 check value
    assert C.rle1(b"a" * 3 + b"b" * 4 + b"c" * 259 + b"d") == b"aaabbbb\x00cccc\xfbcccc\x00d"
    assert C.rle1(b"e" * 256) == b"eeee\xfbe" and C.rle1(b"f" * 510) == b"ffff\xfbffff\xfb"
    assert C.assign_codes([2, 1, 3, 3]) == [2, 0, 6, 7]
    s = C.patch_bits(b"\x00\x00\x00", 5, 10, 0x2AB)
    assert C.get_bits(s, 5, 10) == 0x2AB and C.get_bits(s, 0, 5) == 0 and C.get_bits(s, 15, 9) == 0
    assert C.is_periodic(b"abab") and not C.is_periodic(b"ababa") and C.is_periodic(b"zz")


def test_writer_matches_library_header(bz):
    """parse() and set_crcs() on libbzip2's own streams; craft() round trips."""
    rng = np.random.default_rng(3)
    for n in (1, 50, 700, 3000):
        data = rng.integers(0, 7, n, dtype=np.uint8).tobytes()
        ref = bz.compress(data, 1)
        p = C.parse(ref)
        assert p["crc"] == C.crc32(data) and p["ninuse"] == len(set(C.rle1(data)))
        stream, info = C.craft(data, level=1)
        assert bz.decompress(stream, n) == data
        assert p["orig"] == info["orig"] and p["ngroups"] == info["ngroups"] and p["nsel"] == info["nsel"]
        assert C.set_crcs(ref, p["crc"]) == ref
        with pytest.raises(Exception):
            bz.decompress(C.set_crcs(ref, p["crc"] ^ 1), n)


def test_sweep_premises(bz):
    inputs = K.sweep_inputs()
    streams = [bz.compress(d, 1) for d in inputs]
    assert {C.parse(s)["ngroups"] for s in streams} == {2, 3, 4, 5, 6}
    starts = np.cumsum([0] + [len(s) for s in streams])[:-1]
    assert {int(o) % 4 for o in starts} == {0, 1, 2, 3}
    assert max(len(d) for d in inputs) <= 9001


@pytest.mark.parametrize("fill", [0, 360])
def test_rle_seam_premises(fill):
    inputs = K.rle_seam_inputs(fill)
    assert len(inputs) == 48
    ns = [len(C.rle1(d)) for d in inputs]
    assert (max(ns) < 1024) if fill == 0 else (2900 < min(ns) and max(ns) < 3100)
    for k, d in enumerate(inputs):
        t = C.rle1(d)
        # the run encodings, count bytes equal to the run's byte among them, at offset k (+ the fill)
        assert t[k:k + 5] == bytes(5) and bytes([5]) * 5 in t and bytes([251]) * 5 in t
        assert b"BBBB\xfbBBBB\x00" in t and b"CCCC\xfbCCCC\xfb" in t and b"AAAA\xfbA" in t and t.endswith(b"DDDD\x03")
    # the decoder cuts the text into 64 segments of seg bytes: over the 48 values of k every one
    # of the five machine states (4: the next byte is a count) is met at the start of a segment
    seg = {((n + 63) // 64 + 15) // 16 * 16 for n in ns}
    assert seg == ({16} if fill == 0 else {48})
    seg = seg.pop()
    at_seam = set()
    for d in inputs:
        t, state, prev = C.rle1(d), 0, -1
        for i, c in enumerate(t):
            if i and i % seg == 0:
                at_seam.add(state)
            state = 0 if state == 4 else (state + 1 if state and c == prev else 1)
            prev = c
    assert at_seam == {0, 1, 2, 3, 4}


def test_marker_premises(bz):
    cases = K.marker_cases()
    assert len(cases) == sum((n + 127) // 128 for n in K.MARKER_NS)
    rows = set()
    for text, stream, info in cases:
        assert C.rle1(text) == text and info["n"] == len(text)
        assert info["v0"] % 128 == 0
        rows.add((info["n"], info["v0"]))
        assert bz.decompress(stream, len(text)) == text
    assert rows == {(n, 128 * m) for n in K.MARKER_NS for m in range((n + 127) // 128)}


def test_periodic_premises():
    for d in K.periodic_inputs():
        assert C.is_periodic(C.rle1(d)) and not C.is_periodic(C.rle1(d + d[:1]))


def test_repeated_premises(bz):
    """w w and w w w: periodic, valid for libbzip2 with every origPtr that names one of the equal
    rows, and for each text one of those makes a chain that only counts segments and bytes wrap."""
    cases = K.repeated_cases()
    for text, stream, _ in cases:
        assert C.is_periodic(text) and C.rle1(text) == text
        assert bz.decompress(stream, len(text)) == text
        assert bz.decompress(bz.compress(text, 1), len(text)) == text
    wrapping = {}
    for text, _, wraps in cases:
        wrapping[text] = wrapping.get(text, 0) + wraps
    assert len(wrapping) == 5 and all(v == 1 for v in wrapping.values())
    assert {(len(t) <= 128, len(t) > 128) for t in wrapping} == {(True, False), (False, True)}
    assert not K.chain_wraps(K.noruns(300, 9, 50), 7) and not K.chain_wraps(b"ab" * 300, 0)


def test_crafted_good_premises(bz):
    cases = {name: (data, stream, info) for name, data, stream, info, _ in K.crafted_good()}
    for name, (data, stream, info) in cases.items():
        assert bz.decompress(stream, len(data)) == data, name
    for g in range(2, 7):
        i = cases["groups%d" % g][2]
        assert i["ngroups"] == g and i["nsym"] > 50 * g and i["maxlen"] == 5 + g - 1
    assert cases["all20"][2]["minlen"] == 20
    assert cases["len17to20"][2]["minlen"] >= 17 and cases["len17to20"][2]["maxlen"] >= 18
    assert cases["flat9"][2]["minlen"] == cases["flat9"][2]["maxlen"] == 9
    assert cases["nsym_mod50_0"][2]["nsym"] % 50 == 0 and cases["nsym_mod50_1"][2]["nsym"] % 50 == 1
    assert any(nd >= 3 and a // 50 != (a + nd - 1) // 50 for a, nd in cases["run_straddle"][2]["runs"])
    assert cases["ninuse1_n1"][2]["ninuse"] == 1 and cases["ninuse1_n1"][2]["n"] == 1
    assert cases["ninuse1_n5"][2]["ninuse"] == 1 and cases["ninuse1_n5"][2]["text"] == bytes([5]) * 5
    assert cases["ninuse2"][2]["ninuse"] == 2 and not C.is_periodic(cases["ninuse2"][2]["text"])
    assert cases["ninuse256"][2]["ninuse"] == 256 and cases["ninuse256"][2]["maxpos"] == 255
    i = cases["extra_sel5"][2]
    assert i["nsel"] == (i["nsym"] + 49) // 50 + 5
    # what the device is expected to decode is not periodic (a periodic text cannot be walked as one cycle)
    for name, data, stream, info, on_device in K.crafted_good():
        assert on_device == (name not in ("ninuse1_n5", "extra_sel5")), name
        if on_device and info["n"] > 1:
            assert not C.is_periodic(info["text"]), name


def test_crafted_bad_premises(bz):
    cases = K.crafted_bad()
    assert len({name for name, _, _ in cases}) == len(cases) >= 16
    for name, stream, flag in cases:
        with pytest.raises(Exception):
            bz.decompress(stream, 4096)
    # the two CRC cases fail on the CRC alone: with the CRC of what they decode to, libbzip2 accepts them
    data = K.noruns(300, 9, 50)
    _, info = C.craft(data, ngroups=2)
    wrong = (info["orig"] + 1) % info["n"]
    twin, _ = C.craft(data, ngroups=2, orig_override=wrong)
    r = C.sorted_rotations(data)[wrong]
    rotated = data[r:] + data[:r]
    assert bz.decompress(C.set_crcs(twin, C.crc32(rotated)), 4096) == rotated
