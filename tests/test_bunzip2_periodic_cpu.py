"""The host side of the GPU decode of periodic bzip2 blocks
(lfm_set_bunzip2_periodic): a model of the rule the kernel follows (n steps
from origPtr go round the start's cycle of the LF permutation; its q bytes
repeated to n are the text) against the texts and against the reference
library, the premises of tests/test_bunzip2_periodic_gpu.py, and the switch.
No GPU."""
import os
import subprocess
import sys

import pytest

import bz2_cases as K
import bz2_craft as C
import bz2_periodic_cases as P


@pytest.fixture(scope="module")
def bz(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


def test_rotations_is_the_crafts_sort():
    for text in (b"q", b"ab" * 7, K.noruns(43, 3, 200) * 3, K.noruns(300, 5), bytes([5]) * 5, b"abaabbab"):
        assert P.rotations(text) == C.sorted_rotations(text), text[:8]


def test_model_on_libbzip2s_periodic_streams(bz):
    """periodic_inputs after RLE1, with the origPtr libbzip2 itself wrote
    (whichever of the equal rows its sort left first): the start's cycle is
    one period long and its bytes repeated to n are the text."""
    for d, period in zip(K.periodic_inputs(), (2, 2, 4, 251)):
        text = C.rle1(d)
        assert C.is_periodic(text)
        stream = bz.compress(d, 1)
        orig = C.parse(stream)["orig"]
        assert orig in P.tied_origs(text, period)
        q, out = P.model(text, orig)
        assert q == period and out == text, len(d)
        assert bz.decompress(stream, len(d)) == d


def test_model_on_every_tied_origptr(bz):
    """repeated_cases: w w and w w w with each origPtr that names one of the
    equal rows, as crafted streams; the model gives the text and libbzip2
    decompresses the stream to it."""
    for text, stream, _ in K.repeated_cases():
        assert C.rle1(text) == text
        q, out = P.model(text, C.parse(stream)["orig"])
        assert len(text) % q == 0 and len(text) // q in (2, 3) and out == text
        assert bz.decompress(stream, len(text)) == text


def test_wrong_start_row(bz):
    """An origPtr in range that names a row of another rotation: the model
    (and so libbzip2's walk) gives that rotation, not the text, and libbzip2
    answers with a data error (the block CRC)."""
    text, stream, out = P.wrong_start()
    assert out != text and out == text[1:] + text[:1]
    assert C.crc32(out) != C.crc32(text)
    with pytest.raises(Exception):
        bz.decompress(stream, len(text))


def test_seam_cases_are_what_the_gpu_test_says(bz):
    """Every seam text is periodic and RLE1 leaves it alone, the model gives
    it back for the crafted origPtr and libbzip2 decompresses the stream to
    it; the start cycles hold segments longer than kWalkKeep, one of them
    between shorter ones."""
    cases = P.seam_cases()
    names = [name for name, _, _ in cases]
    assert len(names) == len(set(names))
    for m in P.SEAM_MS:
        assert "m%d_r2_o0" % m in names and "m%d_r3_o2" % m in names
    assert "m1300_r7_o6" in names and "m513_r7_o0" in names and "m2_r4500_o0" in names
    for name, text, stream in cases:
        data = text  # (ninuse1_n5: nine bytes whose RLE1 text is 5 5 5 5 5)
        text = C.rle1(data)
        assert len(data) < P.SEAM_STRIDE and C.is_periodic(text), name
        q, out = P.model(text, C.parse(stream)["orig"])
        assert q < len(text) and out == text, name
        assert bz.decompress(stream, len(data)) == data, name
    by = {name: (text, stream) for name, text, stream in cases}
    text, stream = by["m1300_r2_o1"]
    assert P.segments(text, C.parse(stream)["orig"]) == [1300]
    text, stream = by["long_segment"]
    seg = P.segments(text, C.parse(stream)["orig"])
    assert sum(seg) == 3000 and max(seg) > P.KEEP and min(seg) < P.MARK and len(seg) > 4
    assert P.model(C.rle1(by["ninuse1_n5"][0]), 0) == (1, bytes([5]) * 5)
    text, stream = by["m2_r4500_o0"]
    assert P.model(text, C.parse(stream)["orig"])[0] == 2


def test_switch_default_setter_and_environment(lfmlib):
    assert lfmlib.get_bunzip2_periodic() is False  # the default
    L = lfmlib.lib()
    try:
        assert lfmlib.set_bunzip2_periodic(True) is False
        assert lfmlib.get_bunzip2_periodic() is True
        assert L.lfm_hip_bunzip2_get_periodic() == 1  # one switch, two names
        assert L.lfm_hip_bunzip2_set_periodic(0) == 1
        assert lfmlib.get_bunzip2_periodic() is False
        assert lfmlib.set_bunzip2_periodic(7) is False
        assert L.lfm_get_bunzip2_periodic() == 1
        assert lfmlib.set_bunzip2_periodic(False) is True
    finally:
        lfmlib.set_bunzip2_periodic(False)
    assert not lfmlib.missing_exports()
    # the environment's default, in a fresh process (the library reads it once)
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); "
            "print(L.lfm_get_bunzip2_periodic(), L.lfm_hip_bunzip2_get_periodic())")
    for value, want in (("1", "1 1"), ("0", "0 0"), (None, "0 0")):
        env = {k: v for k, v in os.environ.items() if k != "LFM_BUNZIP2_PERIODIC"}
        if value is not None:
            env["LFM_BUNZIP2_PERIODIC"] = value
        r = subprocess.run([sys.executable, "-c", code, lfmlib.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])
