"""The host side of the multi-block GPU bzip2 decoder (lfm_hip_bunzip2_*_multi,
lfm_set_bunzip2_multiblock): slot bound, workspace sizes and the switch, and
the premises of tests/test_bunzip2_multiblock_gpu.py against the reference
library on the host: every input has the part count the GPU test states, every
crafted bad stream is one libbzip2 rejects.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bz2_multi_cases as M
import bz2_parts


@pytest.fixture(scope="module")
def bz(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


def encoder_bound(stride, level):
    """max_parts of csrc/lfm_bz_caps.h, restated."""
    return (stride + stride // 4 + 1) // (100000 * level - 19) + 1


@pytest.mark.parametrize("stride,level,parts", [(147456, 2, 1), (95000, 1, 2), (250000, 1, 4), (250000, 2, 2),
                                                (700000, 1, 9), (1048576, 9, 2)])
def test_max_parts_is_the_encoders_bound(lfmlib, stride, level, parts):
    assert lfmlib.bunzip2_max_parts(stride, level) == parts == encoder_bound(stride, level)


def test_max_parts_and_workspace_refuse_bad_levels(lfmlib):
    L = lfmlib.lib()
    for level in (0, 10):
        assert lfmlib.bunzip2_max_parts(147456, level) == 0
        assert L.lfm_hip_bunzip2_workspace_bytes_multi(3, 147456, level) == 0


@pytest.mark.parametrize("stride,level", [(9008, 1), (65536, 1), (147456, 2)])
def test_one_part_workspace_is_the_single_entrys(lfmlib, stride, level):
    L = lfmlib.lib()
    assert lfmlib.bunzip2_max_parts(stride, level) == 1
    for count in (1, 3):
        assert L.lfm_hip_bunzip2_workspace_bytes_multi(count, stride, level) == \
            L.lfm_hip_bunzip2_workspace_bytes(count, stride) > 0


def test_workspace_grows_with_the_parts(lfmlib):
    """Slots, not streams, size the multi workspace: per slot one block of the
    level (ll + tt alone are 5 bytes per text byte)."""
    L = lfmlib.lib()
    one = L.lfm_hip_bunzip2_workspace_bytes_multi(2, 95000, 1)   # 2 parts
    nine = L.lfm_hip_bunzip2_workspace_bytes_multi(2, 700000, 1)  # 9 parts
    assert one >= 2 * 2 * 5 * 100000 and nine >= 2 * 9 * 5 * 100000
    assert 4 * one < nine < 5 * one


def test_switch_default_setter_and_environment(lfmlib):
    assert lfmlib.get_bunzip2_multiblock() is True  # the default
    try:
        assert lfmlib.set_bunzip2_multiblock(False) is True
        assert lfmlib.get_bunzip2_multiblock() is False
        assert lfmlib.set_bunzip2_multiblock(True) is False
        assert lfmlib.get_bunzip2_multiblock() is True
    finally:
        lfmlib.set_bunzip2_multiblock(True)
    # the environment's default, in a fresh process (the library reads it once)
    code = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).lfm_get_bunzip2_multiblock())"
    for value, want in (("0", "0"), ("1", "1"), (None, "1")):
        env = {k: v for k, v in os.environ.items() if k != "LFM_BUNZIP2_MULTIBLOCK"}
        if value is not None:
            env["LFM_BUNZIP2_MULTIBLOCK"] = value
        r = subprocess.run([sys.executable, "-c", code, lfmlib.LIB_PATH], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])


def test_part_counts_of_the_gpu_inputs(lfmlib):
    """What test_bunzip2_multiblock_gpu.py states about its inputs."""
    counts = {name: len(bz2_parts.parts(d, 1)) for name, d in bz2_parts.level1_cases()}
    assert len(counts) == 40 and set(counts.values()) == {1, 2, 3, 5, 6}
    assert max(counts.values()) <= lfmlib.bunzip2_max_parts(700000, 1) == 9
    assert max(len(d) for _, d in bz2_parts.level1_cases()) <= 700000
    assert len(bz2_parts.parts(M.random_bytes(450000, 450000), 2)) == 3 == lfmlib.bunzip2_max_parts(450001, 2)
    assert len(bz2_parts.parts(M.random_bytes(1000000, 1000000), 9)) == 2 == lfmlib.bunzip2_max_parts(1000003, 9)
    rows = M.mixed_rows()
    assert [len(bz2_parts.parts(r, 1)) for r in rows] == [3, 1, 3, 4, 3]
    assert bz2_parts.parts(rows[4], 1)[0][2] == 3 * 33327  # 33 327 x "abc": periodic
    assert lfmlib.bunzip2_max_parts(250000, 1) == 4
    assert len(bz2_parts.parts(M.random_bytes(250000, 4), 1)) == 3 > lfmlib.bunzip2_max_parts(250000, 2) == 2
    d = bz2_parts.run_free(120001)
    assert [n for _, n, _ in bz2_parts.parts(d, 1)] == [99981, 20020]
    assert lfmlib.bunzip2_max_parts(120000, 1) == lfmlib.bunzip2_max_parts(120001, 1) == 2
    assert lfmlib.bunzip2_max_parts(M.TWO_PART_STRIDE, 1) == 2


def test_reference_library_reads_the_good_and_rejects_the_bad(bz):
    data, stream, facts = M.two_part(bz.compress)
    assert bz.decompress(stream, len(data)) == data
    assert bz2_parts.stream_crcs(stream)[0] == facts["crc"]
    bad = M.bad_two_part(bz.compress)
    assert [n for n, _, _ in bad] == ["crc2_and_combined", "combined_alone", "block2_magic", "eos_magic",
                                      "trunc_in_block2", "orig2_eq_n2"]
    assert [f for _, _, f in bad] == [2, 1, 1, 1, 1, 1]
    for name, s, _ in bad:
        assert s != stream and s[:4] == stream[:4], name
        with pytest.raises(Exception):
            bz.decompress(s, len(data))
    # the patches are where they claim to be
    by = {n: s for n, s, _ in bad}
    assert bz2_parts.stream_crcs(by["crc2_and_combined"])[0] == [facts["crc"][0], facts["crc"][1] ^ 0x00010000]
    assert len(M.find_magic(by["block2_magic"], M.BLOCK_MAGIC)) == 1
    assert M.find_magic(by["eos_magic"], M.EOS_MAGIC) == []
    assert 8 * len(by["trunc_in_block2"]) > facts["block"][1] + 48 + 32 + 1 + 24
    assert M.get_bits(by["orig2_eq_n2"], facts["block"][1] + 81, 24) == facts["n2"] == 519


def test_engine_inputs_are_multi_block(oracle):
    """The two engine files of the GPU test: streams of several bzip2 blocks."""
    runs4 = np.repeat(np.arange(190000 // 4, dtype=np.uint32) % 251, 4).astype(np.uint8)
    assert len(bz2_parts.parts(runs4[:95000].tobytes(), 1)) == 2
    assert len(bz2_parts.parts(np.tile(np.array([3, 7], np.uint8), 47500).tobytes(), 1)) == 1
