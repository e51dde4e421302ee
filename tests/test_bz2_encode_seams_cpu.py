"""The premises of test_bzip2_seams_gpu.py, without a GPU: bz2_dissect reads
streams correctly (what bz2_craft wrote; what the reference library wrote,
written back bit for bit), every case of bz2_encode_cases passes its witness
against the reference library's stream, stays non-periodic and below
nblockMAX (so the GPU tests may demand flags == 0 of every row), and the
geometry the cases aim at is the kernels'."""
import os
import random
import re

import pytest

import bz2_encode_cases as C
from bz2_craft import craft, crc32, is_periodic, rle1
from bz2_dissect import assemble, bwt_column, dissect, mvals
from bz2_parts import nblock_max
from conftest import PKG
from test_gpu import _bz2_cases


def ref(oracle):
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz


# ------------------------------------------------------------ bz2_dissect --
def _check_crafted(data, **kw):
    stream, info = craft(data, **kw)
    d = dissect(stream)
    assert (d["level"], d["crc"], d["ccrc"], d["orig"]) == (kw.get("level", 9), info["crc"], info["crc"], info["orig"])
    assert d["used"] == sorted(set(info["text"])) and d["alpha"] == info["ninuse"] + 2
    assert (d["ngroups"], d["nsel"], len(d["syms"])) == (info["ngroups"], info["nsel"], info["nsym"])
    assert d["hdr_bits"] == info["bits"]["symbols"] and d["data_end"] == info["bits"]["eos"]
    if "lengths" in kw:
        assert d["lengths"] == [list(ln) for ln in kw["lengths"]]
    if "selectors" in kw:
        assert d["selectors"] == list(kw["selectors"])
    vals, runs = mvals(d["syms"])
    assert len(vals) == info["n"] and len(runs) == len(info["runs"])
    # the column back through the move-to-front, then the text back through the BWT
    col = bwt_column(vals, d["used"])
    n, t2 = info["n"], info["text"] + info["text"]
    rot = sorted(range(n), key=lambda i: t2[i:i + n])
    assert col.tobytes() == bytes(t2[i + n - 1] for i in rot)
    assert assemble(d) == stream
    return d


@pytest.mark.parametrize("ngroups", [2, 3, 4, 5, 6])
def test_dissect_reads_what_craft_wrote(ngroups):
    rnd = random.Random(ngroups)
    data = bytes(rnd.randrange(20) + 60 for _ in range(420)) + bytes([61]) * 9
    alpha = len(set(rle1(data))) + 2
    nsel = -(-craft(data)[1]["nsym"] // 50)
    sel = [rnd.randrange(ngroups) for _ in range(nsel)]
    d = _check_crafted(data, ngroups=ngroups, selectors=sel,
                       lengths=[[5 + (k + t) % 13 for k in range(alpha)] for t in range(ngroups)])
    assert max(max(ln) for ln in d["lengths"]) == 17
    _check_crafted(data, ngroups=ngroups, level=1)
    _check_crafted(data[:1], ngroups=ngroups)


def test_dissect_rewrites_the_reference_streams(oracle):
    """The reference library's stream of every test_gpu._bz2_cases() input that
    is one bzip2 block: taken apart and written back, the same bits; CRC and
    the text length agree with the input."""
    bz = ref(oracle)
    seen = 0
    for name, data in _bz2_cases().items():
        raw = data.tobytes()
        level = 1 if C.text_len(raw) < nblock_max(1) else 2
        if C.text_len(raw) >= nblock_max(level):
            continue
        stream = bz.compress(raw, level)
        d = dissect(stream)
        assert assemble(d) == stream, name
        assert d["crc"] == d["ccrc"] and len(mvals(d["syms"])[0]) == C.text_len(raw), name
        if len(raw) <= 40000:
            assert d["crc"] == crc32(raw), name
        seen += 1
    assert seen == len(_bz2_cases())


def test_rle1_np_is_rle1():
    for _, raw, _ in C.rle1_cases(0)[4096][::7] + C.length_cases()[:80]:
        assert C.rle1_np(raw) == rle1(raw)


# --------------------------------------------------------------- the cases --
@pytest.mark.parametrize("which", ["A", "B", "C", "D", "E", "F"])
def test_every_case_passes_its_witness(oracle, which):
    """... against the reference library; and the GPU tests may demand
    flags == 0: the text is not periodic and shorter than nblockMAX at level 1
    (the geometric row: level 2, where alone it runs)."""
    bz = ref(oracle)
    cases = [c for extra in (0, 1) for c in C.all_cases(extra) if c[0] == which]
    assert cases
    ids = [c[1] for c in C.all_cases(0) if c[0] == which]
    assert len(ids) == len(set(ids))
    seen = set()
    for _, cid, raw, witness in cases:
        if raw in seen:
            continue
        seen.add(raw)
        text = C.rle1_np(raw)
        assert len(text) < nblock_max(2 if cid == "geometric" else 1), cid
        assert not is_periodic(text), cid
        d = None
        if C.NEEDS_REF[which]:
            stream = bz.compress(raw, C.LEVEL)
            assert stream == C.ref_stream(raw)
            d = C.ref_dissect(raw)
        try:
            grouped = which == "B" and len(raw) - (len(raw) & 1) in C.RLE1_ROW.values()
            facts = C.rle1_facts(len(raw) & 1)[cid] if grouped else witness(raw, d)
        except AssertionError as e:
            raise AssertionError("%s:%s %s" % (which, cid, e))
        assert facts, cid


def test_lengths_every_length_survives():
    have = {len(raw) for _, raw, _ in C.length_cases()}
    assert have == set(C.LENGTHS)
    assert 32767 in have and bin(32767 % C.RLE1["TILE"]).count("1") == 14  # every bit of the CRC unshift
    paths = {C.from_img(n, n) for n in have}
    assert paths == {True, False}


def test_rle1_cases_cover_the_stated_edges():
    for extra in (0, 1):
        for n, group in C.rle1_cases(extra).items():
            assert all(len(raw) == n + extra for _, raw, _ in group) and len(group) >= 1
            assert C.from_img(n + extra, n + extra) == (extra == 0)
        facts = C.rle1_facts(extra)
        # the text offset at the run in front of the tile seams takes every value mod 16
        for P in (16384, 32768):
            assert {f["text_offset"] % 16 for cid, f in facts.items() if cid.startswith("P%d-" % P)} == set(range(16))
        tile = {cid: f for cid, f in facts.items() if cid.startswith("P16384-")}
        carried = {f["carried"] for f in tile.values() if "carried" in f}
        assert {1, 2, 3, 4, 5, 222, 223, 224, 225, 254, 0, 1} <= carried
        # the piece reaches 255 at the chunk's last byte, first byte, and one past it
        assert {(f["carried"], f["piece_len"]) for f in tile.values() if "carried" in f} >= {(254, 255), (224, 255), (223, 224)}
        assert tile["P16384-j255-R255"]["run_len"] == 255 and "carried" not in tile["P16384-j255-R255"]
        # runs that end exactly at a chunk end, and at the stream's end
        assert any((f["run_start"] + f["run_len"]) % C.RLE1["CHUNK"] == 0 for f in tile.values())
        last = [f for cid, f in facts.items() if cid.startswith("last-")]
        assert sorted(f["run_len"] for f in last) == [4, 5, 255, 259, 510]
        assert all(f["run_start"] + f["run_len"] == 4096 + extra for f in last)
    solo = {cid: raw for cid, raw, _ in C.rle1_solo_cases()}
    assert len(solo["run4"]) == 4 and len(solo["tiles3+5"]) == 3 * C.RLE1["TILE"] + 5


def test_rle2_cases_cover_the_stated_edges():
    runs = []
    for group in C.rle2_cases().values():
        for cid, raw, witness in group:
            if cid.startswith("pairs"):
                runs += witness(raw, C.ref_dissect(raw))["runs"]
    starts, ends, lens = {s for s, _ in runs}, {s + l for s, l in runs}, {l for _, l in runs}
    for B in C.RLE2_SEAMS:  # PER, WAVE and TILE of rle2
        assert {B - 1, B} <= starts and {B, B + 1} <= ends and {B - 2, B - 1} <= lens, B
    assert any(l > 2 * C.RLE2["TILE"] for l in lens)


def test_mixed_batch_is_mixed(oracle):
    bz = ref(oracle)
    rows = C.mixed_batch()
    img = C.place_blocks(C.MIXED_DIMS, C.MIXED_BS, [raw for _, raw in rows])
    blocks = list(oracle.iter_blocks(C.MIXED_DIMS, C.MIXED_BS))
    assert len(blocks) == len(rows)
    for (i, coord, size), (cid, raw) in zip(blocks, rows):
        assert bytes(oracle.gather_block(img[None, None], coord, size)) == raw, cid
        assert not is_periodic(C.rle1_np(raw)) and C.text_len(raw) < nblock_max(1), cid
    C.mixed_witness([dissect(bz.compress(raw, C.LEVEL)) for _, raw in rows])
    assert {-(-len(raw) // C.RLE1["TILE"]) for _, raw in rows} == {1, 3}
    assert C.from_img(C.MIXED_DIMS[0], C.MIXED_BS[0])


def test_compaction_batch_offsets(oracle):
    bz = ref(oracle)
    C.compaction_witness([bz.compress(raw, C.LEVEL) for raw in C.compaction_batch()])


# ------------------------------------------------------------ the geometry --
def test_geometry_is_the_kernels():
    """The constants the cases restate, read out of the sources: a retune moves
    the cases or fails here."""
    src = open(os.path.join(PKG, "csrc", "lfm_bzip2.hip")).read()
    caps = open(os.path.join(PKG, "csrc", "lfm_bz_caps.h")).read()

    def const(name, text=src):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        return int(m.group(1))
    assert const("kRleChunk") == C.RLE1["CHUNK"]
    assert 64 * const("kRleChunk") == C.RLE1["WAVE"]
    assert const("kRleThreads") * const("kRleChunk") == C.RLE1["TILE"]
    assert re.search(r"kRleTile\s*=\s*kRleThreads\s*\*\s*kRleChunk\s*;", src)
    assert re.search(r"rl0\s*>=\s*%d\s*&&" % C.RLE1["SLOW_FROM"], src)
    assert re.search(r"po\s*=\s*wr0\s*&\s*%d" % (C.RLE1["UNIT"] - 1), src)
    assert const("kSeg") == C.MTF["SEG"]
    assert const("kRle2Per") == C.RLE2["PER"] and 64 * const("kRle2Per") == C.RLE2["WAVE"]
    assert const("kRle2Threads") * const("kRle2Per") == C.RLE2["TILE"]
    assert const("kEmitC") == C.EMIT["PER"] and const("kEmitThreads") * const("kEmitC") == C.EMIT["ROUND"]
    assert const("kGSize", caps) == C.HUFF["GROUP"]
    m = re.search(r"nGroups\s*=\s*nMTF\s*<\s*(\d+)\s*\?\s*2\s*:\s*nMTF\s*<\s*(\d+)\s*\?\s*3\s*:\s*nMTF\s*<\s*(\d+)\s*\?\s*4\s*:"
                  r"\s*nMTF\s*<\s*(\d+)\s*\?\s*5\s*:\s*6", src)
    assert m and tuple(int(x) for x in m.groups()) == C.HUFF["BANDS"]
    # the multi entry takes two slots per stream at MULTI_BLOCK, so its own kernels run
    assert C.max_parts(C.MULTI_BLOCK, 1) == 2 and C.max_parts(C.MULTI_BLOCK - 17, 1) == 1
    fill = C.multi_filler()
    assert len(fill) == C.MULTI_BLOCK and C.text_len(fill) == len(fill) < nblock_max(1) and not is_periodic(fill)
    assert re.search(r"worst\s*/\s*\(100000u\s*\*\s*level\s*-\s*19u\)\)\s*\+\s*1u", caps)
