"""The multi-GPU reader's host side, without a device: the new exports, their
prototypes against the binding's argtypes, the two new structs against the C
compiler's layout, the shard plan (lfm_decode_shard_plan) on real headers, the
LFM_DECODE_GPUS parse, and lfm_decode_memory_multi with no device list: one
plain decode, exact, workers == 1."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include", "lfm")
NEW = ["lfm_set_decode_devices", "lfm_get_decode_devices", "lfm_default_decode_devices", "lfm_release_decoders",
       "lfm_decode_shard_plan", "lfm_decode_memory_multi", "lfm_decode_memory_multi_device"]


def test_exports(lfmlib):
    L = lfmlib.lib()
    assert lfmlib.missing_exports() == []
    for name in NEW:
        assert name in lfmlib.EXPORTS and hasattr(L, name), name
    for name in ("set_decode_devices", "get_decode_devices", "default_decode_devices", "release_decoders",
                 "decode_shard_plan", "decode_multi", "decode_device_sharded"):
        assert callable(getattr(lfmlib, name)), name
    assert L.lfm_api_version() == 2


def prototype(name):
    """(return type, parameter declarations) of `name` in lfm_api.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, "lfm_api.h")).read(), flags=re.S)
    m = re.search(r"LFM_API\s+(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in lfm_api.h" % name
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_prototypes_match_argtypes(lfmlib):
    L = lfmlib.lib()
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    intp, u32p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)
    msp, shp = ctypes.POINTER(lfmlib.DecodeMultiStats), ctypes.POINTER(lfmlib.DecodeShard)
    want = {
        "lfm_set_decode_devices": ("int", [intp, ci], ["const int* devices", "int n"]),
        "lfm_get_decode_devices": ("int", [intp, ci], ["int* devices", "int cap"]),
        "lfm_default_decode_devices": ("int", [ci, intp, ci], ["int n_visible", "int* devices", "int cap"]),
        "lfm_release_decoders": ("void", [], ["void"]),
        "lfm_decode_shard_plan": ("int", [vp, u64, ci, intp, u32p, u32p, ci],
                                  ["const uint8_t* buf", "uint64_t len", "int nworkers", "int* axis",
                                   "uint32_t* first", "uint32_t* count", "int cap"]),
        "lfm_decode_memory_multi": ("int", [vp, u64, vp, ci, msp, shp, ci],
                                    ["const uint8_t* buf", "uint64_t len", "void* img", "int numThreads",
                                     "lfm_decode_multi_stats* stats", "lfm_decode_shard* shards", "int shard_cap"]),
        "lfm_decode_memory_multi_device": ("int", [vp, u64, ctypes.POINTER(vp), ctypes.POINTER(u64), ci, ci, msp, shp, ci],
                                           ["const uint8_t* buf", "uint64_t len", "void* const* d_out",
                                            "const uint64_t* out_bytes", "int nshards", "int numThreads",
                                            "lfm_decode_multi_stats* stats", "lfm_decode_shard* shards",
                                            "int shard_cap"]),
    }
    assert sorted(want) == sorted(NEW)
    for name, (ret, argtypes, decl) in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is (None if ret == "void" else ctypes.c_int), name
        assert prototype(name) == (ret, decl), name


SHARD_FIELDS = ["first", "count", "device", "rc", "stats"]
MULTI_FIELDS = ["total_ms", "axis", "workers", "blocks", "host_blocks", "d2h_bytes"]


def test_struct_layouts(lfmlib, tmp_path):
    """ctypes' DecodeShard and DecodeMultiStats have the size and the field
    offsets the C compiler gives lfm_decode_shard and lfm_decode_multi_stats."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>\n#include "lfm_api.h"\nint main(void) {\n']
    for struct, fields in (("lfm_decode_shard", SHARD_FIELDS), ("lfm_decode_multi_stats", MULTI_FIELDS)):
        lines.append('printf(" %%zu", sizeof(%s));\n' % struct)
        lines += ['printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields]
    src.write_text("".join(lines) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for S, fields in ((lfmlib.DecodeShard, SHARD_FIELDS), (lfmlib.DecodeMultiStats, MULTI_FIELDS)):
        assert [f for f, _ in S._fields_] == fields
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want
    assert sorted(lfmlib.DecodeMultiStats().as_dict()) == sorted(MULTI_FIELDS)
    assert sorted(lfmlib.DecodeShard().as_dict()) == sorted(SHARD_FIELDS)


# ------------------------------------------------------------ shard plan --
@pytest.fixture(scope="module")
def headers(oracle):
    """Uncompressed files of the writer tests' shapes (tests/test_multigpu_gpu.py):
    only their headers are read."""
    vid = oracle.synthetic_lf(200, 96, Z=20, T=13, seed=0x4C464D0A)
    bs = [64, 32, 3, 1, 1]
    out = {
        "video": oracle.encode(vid, header_version=0x80 | (8 + 4), nnum=13, block_size=bs, compression=0),
        "still": oracle.encode(vid, header_version=8 + 4, nnum=13, block_size=bs, compression=0),
        # video, but predictor 0: nothing temporal to keep together
        "video_k0": oracle.encode(vid, header_version=0x80 | 8, nnum=13, block_size=bs, compression=0),
        "default": oracle.encode(oracle.synthetic_lf(300, 200, Z=20, T=15, seed=0x4C464D0B), header_version=8 + 4,
                                 nnum=15, compression=0),
    }
    for name, (tn, c) in (("t3c2", (3, 2)), ("t1c3", (1, 3))):
        img = oracle.synthetic_lf(128, 100, Z=5, C=c, Tn=tn, T=13, seed=0x4C464D0C)
        out[name] = oracle.encode(img, header_version=0x80 | (8 + 4), nnum=13, block_size=[64, 64, 2, 1, 1],
                                  compression=0)
    assert oracle.parse_header(out["video"])["header_version"] == 0x80 | 4
    assert oracle.parse_header(out["video_k0"])["header_version"] == 0x80
    return out


def check_plan(lfmlib, oracle, buf, n):
    """The invariants of every plan; returns (axis, shards)."""
    h = oracle.parse_header(buf)
    axis, shards = lfmlib.decode_shard_plan(buf, n)
    dim, unit = h["xyzct"][axis], h["block_size"][axis]
    assert axis == (4 if h["xyzct"][4] > 1 else 3 if h["xyzct"][3] > 1 else 2)
    assert 1 <= len(shards) <= max(1, n)
    assert shards[0][0] == 0 and sum(c for _, c in shards) == dim
    for (f0, c0), (f1, _) in zip(shards, shards[1:]):
        assert c0 > 0 and f1 == f0 + c0              # disjoint, contiguous
    for f, c in shards:
        assert f % unit == 0 and c > 0               # whole block layers
    assert lfmlib.decode_shard_plan(buf, len(shards)) == (axis, shards)  # idempotent
    return axis, shards


def test_plan_video_pairs_of_layers(lfmlib, oracle, headers):
    """Predicted video, block depth 3: shards begin on even z, in pairs of layers."""
    buf = headers["video"]
    assert check_plan(lfmlib, oracle, buf, 2) == (2, [(0, 12), (12, 8)])
    assert check_plan(lfmlib, oracle, buf, 3) == (2, [(0, 12), (12, 8)])
    assert check_plan(lfmlib, oracle, buf, 5) == (2, [(0, 6), (6, 6), (12, 6), (18, 2)])
    assert check_plan(lfmlib, oracle, buf, 4) == (2, [(0, 6), (6, 6), (12, 6), (18, 2)])
    for n in (1, 2, 3, 4, 5, 7, 50):
        assert all(f % 2 == 0 for f, _ in check_plan(lfmlib, oracle, buf, n)[1]), n


def test_plan_is_the_writers_split(lfmlib, oracle, headers):
    """No video bit (or no predictor): the writer's split, per = ceil(7 / 5) = 2 layers."""
    for name in ("still", "video_k0"):
        assert check_plan(lfmlib, oracle, headers[name], 5) == (2, [(0, 6), (6, 6), (12, 6), (18, 2)]), name
        assert check_plan(lfmlib, oracle, headers[name], 2) == (2, [(0, 12), (12, 8)]), name
        assert check_plan(lfmlib, oracle, headers[name], 7)[1] == [(3 * w, 3 if w < 6 else 2) for w in range(7)], name
    axis, shards = check_plan(lfmlib, oracle, headers["default"], 3)
    assert axis == 2 and [c for _, c in shards] == [8, 8, 4]


def test_plan_5d(lfmlib, oracle, headers):
    assert check_plan(lfmlib, oracle, headers["t3c2"], 2) == (4, [(0, 2), (2, 1)])
    assert check_plan(lfmlib, oracle, headers["t3c2"], 3) == (4, [(0, 1), (1, 1), (2, 1)])
    assert check_plan(lfmlib, oracle, headers["t1c3"], 2) == (3, [(0, 2), (2, 1)])


def test_plan_more_workers_than_layers(lfmlib, oracle, headers):
    assert len(check_plan(lfmlib, oracle, headers["video"], 50)[1]) == 4
    assert len(check_plan(lfmlib, oracle, headers["still"], 50)[1]) == 7
    assert len(check_plan(lfmlib, oracle, headers["t3c2"], 8)[1]) == 3
    for n in (1, 0, -3):
        assert lfmlib.decode_shard_plan(headers["still"], n) == (2, [(0, 20)]), n


def test_plan_bad_header(lfmlib, headers):
    L = lfmlib.lib()
    buf = headers["still"]
    assert L.lfm_decode_shard_plan(buf, 10, 2, None, None, None, 0) == 0
    assert L.lfm_decode_shard_plan(None, 0, 2, None, None, None, 0) == 0
    assert L.lfm_decode_shard_plan(buf, len(buf), 2, None, None, None, 0) == 2  # (the count alone)
    with pytest.raises(lfmlib.LfmError):
        lfmlib.decode_shard_plan(buf[:10], 2)


# ----------------------------------------------------------- device list --
def test_default_decode_devices(lfmlib, monkeypatch):
    monkeypatch.delenv("LFM_DECODE_GPUS", raising=False)
    monkeypatch.setenv("LFM_GPUS", "0,1")  # the writers' list is not the readers'
    assert lfmlib.default_decode_devices(8) == []
    assert lfmlib.get_decode_devices() == []
    for value, n, want in (("0,1,1,3", 4, [0, 1, 1, 3]), ("0,0,0", 1, [0, 0, 0]), ("3", 8, [0, 1, 2]), ("8", 2, [0, 1]),
                           ("0,9,1", 4, [0, 1]), ("2,", 4, [2]), ("", 4, []), ("0,1", 0, [])):
        monkeypatch.setenv("LFM_DECODE_GPUS", value)
        assert lfmlib.default_decode_devices(n) == want, (value, n)
    monkeypatch.delenv("LFM_DECODE_GPUS")
    assert lfmlib.default_decode_devices(8) == []
    L = lfmlib.lib()
    assert L.lfm_set_decode_devices(None, 2) == 3 and L.lfm_set_decode_devices(None, -1) == 3
    assert L.lfm_set_decode_devices((ctypes.c_int * 1)(1 << 20), 1) == 3  # no such device
    assert L.lfm_set_decode_devices(None, 0) == 0
    assert lfmlib.get_decode_devices() == []


# ------------------------------------------------- no list: a plain decode --
def test_decode_multi_without_a_list(lfmlib, oracle, monkeypatch):
    """With no decode device list (the default) lfm_decode_memory_multi is one
    plain decode: the exact image, workers == 1, one shard over the whole axis."""
    monkeypatch.delenv("LFM_DECODE_GPUS", raising=False)
    lfmlib.set_decode_devices(None)
    vid = oracle.synthetic_lf(70, 90, Z=5, T=2, seed=0x4C464D22)
    u8 = np.random.default_rng(31).integers(0, 7, (1, 1, 3, 33, 50), dtype=np.uint8)
    for img, buf in ((vid, oracle.encode(vid, header_version=0x80 | (8 + 4), nnum=2, block_size=[32, 32, 1, 1, 1])),
                     (vid, oracle.encode(vid, header_version=8 + 4, nnum=2, compression=0)),
                     (u8, oracle.encode(u8, data_type=0, block_size=[16, 16, 2, 1, 1]))):
        got, st = lfmlib.decode_multi(buf, return_stats=True)
        assert got.dtype == img.dtype and np.array_equal(got, img)
        assert np.array_equal(lfmlib.decode(buf), img)
        h = oracle.parse_header(buf)
        assert st["workers"] == 1 and st["axis"] == 2 and st["blocks"] == h["nb"], st
        assert len(st["shards"]) == 1, st
        sh = st["shards"][0]
        assert (sh["first"], sh["count"], sh["rc"]) == (0, h["xyzct"][2], 0), st
        assert sh["stats"]["blocks"] == h["nb"] and sh["stats"]["staged_bytes"] == 0, st
    L = lfmlib.lib()
    out = np.empty(vid.shape, np.uint16)
    assert L.lfm_decode_memory_multi(None, 0, out.ctypes.data, 1, None, None, 0) == 3
    assert L.lfm_decode_memory_multi(buf, len(buf), None, 1, None, None, 0) == 3
    assert L.lfm_decode_memory_multi(buf[:10], 10, out.ctypes.data, 1, None, None, 0) != 0
    assert L.lfm_decode_memory_multi_device(buf, len(buf), None, None, 2, 1, None, None, 0) == 3
    lfmlib.release_decoders()  # (nothing was started: a no-op)
