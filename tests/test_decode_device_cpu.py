"""The device-destination decode's host side, without a device: argument
validation of lfm.decode_device / decode_roi_device / crop_device, the new
exports and their ctypes signatures against include/lfm, and the layout of
lfm_decode_stats against the C compiler's."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include", "lfm")
FIELDS = ["total_ms", "path", "chunks", "blocks", "host_blocks", "d2h_bytes", "staged_bytes"]


@pytest.fixture(scope="module")
def small_file(oracle):
    img = oracle.synthetic_lf(40, 24, Z=2, T=13, seed=3)
    return img, oracle.encode(img, header_version=8 + 4, nnum=13, block_size=[16, 16, 1, 1, 1])


def test_argument_validation(lfmlib, small_file):
    import torch
    img, buf = small_file
    for bad in (b"", buf[:10], buf[:42]):
        with pytest.raises(ValueError):
            lfmlib.decode_device(bad)
        with pytest.raises(ValueError):
            lfmlib.decode_roi_device(bad, [0] * 5, [0] * 5)
    unknown = bytearray(buf)
    unknown[42] = 77  # no such KLB data type
    with pytest.raises(ValueError):
        lfmlib.decode_device(bytes(unknown))
    # destinations that are not CUDA tensors are refused before any device call
    for out in (np.empty(img.shape, np.uint16), torch.empty(img.shape, dtype=torch.int16), [0] * img.size):
        with pytest.raises(ValueError):
            lfmlib.decode_device(buf, out=out)
        with pytest.raises(ValueError):
            lfmlib.decode_roi_device(buf, [0] * 5, [3, 3, 0, 0, 0], out=out)
    for lb, ub in (([0] * 5, [40, 0, 0, 0, 0]), ([2, 0, 0, 0, 0], [1, 0, 0, 0, 0]), ([0] * 5, [0, 0, 2, 0, 0]),
                   ([0] * 4, [0] * 4), ([-1, 0, 0, 0, 0], [0] * 5)):
        with pytest.raises(ValueError):
            lfmlib.decode_roi_device(buf, lb, ub)
    with pytest.raises(ValueError):
        lfmlib.decode_device(buf, device="cpu")
    with pytest.raises(ValueError):
        lfmlib.crop_device(0, [4, 4, 1, 1], [0] * 5, [1] * 5, 2, 0)
    with pytest.raises(ValueError):
        lfmlib.crop_device(0, [4, 4, 1, 1, 1], [0] * 5, [1, 1, 1, 1, 1 << 32], 2, 0)


def test_c_functions_refuse_bad_arguments(lfmlib, small_file):
    """Checks the library makes before it touches a device: no buffer, no
    header, a region outside the image, a destination too small."""
    img, buf = small_file
    L = lfmlib.lib()
    u5 = ctypes.c_uint32 * 5
    host = np.empty(img.shape, np.uint16)
    assert L.lfm_decode_memory_device(None, 0, host.ctypes.data, host.nbytes, 1, None) == 3
    assert L.lfm_decode_memory_device(buf, len(buf), None, host.nbytes, 1, None) == 3
    assert L.lfm_decode_memory_device(buf[:10], 10, host.ctypes.data, host.nbytes, 1, None) != 0
    assert L.lfm_decode_memory_device(buf, len(buf), host.ctypes.data, host.nbytes - 1, 1, None) == 3
    assert L.lfm_decode_memory_roi_device(buf, len(buf), None, None, host.ctypes.data, host.nbytes, 1, None) == 3
    assert L.lfm_decode_memory_roi_device(buf, len(buf), u5(0, 0, 0, 0, 0), u5(40, 0, 0, 0, 0), host.ctypes.data,
                                          host.nbytes, 1, None) == 3
    assert L.lfm_decode_memory_roi_device(buf, len(buf), u5(0, 0, 0, 0, 0), u5(9, 9, 1, 0, 0), host.ctypes.data,
                                          10 * 10 * 2 * 2 - 1, 1, None) == 3
    # the region copy checks its box on the host
    assert L.lfm_hip_crop_region(None, u5(4, 4, 1, 1, 1), u5(0, 0, 0, 0, 0), u5(1, 1, 1, 1, 1), 2, None, None) == 1
    for dims, lb, n, bpp in (((4, 4, 1, 1, 1), (3, 0, 0, 0, 0), (2, 1, 1, 1, 1), 2),
                             ((4, 4, 1, 1, 1), (0, 0, 0, 0, 0), (1, 0, 1, 1, 1), 2),
                             ((4, 4, 1, 1, 1), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), 2),
                             ((4, 4, 1, 1, 1), (0xFFFFFFFF, 0, 0, 0, 0), (2, 1, 1, 1, 1), 2),
                             ((4, 4, 1, 1, 1), (0, 0, 0, 0, 0), (1, 1, 1, 1, 1), 3),
                             ((4, 4, 1, 1, 1), (0, 0, 0, 0, 0), (1, 1, 1, 1, 1), 16)):
        assert L.lfm_hip_crop_region(1 << 20, u5(*dims), u5(*lb), u5(*n), bpp, 1 << 21, None) == 1, (dims, lb, n, bpp)


def prototype(header, name):
    """The parameter list of `name` in a header, comments removed, as a list of C declarations."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in %s" % (name, header)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_exports_and_signatures(lfmlib):
    L = lfmlib.lib()
    assert lfmlib.missing_exports() == []
    vp, u64, u32p = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)
    stp = ctypes.POINTER(lfmlib.DecodeStats)
    want = {
        "lfm_decode_memory_device": ("lfm_api.h", [vp, u64, vp, u64, ctypes.c_int, stp],
                                     ["const uint8_t* buf", "uint64_t len", "void* d_img", "uint64_t d_img_bytes",
                                      "int numThreads", "lfm_decode_stats* stats"]),
        "lfm_decode_memory_roi_device": ("lfm_api.h", [vp, u64, u32p, u32p, vp, u64, ctypes.c_int, stp],
                                         ["const uint8_t* buf", "uint64_t len", "const uint32_t lb[KLB_DATA_DIMS]",
                                          "const uint32_t ub[KLB_DATA_DIMS]", "void* d_out", "uint64_t out_bytes",
                                          "int numThreads", "lfm_decode_stats* stats"]),
        "lfm_hip_crop_region": ("lfm_hip.h", [vp, u32p, u32p, u32p, ctypes.c_uint32, vp, vp],
                                ["const void* d_src", "const uint32_t src_dims[5]", "const uint32_t lb[5]",
                                 "const uint32_t n[5]", "uint32_t bpp", "void* d_dst", "void* stream"]),
    }
    for name, (header, argtypes, decl) in want.items():
        assert name in lfmlib.EXPORTS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == argtypes, name
        assert getattr(L, name).restype is ctypes.c_int, name
        assert prototype(header, name) == decl, name
    assert L.lfm_api_version() == 2


def test_decode_stats_layout(lfmlib, tmp_path):
    """ctypes' DecodeStats has the size and the field offsets the C compiler
    gives lfm_decode_stats."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "lfm_api.h"\n'
                   'int main(void) { printf("%zu", sizeof(lfm_decode_stats));\n'
                   + "".join('printf(" %%zu", offsetof(lfm_decode_stats, %s));\n' % f for f in FIELDS)
                   + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = lfmlib.DecodeStats
    assert [f for f, _ in S._fields_] == FIELDS
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert sorted(S().as_dict()) == sorted(FIELDS)
