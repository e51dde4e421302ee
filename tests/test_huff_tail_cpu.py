"""The Huffman stage outside the merge trips, without a GPU.

Two stand-alone programs, compiled here (with the address and
undefined-behaviour sanitizers where the compiler links them) and run as child
processes:

tests/c/sel_mtf_main.cpp: csrc/lfm_sel_mtf.h, the selector move-to-front of
huff_final as a scan of run summaries, against the serial move-to-front of
compress.c -- every sequence of length 0 .. 7 over six symbols, random
sequences up to 18 002 selectors with 2 to 6 tables, every chunk length 1 .. 64
at stream lengths around each multiple of the wave pass, associativity of the
compose on random triples.  It fails if it never met a chunk with all six
symbols, a chunk of one repeated symbol, or a carry across a pass.

tests/c/huff_insert_main.cpp: heap_insert_levels of csrc/lfm_huff_heap.h, the
level-wise initial inserts of huff_lengths_heap, against sequential UPHEAP,
entry by entry, for every alphabet size 3 .. 258, both entry widths and the
shape classes of huff_heap_main.cpp.  It fails if it never met a climb to the
root from the deepest level, a heap without a climb, or a heap whose inserts
all climb to the root."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def build_and_run(name, tmp_path):
    """Compiles tests/c/<name>.cpp and runs it; {counter: value} of its "ok" line."""
    cxx = _compiler()
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / name)
    base = [cxx, "-std=c++17", "-O2", "-I" + INC, os.path.join(REPO, "tests", "c", name + ".cpp"), "-o", exe]
    san = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode != 0:  # no sanitizer runtime here: the plain build still checks the steps
        subprocess.run(base, check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    print(out.stdout, out.stderr, "(sanitizers: %s)" % (san.returncode == 0))
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    words = out.stdout.split()
    return {k: int(v) for k, v in zip(words[1::2], words[2::2])}


def test_selector_mtf_scan_matches_the_serial_walk(tmp_path):
    counts = build_and_run("sel_mtf_main", tmp_path)
    assert counts["sequences"] >= sum(6 ** n for n in range(8)) * 3 + 64 * 14 + 400
    assert counts["triples"] >= 100000
    for k in ("six", "one", "carry"):
        assert counts[k] > 0, k


def test_level_wise_inserts_match_upheap(tmp_path):
    counts = build_and_run("huff_insert_main", tmp_path)
    assert counts["heaps"] == 256 * 2 * 14
    for k in ("deeproot", "noclimb", "allroot"):
        assert counts[k] > 0, k
