"""The heap steps of the GPU encoder's Huffman code lengths, without a GPU.

csrc/lfm_huff_heap.h (host-callable: the pref bits, the path sift, pop, push
and the merge loop that huff_lengths_heap runs per lane) is checked by a
stand-alone program, tests/c/huff_heap_main.cpp, which this file compiles and
runs as a child process.  The program holds a plain array restatement of
BZ2_hbMakeCodeLengths and compares code lengths and retry counts for every
alphabet size 3 .. 258, both entry widths (frequencies up to 2^20 for the wide
one) and the shape classes all equal, 0/1, 0..3, random, powers of two with
zeros, ramps and Fibonacci weights; each heap is walked alone, beside a heap of
258 entries and beside one of a random size (the wave's level count).  After
every pop, sift and push it checks each pref bit against its node's children.
It fails if one of its premises was never met: retries, heaps of equal
weights, sifts that stop at level 0, sifts that reach the deepest level,
pushes that climb to the root."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREMISES = ("retries", "equal", "stop0", "deepest", "rootpush")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def build_program(exe, inc=None):
    """Compiles tests/c/huff_heap_main.cpp against the header in `inc`, with
    the address and undefined-behaviour sanitizers where the compiler links
    them; returns whether it did."""
    cxx = _compiler()
    assert cxx, "no C++ compiler"
    src = os.path.join(REPO, "tests", "c", "huff_heap_main.cpp")
    inc = inc or os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd", "csrc")
    base = [cxx, "-std=c++17", "-O2", "-I" + inc, src, "-o", exe]
    san = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode != 0:  # no sanitizer runtime here: the plain build still checks the heap steps
        subprocess.run(base, check=True, capture_output=True, text=True)
    return san.returncode == 0


def run_program(exe):
    return subprocess.run([exe], capture_output=True, text=True, timeout=240)


def test_heap_steps_match_the_restatement(tmp_path):
    exe = str(tmp_path / "huff_heap_main")
    sanitized = build_program(exe)
    out = run_program(exe)
    print(out.stdout, out.stderr, "(sanitizers: %s)" % sanitized)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    words = out.stdout.split()
    counts = {k: int(v) for k, v in zip(words[1::2], words[2::2])}
    assert counts["heaps"] >= 256 * 2 * 14 * 3
    for k in PREMISES:
        assert counts[k] > 0, k
