"""The bucket pass's word-level rotation classifier, without a GPU.

A NumPy model of the classifier at G = 4 and G = 8 positions per lane,
written from its description: a lane holds positions k .. k + G - 1 and the
bytes after them; it forms the masks T[p] < T[p + 1] and T[p] == T[p + 1] over
its positions and its lookahead, and propagates the type through equal
neighbours from the right; a position whose next 8 comparisons are all
"equal" (9 equal bytes in a row) is undecided and sends the stream through
the sort whole.  Types are decided cyclically over the wrap n - 1 -> 0.  The
model is checked against placed_types and kernel_mode of
test_bwt_induce_compact_cpu.

The C++ classifier itself (csrc/lfm_bwt_types.h, host-callable) is checked
against the byte loop by a stand-alone program, tests/c/bwt_types_main.cpp,
which this file compiles and runs as a child process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_bwt_induce_compact_cpu as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOK = 8  # comparisons that decide a type, at the most


def lane_types(T, G):
    """(is_b[n], undecided[n]) by the word-level classifier with G positions
    per lane.  A lane sees its G bytes and the LOOK bytes after them: G + LOOK
    - 1 comparisons.  The type of the byte past its window is unknown to it
    (taken as A); it can only reach a position that is undecided."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    is_b = np.zeros(n, bool)
    und = np.zeros(n, bool)
    for k in range(0, n, G):
        valid = min(G, n - k)
        w = T[(k + np.arange(G + LOOK)) % n].astype(np.int16)
        lt, eq = w[:-1] < w[1:], w[:-1] == w[1:]
        b = np.zeros(G + LOOK, bool)  # b[G + LOOK - 1]: past the window
        for j in range(G + LOOK - 2, -1, -1):
            b[j] = lt[j] or (eq[j] and b[j + 1])
        for j in range(valid):
            und[k + j] = eq[j:j + LOOK].all()
        is_b[k:k + valid] = b[:valid]
    return is_b, und


def lane_mode(T, G):
    """The mode the bucket pass picks from the classifier's types."""
    is_b, und = lane_types(T, G)
    if und.any():
        return M.FULL
    nb = int(is_b.sum())
    return M.SORT_A if nb * 8 >= (len(T) - nb) * 7 else M.SORT_B


def check_text(T, G):
    T = np.asarray(T, np.uint8)
    is_b, und = lane_types(T, G)
    want_a = M.placed_types(T)  # in plain bytes the scan places the A rotations
    assert np.array_equal(is_b[~und], ~want_a[~und])
    mode = M.kernel_mode(T)
    assert (mode == M.FULL) == bool(und.any())
    assert lane_mode(T, G) == mode
    if mode != M.FULL:
        # the sorted rotations of the mode, and the live rule from the masks:
        # T[p - 1] <= T[p] is the "less or equal" comparison of the position before
        _, placed = M.scan_view(T, mode)
        assert np.array_equal(placed, is_b if mode == M.SORT_A else ~is_b)
        prev = np.roll(T, 1)
        le_before = np.roll((T < np.roll(T, -1)) | (T == np.roll(T, -1)), 1)
        ge_before = np.roll(~(T < np.roll(T, -1)), 1)
        assert np.array_equal(M.live_rule(T, mode), le_before if mode == M.SORT_A else ge_before)
        assert np.array_equal(prev <= T, le_before)
    return mode


def run_texts(G):
    """Equal runs of 2 .. 12 bytes ending at every offset of a group of G
    positions, followed by a smaller and by a larger byte, inside the text and
    with the run's end at the text's last position (decided across the wrap)."""
    for run in range(2, 13):
        for off in range(G):
            for larger in (False, True):
                for at_end in (False, True):
                    n = 6 * G + off + 1 if at_end else 12 * G + 3
                    rng = np.random.default_rng(run * 100 + off * 4 + larger * 2 + at_end)
                    T = (1 + (np.cumsum(rng.integers(1, 90, n)) % 90)).astype(np.uint8)  # no equal neighbours
                    last = n - 1 if at_end else 4 * G + off
                    if last - run + 1 < 1:
                        continue
                    T[last - run + 1:last + 1] = 100
                    T[(last + 1) % n] = 101 if larger else 99
                    T[last - run] = 120
                    assert last % G == off and not M.is_periodic(T)
                    yield run, T


@pytest.mark.parametrize("G", [4, 8])
def test_model_on_random_texts(G):
    """Seeded random non-periodic texts, alphabets of 2 .. 256 symbols (small
    alphabets make long equal runs: kModeFull texts are among them)."""
    modes = set()
    for T in M.random_texts(1500, 0xB0C + G):
        if len(T) >= LOOK:  # (kernel_mode looks 8 bytes ahead)
            modes.add(check_text(T, G))
    assert modes == {M.SORT_A, M.SORT_B, M.FULL}


@pytest.mark.parametrize("G", [4, 8])
def test_model_on_the_stream_shapes(G):
    for name, raw, want in M.shapes(5000):
        T = M.rle1(raw)
        mode = check_text(T, G)
        assert want is None or mode == want, name


@pytest.mark.parametrize("G", [4, 8])
def test_model_on_equal_runs_at_every_offset(G):
    """A run of 9 or more equal bytes is undecided at its first positions, a
    shorter one is decided by the byte after it, wherever it ends in a group."""
    seen = set()
    for run, T in run_texts(G):
        mode = check_text(T, G)
        assert (mode == M.FULL) == (run >= 9), run
        seen.add((run, int(np.flatnonzero(T == 100)[-1]) % G if T[-1] != 100 else (len(T) - 1) % G))
    assert {r for r, _ in seen} == set(range(2, 13)) and {o for _, o in seen} == set(range(G))


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_cpp_classifier_matches_the_byte_loop(tmp_path):
    """tests/c/bwt_types_main.cpp: bwt_types8 against the byte loop on random
    texts, 16-bit symbols, equal runs of 2 .. 12 bytes at every offset, constant
    texts, every group phase, the wrap included; with the address and
    undefined-behaviour sanitizers where the compiler links them."""
    cxx = _compiler()
    assert cxx, "no C++ compiler"
    src = os.path.join(REPO, "tests", "c", "bwt_types_main.cpp")
    inc = os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd", "csrc")
    exe = str(tmp_path / "bwt_types_main")
    base = [cxx, "-std=c++17", "-O1", "-I" + inc, src, "-o", exe]
    san = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode != 0:  # no sanitizer runtime here: the plain build still checks the classifier
        subprocess.run(base, check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr, "(sanitizers: %s)" % (san.returncode == 0))
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    groups, undecided = map(int, out.stdout.split()[1:3])
    assert groups > 100000 and undecided > 0
