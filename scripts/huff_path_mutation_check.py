"""Mutation check of tests/test_huff_heap_path_cpu.py, on the CPU: builds
tests/c/huff_heap_main.cpp against copies of csrc/lfm_huff_heap.h with one
edit each and reports whether the program fails, as it must.
usage: python scripts/huff_path_mutation_check.py > profiles/huff_path_mutation_check.txt"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_huff_heap_path_cpu as T  # noqa: E402

HEADER = os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd", "csrc", "lfm_huff_heap.h")
MUTATIONS = [
    ("none (the header as committed)", None, None),
    ("the pref clear on pop dropped",
     "    heap_pref_set_any(m, nHeap >> 1, 0u);\n", ""),
    ("<= for < in the mask (heap_wless)",
     "    return (a | (Ent)1023) < b;", "    return (a | (Ent)1023) <= (b | (Ent)1023);"),
    ("the sibling recompute skipped after a push that climbed (only the first step's position kept)",
     "        if (z >= 2u) {\n            const Ent right = z & 1u ? v : sib",
     "        if (z >= 2u && z == from) {\n            const Ent right = z & 1u ? v : sib"),
]


def main():
    text = open(HEADER).read()
    ok = True
    for name, old, new in MUTATIONS:
        with tempfile.TemporaryDirectory() as d:
            src = text
            if old is not None:
                assert src.count(old) == 1, name
                src = src.replace(old, new)
            open(os.path.join(d, "lfm_huff_heap.h"), "w").write(src)
            exe = os.path.join(d, "huff_heap_main")
            sanitized = T.build_program(exe, inc=d)
            out = T.run_program(exe)
            first = (out.stdout.strip().splitlines() or out.stderr.strip().splitlines() or [""])[0]
            failed = out.returncode != 0
            want = old is not None
            ok = ok and failed == want
            print("%-28s %s" % ("mutation:", name))
            print("%-28s exit %d (%s), sanitizers %s: %s" % ("", out.returncode, "FAILS" if failed else "passes",
                                                           "on" if sanitized else "off", first))
            print("%-28s %s" % ("", "as it must" if failed == want else "UNEXPECTED"))
    print("verdict: %s" % ("every variant fails the CPU test, the committed header passes" if ok else "NOT as expected"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
