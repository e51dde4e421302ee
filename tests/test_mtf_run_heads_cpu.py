"""The premises of mtf_win's run-head walk, on the reference library's own
streams (no GPU): a position of the BWT column that repeats its predecessor
has move-to-front value 0 and leaves the list alone, so the values at the run
heads are the move-to-front of the head subsequence; and every row of
tests/bz2_mtf_run_cases.py puts on the kernel's seams what its id names."""
import numpy as np
import pytest

import bz2_encode_cases as C
import bz2_mtf_run_cases as R


def _rows():
    return [("run",) + c for c in R.cases()] + [("D",) + c for c in C.mtf_cases()]


ROWS = _rows()


@pytest.mark.parametrize("row", ROWS, ids=["%s:%s" % (r[0], r[1]) for r in ROWS])
def test_values_at_heads_are_the_mtf_of_the_heads(row):
    _, cid, raw, witness = row
    d = C.ref_dissect(raw)
    col, vals, _ = R.column_and_values(d)
    heads = R.heads_of(col)
    assert not vals[~heads].any(), "a repeat with a non-zero value"
    order = list(d["used"])
    got = []
    for c in col[heads].tolist():
        v = order.index(c)
        got.append(v)
        order.insert(0, order.pop(v))
    assert got == vals[heads].tolist()
    print(cid, "positions", len(col), "heads", int(heads.sum()), "per segment", R.heads_per_segment(col))


@pytest.mark.parametrize("case", R.cases(), ids=[c[0] for c in R.cases()])
def test_witness_holds(case):
    cid, raw, witness = case
    assert 4096 <= len(raw) <= 41000
    facts = witness(raw, C.ref_dissect(raw))
    print(cid, facts)


def test_list_covers_the_seams():
    """The ids the GPU module relies on are there, each once, and the mixed
    batch's rows share a length."""
    ids = [c[0] for c in R.cases()]
    assert len(set(ids)) == len(ids) == 12
    assert set(R.MIXED) <= set(ids) and len(R.mixed_batch()) == len(R.MIXED)
    assert sorted(len(raw) % R.S for cid, raw, _ in R.cases() if cid.startswith("last-segment")) == [1, 63, 65]
