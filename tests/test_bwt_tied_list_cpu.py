"""The premises of test_bwt_tied_list_gpu.py, without a GPU: every call of
tests/bwt_tied_list_cases.py hits the seams it is listed for -- chunk lengths
per sorter class, the in-chunk slot and length of its tied runs, the run that
holds rotation 0, runs in several chunks and streams, the run of 33 that sends
the call through the sorts a second time -- all recomputed from the first-round
model of bz2_sort_cases.py; the calls together hit every seam of `required()`;
and each call's place path is the one its seams imply."""
import pytest

import bwt_tied_list_cases as C
import bz2_place_cases as P
import bz2_sort_cases as S

IDS = [c[0] for c in C.CASES]


def case_labels(cid):
    (c,) = [c for c in C.CASES if c[0] == cid]
    per_stream = [C.labels(fam, seed) for fam, seed in c[1]]
    lab = set().union(*per_stream)
    if sum(1 for fam, seed in c[1] if C.runs_of(C.first_round_of(fam, seed)[2])) >= 3:
        lab.add("streams3")
    return lab, per_stream


def test_shape_of_the_calls():
    assert C.CASES
    for cid, streams, _ in C.CASES:
        assert 1 <= len(streams) <= 8 and all(C.FAMILIES[fam][1] <= 20000 for fam, _ in streams), cid
        assert len({len(r) for r in C.rows_of(cid)}) == 1
        assert all(len(set(r)) <= 6 for r in C.rows_of(cid)), "a small alphabet"


@pytest.mark.parametrize("cid", IDS)
def test_case_hits_its_seams(cid):
    (c,) = [c for c in C.CASES if c[0] == cid]
    lab, per_stream = case_labels(cid)
    print(cid, sorted(lab))
    assert all(per_stream), "a stream leaves the device or the three sorters"
    assert set(c[2]) <= lab, sorted(set(c[2]) - lab)


@pytest.mark.parametrize("cid", IDS)
def test_case_path(cid):
    """Fused, unless the call holds the run of 33: then exactly one run is
    left, beside streams whose ties settle, and the whole batch is placed
    after a text round (no restart)."""
    (c,) = [c for c in C.CASES if c[0] == cid]
    m = C.model_of(cid)
    st = m["stats"]
    assert not any(m["host"]) and st["chunks_segmented"] == 0 and st["first_ties"] > 0
    if "run33" in c[2]:
        assert st["left_runs"] == 1 and st["restarted"] == 0 and st["text_rounds"] >= 1
        assert P.place_path(st) == P.WHOLE
        settled = [s for s in range(len(c[1])) if m["rounds"][s]["first_ties"] and not m["rounds"][s]["left_runs"]]
        assert len(settled) >= 2
    else:
        assert st["left_runs"] == 0 and P.place_path(st) == P.FUSED


def test_every_seam_is_hit():
    hit = set()
    for cid in IDS:
        (c,) = [c for c in C.CASES if c[0] == cid]
        hit |= set(c[2])
    assert C.required() <= hit, sorted(C.required() - hit)
    print("len=4096 (a single-bucket chunk of exactly 4 096):", "found" if "len=4096" in hit else "not found")


def test_control_restarts():
    st = S.model_of(C.CONTROL)["stats"]
    assert st["restarted"] == 1 and P.place_path(st) == P.NONE
