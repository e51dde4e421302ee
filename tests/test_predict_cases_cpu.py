"""The forward predictor's case lists (tests/predict_cases.py) are what they
claim, shown without a GPU:

1. with a forced piece count lfm.predict_plan (pure then: no HIP call) equals
   the planner model for every case, family and predictor, so the model can
   stand for the planner below;
2. the lists reach every class of seam they name;
3. every case input tells a broken seam from a sound one: a stale halo left
   of a strip start, stale rows above a piece start and a temporal frame's P
   from the wrong frame each change the oracle's symbols in at least one
   predictor of every family."""
import numpy as np
import pytest

import predict_cases as pc


@pytest.fixture(autouse=True)
def automatic_pieces_afterwards(lfmlib):
    yield
    lfmlib.predict_set_pieces(0)


def forced(c):
    """The case's forced piece counts (the automatic one needs a device)."""
    return [p for p in c.pieces if p] or [1]


def model_launches(cases, fams=pc.FAMS):
    """(case, family, pieces, launch) of every forced plan of the cases."""
    for c in cases:
        for fam in fams:
            for pieces in forced(c):
                for L in pc.model_plan(c.W, c.H, c.n, c.T, fam, 1, c.video, c.z0, c.cands, True, pieces):
                    yield c, fam, pieces, L


def v_cases():
    return [c for T in pc.V_T for g in pc.V_GROUPS for c in pc.list_v(T, g)]


def p_cases():
    return [c for T in pc.V_T for W in pc.P_WIDTHS for H in pc.p_heights(T) for c in pc.list_p(T, W, H)]


def r_cases():
    return [c for T in pc.R_T for W in pc.R_WIDTHS for c in pc.list_r(T, W)] + pc.list_r_xcd()


def c_cases():
    return [c for T in pc.C_T for c in pc.list_c(T)] + pc.list_c_xcd()


def g_cases():
    return [c for T in pc.G_T for c in pc.list_g(T)]


# ------------------------------------------------------ 1. model == query --
def test_plan_query_equals_model_for_every_case(lfmlib):
    checked = 0
    for c in pc.all_cases():
        for pieces in forced(c):
            lfmlib.predict_set_pieces(pieces)
            for fam in pc.FAMS:
                for k in range(1, 8):
                    got = lfmlib.predict_plan(c.W, c.H, c.n, c.T, fam, k, c.video, c.z0, c.cands, True)
                    assert got == pc.model_plan(c.W, c.H, c.n, c.T, fam, k, c.video, c.z0, c.cands, True, pieces), \
                        (pc.case_id(c), fam, k, pieces)
                    checked += 1
                # any base that is not 16-byte aligned: generic, whatever the shape
                got = lfmlib.predict_plan(c.W, c.H, c.n, c.T, fam, 4, c.video, c.z0, c.cands, False)
                assert got == pc.model_plan(c.W, c.H, c.n, c.T, fam, 4, c.video, c.z0, c.cands, False, pieces)
                assert {L["kernel"] for L in got} == {"generic"} and len(got) == (7 if c.cands else 1)
    assert checked > 50000


def test_plan_query_details(lfmlib):
    """Predictor 0 is a copy; refused arguments; the override returns the
    previous value and 0 restores the automatic count."""
    assert lfmlib.predict_set_pieces(3) == 0
    assert lfmlib.predict_set_pieces(-5) == 3      # negative counts mean automatic
    assert lfmlib.predict_set_pieces(2) == 0
    assert lfmlib.predict_plan(520, 131, 3, 13, "tiles", 0, 1, 1) == pc.model_plan(520, 131, 3, 13, "tiles", 0, 1, 1)
    assert lfmlib.predict_plan(520, 131, 3, 13, "tiles", 0)[0]["kernel"] == "copy"
    for bad in ((0, 4, 1, 13, "tiles", 1), (4, 0, 1, 13, "tiles", 1), (8, 8, 0, 13, "tiles", 1),
                (8, 8, 1, 0, "tiles", 1), (8, 8, 1, 13, 3, 1), (8, 8, 1, 13, "tiles", 8)):
        with pytest.raises(lfmlib.LfmError):
            lfmlib.predict_plan(*bad)
    assert lfmlib.predict_set_pieces(0) == 2
    # production, config 3: with the automatic count and no device the planner assumes 256 CUs
    # of one workgroup; the shape fields do not depend on that
    plan = lfmlib.predict_plan(2048, 2048, 64, 15, "tiles", 4, 1, 0)
    assert pc.device_free(plan) == pc.device_free(pc.model_plan(2048, 2048, 64, 15, "tiles", 4, 1, 0))


# ----------------------------------------------------------- 2. classes ----
def strip_class(W, L):
    rest = W % L["strip"]
    return "exact" if rest == 0 else "one-lane" if rest == 8 else "partial"


def prefetch_depth(c, L):
    """PD, from R = rows_per_step * (PD + 1) + T + 1."""
    return (L["R"] - c.T - 1) // L["rows_per_step"] - 1


def test_lists_reach_every_named_class():
    strips, tiles_strip, tiles_rest, starts, steps, xcd = {}, {}, set(), {}, {}, {}
    roles, halo_reach = set(), set()
    lists = v_cases() + p_cases() + r_cases() + c_cases()
    for c, fam, pieces, L in model_launches(lists):
        kern = L["kernel"]
        assert kern == {"V": "vec", "R": "ring", "C": "cands"}.get(c.lst, kern), (pc.case_id(c), fam)
        strips.setdefault(kern, set()).add(strip_class(c.W, L))
        xcd.setdefault(kern, set()).add(L["xcd_map"])
        if fam == "tiles":
            tiles_strip.setdefault(kern, set()).add(L["strip"])
            if kern == "vec":
                tiles_rest.add(c.W % 1024)
        pd = prefetch_depth(c, L)
        for ys, ye in pc.pieces_of(L, c.H):
            n = -(-(ye - ys) // L["rows_per_step"])
            steps.setdefault(kern, set()).add({-1: "<PD", 0: "PD", 1: "PD+1"}.get(max(-1, n - pd), "other"))
            if ys:
                starts.setdefault(kern, set()).add(ys % c.T == 0)
        roles.add(pc.launch_role(c, L))
        halo_reach.add((kern, L["halo"], c.T + 1))
    everything = {"exact", "one-lane", "partial"}
    assert strips["vec"] == everything and strips["ring"] == everything and strips["cands"] == everything
    assert strips["vec_pair"] == {"one-lane", "partial"}        # list P's widths: 504, 520, 1032
    assert tiles_strip["vec"] == {1024} and tiles_strip["vec_pair"] == {512}
    # tiles, 1024-pixel strips: the second wave of the last strip wholly outside the frame, or all but one lane
    assert {512, 520, 0, 8} <= tiles_rest
    for kern in ("vec", "ring", "cands"):
        assert starts[kern] == {True, False}, kern
        assert {"<PD", "PD+1"} <= steps[kern], kern
    assert {"<PD", "PD"} <= steps["vec_pair"] and starts["vec_pair"]
    for kern in ("vec", "vec_pair", "ring", "cands"):
        assert xcd[kern] == {0, 1}, kern
    assert {"temporal-first", "pairs", "spatial-last"} <= roles
    assert ("cands", 16, 16) in halo_reach       # predict_ring's code at T = 15: reach = halo
    assert ("vec", 16, 16) in halo_reach and ("vec_pair", 16, 16) in halo_reach
    assert ("ring", 32, 32) in halo_reach and ("cands", 32, 32) in halo_reach
    assert ("ring", 32, 17) in halo_reach        # T = 16, the first halo of 32
    # (1, 1): the lone temporal frame, the only way into predict_vec's own P ring
    lone = [L for c, fam, pieces, L in model_launches(p_cases()) if (c.n, c.z0) == (1, 1)]
    assert lone and all(L["kernel"] == "vec" and L["RP"] > 0 for L in lone)
    assert {c.W for c in p_cases() if (c.n, c.z0) == (1, 1)} == set(pc.P_WIDTHS)
    # list G and the candidates' two extra shapes never leave the generic kernel
    for c, fam, pieces, L in model_launches(g_cases() + pc.list_c_generic()):
        assert L["kernel"] == "generic", pc.case_id(c)
    # list A: fast when aligned
    for c, kernels in pc.A_CASES:
        for fam in pc.FAMS:
            plan = pc.model_plan(c.W, c.H, c.n, c.T, fam, 1, c.video, c.z0, c.cands, True, 1)
            assert tuple(L["kernel"] for L in plan) == kernels


# ------------------------------------------------------- 3. sensitivity ----
def seams_of(c):
    """Strip starts (xs, halo), piece starts ys and temporal frames z (of the
    whole stack) over every family's forced plans of the case."""
    cols, rows = set(), set()
    for _, fam, pieces, L in model_launches([c]):
        if L["strip"]:
            cols |= {(s * L["strip"], L["halo"]) for s in range(1, L["nstrip"])}
            rows |= {ys for ys, _ in pc.pieces_of(L, c.H) if ys}
    temporal = [z for z in range(1, c.n + c.z0) if c.video and z & 1 and z >= c.z0]
    return sorted(cols), sorted(rows), temporal


def check_sensitive(oracle, cases):
    n = 0
    for c in cases:
        cols, rows, temporal = seams_of(c)
        for kind in pc.INPUTS:
            full = pc.case_input(oracle, c, kind)
            good = {}   # the oracle's symbols of the input, shared by its seams
            for xs, halo in cols:
                assert pc.stale_columns_missed(oracle, c, full, xs, halo, good) == [], (pc.case_id(c), kind, "xs", xs)
            for ys in rows:
                assert pc.stale_rows_missed(oracle, c, full, ys, good) == [], (pc.case_id(c), kind, "ys", ys)
            for z in temporal:
                assert pc.wrong_previous_missed(oracle, c, full, z) == [], (pc.case_id(c), kind, "z", z)
            n += len(cols) + len(rows) + len(temporal)
    return n


@pytest.mark.parametrize("T", pc.V_T)
def test_inputs_tell_broken_seams_vec_and_pairs(oracle, T):
    cases = [c for g in pc.V_GROUPS for c in pc.list_v(T, g)]
    cases += [c for W in pc.P_WIDTHS for H in pc.p_heights(T) for c in pc.list_p(T, W, H)]
    assert check_sensitive(oracle, cases) > 100


@pytest.mark.parametrize("T", pc.R_T)
def test_inputs_tell_broken_seams_ring(oracle, T):
    assert check_sensitive(oracle, [c for W in pc.R_WIDTHS for c in pc.list_r(T, W)]) > 50


@pytest.mark.parametrize("T", pc.C_T)
def test_inputs_tell_broken_seams_cands(oracle, T):
    assert check_sensitive(oracle, pc.list_c(T)) >= 12


def test_inputs_tell_broken_seams_xcd_shapes_and_alignment(oracle):
    assert check_sensitive(oracle, pc.list_c_xcd() + pc.list_r_xcd() + [c for c, _ in pc.A_CASES]) > 20


def test_carry_stack_is_what_it_says():
    s = pc.carry_stack(6, 12, 16)
    assert (s[1] == 0xFFFF).all() and (s[2] == 0).all() and np.array_equal(s[3], ~s[0]) and (s[4] == 0xFFFF).all()
    assert (s[0, 0] == 0x8000).all() and (s[0, 1] == 0x7FFF).all() and (s[0, 2] == 0x8000).all()
    assert s[0, 3].tolist() == [0, 0xFFFF] * 8 and s[0, 5].tolist() == [0, 0xFFFF] * 8
    assert (s[0, 6] == 0x8000).all() and (s[0, 7] == 0x7FFF).all()
