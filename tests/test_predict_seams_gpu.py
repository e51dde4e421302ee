"""The forward predictor's five kernels (lfm_predict.hip: predict_generic,
predict_ring, predict_cands, predict_vec, predict_vec_pair) at every seam of
their strips, row pieces and frame pairs, bit for bit against the oracle.

Every case (tests/predict_cases.py) first pins what lfm.predict_plan reports
for it: with a forced piece count the whole plan equals the planner model,
with the automatic count (it depends on the device) the kernels and the strip
fields do, and the automatic plan is carried in the assertion messages.  A
change to the dispatch, the kernel shapes or the planner therefore cannot move
a seam away from its case without a failure here.

Every shape runs on three inputs (a synthetic light field with one frame of
full-range noise, full-range noise, and the carry stack), every family and
predictor.  Every launch writes into the middle of one allocation with 4 KiB
of 0xA5 before and after the frames: both guards, and d_in and d_prev, are
compared after every launch.  tests/test_predict_cases_cpu.py shows without a
GPU that the lists reach the seams they name and that these inputs tell a
broken seam from a sound one."""
import numpy as np
import pytest

import predict_cases as pc

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5


@pytest.fixture(autouse=True)
def automatic_pieces_afterwards(lfmlib):
    yield
    lfmlib.predict_set_pieces(0)


def dev_bytes(torch, a, off):
    """`a`'s bytes in a device allocation of its own, `off` bytes in."""
    buf = torch.zeros(off + a.nbytes, dtype=torch.uint8, device="cuda")
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    return buf


def brief(plan):
    return ["%(kernel)s f%(first)d+%(nframes)d %(strip)dx%(nstrip)d rows%(rows_per_piece)dx%(npiece)d xcd%(xcd_map)d"
            % L for L in plan]


def pin_plan(lfmlib, c, fam, k, pieces, aligned):
    """Assert what the plan query reports for the case; returns (plan, automatic plan in brief)."""
    lfmlib.predict_set_pieces(0)
    auto = lfmlib.predict_plan(c.W, c.H, c.n, c.T, fam, k, c.video, c.z0, c.cands, aligned)
    what = (pc.case_id(c), fam, k, pieces, "automatic plan", brief(auto))
    model = pc.model_plan(c.W, c.H, c.n, c.T, fam, k, c.video, c.z0, c.cands, aligned, pieces or 1)
    assert pc.device_free(auto) == pc.device_free(model), what
    if not pieces:
        return auto, what
    lfmlib.predict_set_pieces(pieces)
    plan = lfmlib.predict_plan(c.W, c.H, c.n, c.T, fam, k, c.video, c.z0, c.cands, aligned)
    assert plan == model, what
    return plan, what


def run_case(lfmlib, O, torch, c, fams=pc.FAMS, off_in=0, off_out=0, off_prev=0):
    """Every input x family x predictor x piece count of one case against the
    oracle, between guards.  The off_* put d_in, d_out and d_prev that many
    bytes past a 16-byte boundary.  Returns the plans that ran."""
    n_out = 7 if c.cands else c.n
    fb = c.H * c.W * 2
    uses_prev = bool(c.video and c.z0 & 1)
    aligned = off_in % 16 == 0 and off_out % 16 == 0 and (not uses_prev or off_prev % 16 == 0)
    plans = {}
    out_buf = torch.empty(GUARD + off_out + n_out * fb + GUARD, dtype=torch.uint8, device="cuda")
    exp_buf = torch.empty_like(out_buf)
    lo = GUARD + off_out
    for kind in pc.INPUTS:
        full = pc.case_input(O, c, kind)
        in_buf = dev_bytes(torch, full[c.z0:], off_in)
        in_ref = in_buf.clone()
        prev_buf = dev_bytes(torch, full[c.z0 - 1], off_prev) if uses_prev else None
        prev_ref = prev_buf.clone() if uses_prev else None
        for fam in fams:
            for k in ((0,) if c.cands else range(1, 8)):
                exp = pc.expected(O, c, full, fam, k)
                exp_buf.fill_(FILL)
                exp_buf[lo:lo + n_out * fb] = torch.from_numpy(exp.view(np.uint8).reshape(-1)).cuda()
                for pieces in c.pieces:
                    if (fam, k, pieces) not in plans:
                        plans[fam, k, pieces] = pin_plan(lfmlib, c, fam, k, pieces, aligned)
                    what = plans[fam, k, pieces][1] + (kind,)
                    lfmlib.predict_set_pieces(pieces)
                    out_buf.fill_(FILL)
                    if c.cands:
                        lfmlib.predict_candidates_device(in_buf[off_in:], out_buf[lo:], c.W, c.H, c.T, fam)
                    else:
                        lfmlib.predict_device(in_buf[off_in:], out_buf[lo:], c.W, c.H, c.n, c.T, fam, k, c.video,
                                              c.z0, prev_buf[off_prev:] if uses_prev else None)
                    if not torch.equal(out_buf, exp_buf):
                        explain(out_buf, exp, lo, what)
                    assert torch.equal(in_buf, in_ref), ("d_in written",) + what
                    assert not uses_prev or torch.equal(prev_buf, prev_ref), ("d_prev written",) + what
    return [p for p, _ in plans.values()]


def explain(out_buf, exp, lo, what):
    host = out_buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all(), ("guard before the frames written",) + what
    assert (host[GUARD:lo] == FILL).all(), ("bytes before the frames written",) + what
    assert (host[lo + exp.nbytes:] == FILL).all(), ("guard after the frames written",) + what
    got = host[lo:lo + exp.nbytes].view(np.uint16).reshape(exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, ("%d symbols differ, first at (frame, y, x)" % len(bad), bad[0].tolist()) + what
    raise AssertionError(("device buffer differs",) + what)


def kernels_of(plans):
    return {L["kernel"] for p in plans for L in p}


# ------------------------------------------------------------- B1: list V --
@pytest.mark.parametrize("fam", pc.FAMS)
@pytest.mark.parametrize("group", pc.V_GROUPS)
@pytest.mark.parametrize("T", pc.V_T)
def test_vec(lfmlib, oracle, gpu, T, group, fam):
    """predict_vec: widths around the 512- and 1024-pixel strips, heights from
    one row to a ring that wraps nine times, one to several pieces, stacks."""
    xcd = set()
    for c in pc.list_v(T, group):
        plans = run_case(lfmlib, oracle, gpu, c, fams=(fam,))
        assert kernels_of(plans) == {"vec"}, pc.case_id(c)
        xcd |= {L["xcd_map"] for p in plans for L in p}
    if group == "stacks":
        assert xcd == {0, 1}, "8 frames x 1 piece turn xcd_map on, 3 frames leave it off"


# ------------------------------------------------------------- B2: list P --
@pytest.mark.parametrize("fam", pc.FAMS)
@pytest.mark.parametrize("W", pc.P_WIDTHS)
@pytest.mark.parametrize("T", pc.V_T)
def test_vec_pair_and_singles(lfmlib, oracle, gpu, T, W, fam):
    """Video volumes: frame pairs, a temporal first frame from d_prev (the
    lone one is the only way into predict_vec's own P ring) and a spatial
    last frame."""
    roles, xcd = set(), set()
    for H in pc.p_heights(T):
        for c in pc.list_p(T, W, H):
            plans = run_case(lfmlib, oracle, gpu, c, fams=(fam,))
            for p in plans:
                roles |= {pc.launch_role(c, L) for L in p}
                xcd |= {L["xcd_map"] for L in p if L["kernel"] == "vec_pair"}
            assert kernels_of(plans) <= {"vec", "vec_pair"}, pc.case_id(c)
    assert {"temporal-first", "pairs", "spatial-last"} <= roles
    # (16, 0) x 1 piece and (8, 0) x 2 pieces turn xcd_map on where a row has more than one strip
    assert xcd == ({0, 1} if W > 512 else {0})


# ------------------------------------------------------------- B3: list R --
@pytest.mark.parametrize("W", pc.R_WIDTHS)
@pytest.mark.parametrize("T", pc.R_T)
def test_ring(lfmlib, oracle, gpu, T, W):
    """predict_ring: every other T <= 31, halo 16 and 32, with and without video."""
    for c in pc.list_r(T, W):
        assert kernels_of(run_case(lfmlib, oracle, gpu, c)) == {"ring"}, pc.case_id(c)


def test_ring_and_cands_with_xcd_map(lfmlib, oracle, gpu):
    """Lists R and C leave xcd_map off with every forced piece count; here it is on."""
    for c in pc.list_r_xcd() + pc.list_c_xcd():
        plans = run_case(lfmlib, oracle, gpu, c)
        assert kernels_of(plans) == {"cands" if c.cands else "ring"}, pc.case_id(c)
        assert {L["xcd_map"] for p in plans for L in p} == {1}, pc.case_id(c)


# ------------------------------------------------------------- B4: list C --
@pytest.mark.parametrize("T", pc.C_T)
def test_cands(lfmlib, oracle, gpu, T):
    """predict_cands: all seven outputs against predict_frame."""
    for c in pc.list_c(T):
        plans = run_case(lfmlib, oracle, gpu, c)
        assert kernels_of(plans) == {"cands"} and {L["grid_y"] for p in plans for L in p} == {7}, pc.case_id(c)


def test_cands_generic_loop(lfmlib, oracle, gpu):
    for c in pc.list_c_generic():
        plans = run_case(lfmlib, oracle, gpu, c)
        assert kernels_of(plans) == {"generic"} and {len(p) for p in plans} == {7}, pc.case_id(c)


# ------------------------------------------------------------- B5: list G --
@pytest.mark.parametrize("T", pc.G_T)
def test_generic(lfmlib, oracle, gpu, T):
    """predict_generic: T beyond W, H or both, widths no ring kernel takes."""
    for c in pc.list_g(T):
        assert kernels_of(run_case(lfmlib, oracle, gpu, c)) == {"generic"}, pc.case_id(c)


# ------------------------------------------------------------- B6: list A --
@pytest.mark.parametrize("which", pc.A_WHICH)
@pytest.mark.parametrize("i", range(len(pc.A_CASES)), ids=[pc.case_id(c) for c, _ in pc.A_CASES])
def test_misaligned_pointers_take_the_generic_kernel(lfmlib, oracle, gpu, i, which):
    """d_in, d_out and d_prev 2, 4 and 8 bytes past a 16-byte boundary, one at
    a time and all together: the call takes predict_generic (the ring, vec and
    pair kernels move 16 bytes per lane), the symbols are exact and the guards
    clean.  Aligned, the same shapes take their fast kernels."""
    c, kernels = pc.A_CASES[i]
    for fam in pc.FAMS:
        plan = lfmlib.predict_plan(c.W, c.H, c.n, c.T, fam, 1, c.video, c.z0, c.cands, True)
        assert tuple(L["kernel"] for L in plan) == kernels
    if which == "prev" and not (c.video and c.z0 & 1):
        return  # this call reads no d_prev
    for off in pc.A_OFFSETS:
        offs = dict(off_in=off if which in ("in", "all") else 0, off_out=off if which in ("out", "all") else 0,
                    off_prev=off if which in ("prev", "all") else 0)
        assert kernels_of(run_case(lfmlib, oracle, gpu, c, **offs)) == {"generic"}, (pc.case_id(c), which, off)
