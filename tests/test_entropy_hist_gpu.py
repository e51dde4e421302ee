"""Predictor selection, exactly (csrc/lfm_entropy.hip).

The integer bigram histograms ent_next -> ent_link -> ent_rows count
(lfm_hip_entropy2d_hist: the same launches, the counters stored before any
float arithmetic) against the oracle's counting sort, bin for bin, on the cases
of tests/entropy_cases.py -- every seam across which a byte is linked to its
next occurrence: 64-lane windows, 4 KiB waves, 16 KiB segments, keys (sentinel,
end of L) and 900 000-byte chunks.  test_entropy_cases_cpu.py shows that these
cases see errors the float tolerance of tests/test_gpu.py cannot.  Then the
caller's workspace of lfm_hip_select between guards, and the selection rule
(exact ties to the highest index, candidate 0 times 0.96) on frames that tie."""
import ctypes
import json
import os

import numpy as np
import pytest

import entropy_cases as E
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CASES = E.all_cases()


def dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def assert_rule(k, ent):
    """std::map<float, int>: the lowest entropy wins, equal keys keep the last index."""
    assert k == max(i for i in range(8) if ent[i] == ent.min()), (k, ent)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bigram_histograms_equal_the_oracles(lfmlib, oracle, gpu, case):
    torch = gpu
    buf = case.build()
    cands = E.candidates(case, buf)
    d_buf = dev16(torch, buf)
    d_cands = [d_buf[k:k + case.npix] for k in range(case.ncand)]  # byte offsets 2k of one allocation
    got = lfmlib.entropy_hist_device(d_cands, case.npix)
    assert got.shape == (case.ncand, case.claims["nchunks"], 65536)
    for k, cand in enumerate(cands):
        want = oracle.bigram_hist(cand)
        for q in range(want.shape[0]):
            if not np.array_equal(got[k, q], want[q]):
                b = int(np.flatnonzero(got[k, q] != want[q])[0])
                pytest.fail("%s candidate %d chunk %d: %d bins differ, the first is 0x%04X: kernel %d, oracle %d"
                            % (case.name, k, q, int((got[k, q] != want[q]).sum()), b, got[k, q, b], want[q, b]))
        # the float stage on top of the exact counts (the tolerance of tests/test_gpu.py: the two sides
        # differ in logf only)
        e = lfmlib.entropy_device(d_cands[k], case.npix)
        assert abs(e - oracle.entropy2d(cand)) <= 1e-5 * max(1.0, abs(e)), (case.name, k)


def test_hist_entry_rejects_bad_operands(lfmlib, gpu):
    torch = gpu
    L = lfmlib.lib()
    d = torch.zeros(8, dtype=torch.int16, device="cuda")
    h = torch.zeros(65536, dtype=torch.int32, device="cuda")
    one = (ctypes.c_void_p * 9)(*[d.data_ptr()] * 9)
    LFM_HIP_EINVAL = 1  # lfm_hip.h
    assert L.lfm_hip_entropy2d_hist(one, 0, 8, h.data_ptr(), None) == LFM_HIP_EINVAL
    assert L.lfm_hip_entropy2d_hist(one, 9, 8, h.data_ptr(), None) == LFM_HIP_EINVAL
    assert L.lfm_hip_entropy2d_hist(one, 1, 0, h.data_ptr(), None) == LFM_HIP_EINVAL
    assert L.lfm_hip_entropy2d_hist(one, 1, 8, None, None) == LFM_HIP_EINVAL
    assert L.lfm_hip_entropy2d_hist((ctypes.c_void_p * 2)(d.data_ptr(), None), 2, 8, h.data_ptr(), None) == LFM_HIP_EINVAL
    torch.cuda.synchronize()
    assert not h.any()


# -------------------------------------------------------------- workspace --
GUARD, GUARD_FILL = 4096, 0x3C


class Guarded:
    """nbytes of device memory at a 256-byte aligned address between two 4 KiB guards."""

    def __init__(self, torch, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + 256 + nbytes + GUARD,), GUARD_FILL, dtype=torch.uint8, device="cuda")
        self.lo = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = self.buf.data_ptr() + self.lo
        assert self.ptr % 256 == 0

    def fill(self, v):
        self.buf[self.lo:self.lo + self.nbytes] = v

    def check(self):
        assert bool((self.buf[:self.lo] == GUARD_FILL).all()), "guard before the workspace written"
        assert bool((self.buf[self.lo + self.nbytes:] == GUARD_FILL).all()), "guard after the workspace written"


def select_raw(lfmlib, torch, d_frame, W, H, T, fam, ws_ptr):
    ent, k = (ctypes.c_float * 8)(), ctypes.c_int(-1)
    rc = lfmlib.lib().lfm_hip_select(d_frame.data_ptr(), W, H, T, lfmlib.FAMILIES[fam], ent, ctypes.byref(k), ws_ptr, None)
    torch.cuda.synchronize()
    assert rc == 0
    return k.value, np.array(list(ent), dtype=np.float32)


def frame_of(oracle, W, H, T):
    return oracle.synthetic_lf(W, H, Z=1, T=T, seed=0x4C464D31 + W)[0, 0, 0]


@pytest.mark.parametrize("W,H", [(97, 53), (300, 1600)], ids=["odd-npix", "two-chunks"])
def test_select_workspace_is_exactly_its_size(lfmlib, oracle, gpu, W, H):
    """lfm_hip_select through ctypes with a workspace of exactly
    lfm_hip_select_workspace_bytes(W, H): the guards stay untouched, and
    nothing the workspace held before the call reaches the result."""
    torch = gpu
    T, fam = 13, "tiles"
    fr = frame_of(oracle, W, H, T)
    d = dev16(torch, fr)
    ws = Guarded(torch, lfmlib.lib().lfm_hip_select_workspace_bytes(W, H))
    k0, e0 = select_raw(lfmlib, torch, d, W, H, T, fam, None)
    for fill in (0x00, 0xFF, 0xA5):
        ws.fill(fill)
        k, e = select_raw(lfmlib, torch, d, W, H, T, fam, ws.ptr)
        ws.check()
        assert k == k0 and e.tobytes() == e0.tobytes(), hex(fill)
    ko, eo = oracle.select(fr, T, fam)
    assert k0 == ko
    np.testing.assert_allclose(e0, eo, rtol=1e-5, atol=1e-6)
    assert_rule(k0, e0)


def test_select_workspace_reused_for_a_smaller_frame(lfmlib, oracle, gpu):
    """The larger frame's workspace, then a smaller frame in the same memory
    right after it: tables, partners and row sums of the first call are stale
    bytes for the second."""
    torch = gpu
    T, fam = 13, "tiles"
    big, small = (300, 1600), (97, 53)
    ws = Guarded(torch, lfmlib.lib().lfm_hip_select_workspace_bytes(*big))
    assert lfmlib.lib().lfm_hip_select_workspace_bytes(*small) < ws.nbytes
    frames = {s: dev16(torch, frame_of(oracle, s[0], s[1], T)) for s in (big, small)}
    alone = {s: select_raw(lfmlib, torch, frames[s], s[0], s[1], T, fam, None) for s in (big, small)}
    ws.fill(0xA5)
    for s in (big, small, big, small):
        k, e = select_raw(lfmlib, torch, frames[s], s[0], s[1], T, fam, ws.ptr)
        ws.check()
        assert k == alone[s][0] and e.tobytes() == alone[s][1].tobytes(), s
        assert_rule(k, e)


# ------------------------------------------------ ties and the 0.96 factor --
TIES = E.tie_frames()


@pytest.mark.parametrize("name,frame,fam,tied,chosen", TIES, ids=[t[0] for t in TIES])
def test_exact_ties_go_to_the_highest_index(lfmlib, oracle, gpu, name, frame, fam, tied, chosen):
    torch = gpu
    d = dev16(torch, frame)
    k, ent = lfmlib.select_device(d, E.TIE_W, E.TIE_H, E.TIE_T, fam)
    ko, ento = oracle.select(frame, E.TIE_T, fam)
    assert k == ko == chosen == max(tied)
    assert len({ent[i].tobytes() for i in tied}) == 1, "equal candidate buffers give equal floats: %s" % ent
    assert [i for i in range(8) if ent[i] == ent.min()] == tied
    assert_rule(k, ent)
    np.testing.assert_allclose(ent, ento, rtol=1e-5, atol=1e-6)
    raw = np.float32(lfmlib.entropy_device(d.reshape(-1)))
    assert ent[0].tobytes() == np.float32(np.float64(raw) * 0.96).tobytes()


def test_golden_selections_follow_the_map_rule(lfmlib, oracle, gpu):
    """The golden frames of test_entropy_and_selection_vs_golden, close calls
    included: chosen is the highest index among the lowest returned floats."""
    torch = gpu
    for r in json.load(open(os.path.join(GOLDEN, "entropy_vectors.json"))):
        if r["kind"] == "zeros":
            fr = np.zeros((r["H"], r["W"]), np.uint16)
        elif r["kind"] == "lf":
            fr = oracle.synthetic_lf(r["W"], r["H"], Z=2, T=r["T"], seed=r["seed"])[0, 0, 1]
        else:
            fr = np.random.default_rng(r["seed"]).integers(0, 65536, size=(2, r["H"], r["W"]), dtype=np.uint16)[1]
        d = dev16(torch, fr)
        k, ent = lfmlib.select_device(d, r["W"], r["H"], r["T"], r["family"])
        assert_rule(k, ent)
        raw = np.float32(lfmlib.entropy_device(d.reshape(-1)))
        assert ent[0].tobytes() == np.float32(np.float64(raw) * 0.96).tobytes(), r
