"""The inverse predictor's three kernels (lfm_unpredict.hip: the chain
unpredict_band5, the frame wave unpredict_band3, the one-wave kernel
unpredict_band) at their seams, bit for bit against the oracle.

Every case first pins the path its shape takes (lfm_hip_unpredict_path), so a
change to choose_path cannot silently move a seam to another kernel.  Two
references:

1. forward then inverse: the oracle's forward symbols of a stack decode to
   that stack;
2. arbitrary symbols: uniform uint16 symbols with one all-0xFFFF frame (the
   residual -32768) and one all-0xFFFE frame decode to the oracle's
   unpredict_volume of them.  Zig-zag is a bijection on uint16 and every
   inverse formula is defined for any residual, so this is a valid reference
   (tests/test_oracle.py::test_unpredict_is_a_bijection_on_arbitrary_symbols
   pins it without a GPU); it puts the uint16 wrap and the (pred + P) >> 1 of
   temporal frames at every position and in every case.

Every call decodes into the middle of one larger allocation with 4 KiB of
0xA5 before and after the frames: a kernel writes inside its frames only."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMS = ("tiles", "angle", "space")
CHAIN, FRAME_WAVE, ONE_WAVE = 0, 1, 2
GUARD, FILL = 4096, 0xA5
Z = 3
EINVAL, ENOTINV = 1, 3  # lfm_hip.h

# (path, W, H, T): kSync = 32 columns per chain round, kRing = 64, kHand = 128,
# kSymAhead = 8, bands of 64 rows, the frame wave's LDS gate at 163840 B
SHAPES = [
    (CHAIN, 8, 65, 2),         # narrowest frame, one-row last band, smallest T
    (CHAIN, 16, 129, 3),
    (CHAIN, 24, 70, 5),
    (CHAIN, 32, 128, 13),      # exactly two bands
    (CHAIN, 40, 66, 7),
    (CHAIN, 48, 200, 15),      # W % 32 = 16
    (CHAIN, 56, 130, 30),      # W % 32 = 24, T = 30
    (CHAIN, 64, 192, 13),      # W = kRing, three exact bands
    (CHAIN, 72, 65, 2),
    (CHAIN, 120, 70, 11),      # W % 32 = 24
    (CHAIN, 128, 129, 13),     # W = kHand
    (CHAIN, 144, 100, 9),      # W % 32 = 16
    (CHAIN, 8, 1000, 2),       # 16 bands, each completed before the next may start
    (CHAIN, 1024, 70, 15),     # the hand-over ring wraps 8 times
    (CHAIN, 2504, 70, 30),     # widest T = 30 chain frame
    (CHAIN, 4864, 65, 15),     # frame_wave_lds exactly 163840 B, the gate's last chain width
    (FRAME_WAVE, 8, 64, 13),   # W % 8 == 0 but one band
    (FRAME_WAVE, 64, 64, 2),
    (FRAME_WAVE, 2048, 64, 15),
    (FRAME_WAVE, 7, 65, 2),
    (FRAME_WAVE, 9, 128, 3),
    (FRAME_WAVE, 63, 129, 13),
    (FRAME_WAVE, 65, 66, 30),
    (FRAME_WAVE, 127, 70, 30),
    (FRAME_WAVE, 1, 130, 2),   # narrower than the delay line or one lenslet
    (FRAME_WAVE, 2, 70, 13),
    (FRAME_WAVE, 3, 65, 5),
    (FRAME_WAVE, 5, 200, 13),
    (FRAME_WAVE, 2510, 65, 30),  # 163812 B of LDS
    (FRAME_WAVE, 4862, 70, 15),  # 163776 B of LDS
    (FRAME_WAVE, 4864, 64, 15),  # exactly 160 KiB of LDS, one band
    (ONE_WAVE, 64, 130, 1),    # T = 1 with W % 8 == 0, H > 64
    (ONE_WAVE, 1, 1, 1),
    (ONE_WAVE, 200, 64, 1),
    (ONE_WAVE, 248, 130, 31),  # T = 31, several bands
    (ONE_WAVE, 31, 31, 31),
    (ONE_WAVE, 62, 65, 31),
    (ONE_WAVE, 4872, 65, 15),  # first width past the LDS gate
    (ONE_WAVE, 2512, 66, 30),  # first width past the LDS gate
]
PATH_NAMES = ("chain", "framewave", "onewave")
SHAPE_IDS = ["%s-%dx%d-T%d" % (PATH_NAMES[p], W, H, T) for p, W, H, T in SHAPES]
# one shape of each path for the z0 / d_prev cases
Z0_SHAPES = [(CHAIN, 72, 65, 2), (FRAME_WAVE, 63, 129, 13), (ONE_WAVE, 64, 130, 1)]
Z0_IDS = ["%s-%dx%d-T%d" % (PATH_NAMES[p], W, H, T) for p, W, H, T in Z0_SHAPES]


def combos():
    """(family, k, video): every family and predictor, video for tiles."""
    for fam in FAMS:
        for k in range(1, 8):
            for video in ((0, 1) if fam == "tiles" else (0,)):
                yield fam, k, video


def frozen(a):
    a.setflags(write=False)
    return a


def arbitrary_symbols(rng, nframes, H, W, k):
    """Uniform uint16 symbols; one whole frame 0xFFFF, one 0xFFFE.  Which
    frames rotates with k, so over the predictors every frame position
    (spatial and temporal) carries each of the three kinds."""
    sym = rng.integers(0, 65536, size=(nframes, H, W), dtype=np.uint16)
    sym[k % nframes] = 0xFFFF
    sym[(k + 1) % nframes] = 0xFFFE
    return sym


def decode_guarded(lfmlib, torch, sym, W, H, T, fam, k, video, z0=0, prev=None, adjacent=False, what=()):
    """lfm_hip_unpredict of `sym` (n, H, W) into the middle of one allocation:
    4 KiB of 0xA5, [the previous frame when `adjacent`], the n frames, 4 KiB
    of 0xA5.  Checks both guards and that the previous frame was not written;
    returns the decoded frames."""
    n = sym.shape[0]
    fb = H * W * 2
    lead = fb if (prev is not None and adjacent) else 0
    buf = torch.full((GUARD + lead + n * fb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_sym = torch.from_numpy(sym.view(np.int16).copy()).cuda()
    d_prev = None
    if prev is not None:
        pbytes = torch.from_numpy(prev.view(np.uint8).reshape(-1).copy())
        if adjacent:
            buf[GUARD:GUARD + fb] = pbytes.cuda()
            d_prev = buf.data_ptr() + GUARD
        else:
            d_prev = pbytes.cuda()
    torch.cuda.synchronize()
    lfmlib.unpredict_device(d_sym, buf.data_ptr() + GUARD + lead, W, H, n, T, fam, k, video=video, z0=z0,
                            d_prev=d_prev)
    torch.cuda.synchronize()
    return check_guarded(buf, n, H, W, lead, prev, None if adjacent else d_prev, what)


def check_guarded(buf, n, H, W, lead, prev, d_prev, what):
    host = buf.cpu().numpy()
    fb = H * W * 2
    assert (host[:GUARD] == FILL).all(), ("guard before the frames written",) + tuple(what)
    assert (host[GUARD + lead + n * fb:] == FILL).all(), ("guard after the frames written",) + tuple(what)
    if prev is not None:
        pv = host[GUARD:GUARD + lead] if lead else d_prev.cpu().numpy()
        assert np.array_equal(pv.view(np.uint16).reshape(H, W), prev), ("previous frame written",) + tuple(what)
    return host[GUARD + lead:GUARD + lead + n * fb].view(np.uint16).reshape(n, H, W)


def seed_of(W, H, T):
    return (W * 1000003 + H * 1009 + T) & 0x7FFFFFFF


@pytest.mark.parametrize("path,W,H,T", SHAPES, ids=SHAPE_IDS)
def test_inverts_forward(lfmlib, oracle, gpu, path, W, H, T):
    """Reference 1: the oracle's forward symbols of a stack (synthetic light
    field, frame 1 full-range noise) decode to the stack, every family,
    predictor and video setting."""
    torch = gpu
    assert lfmlib.unpredict_path(W, H, T) == path
    stack = oracle.synthetic_lf(W, H, Z=Z, T=T, seed=seed_of(W, H, T))[0, 0].copy()
    stack[1] = np.random.default_rng(seed_of(W, H, T)).integers(0, 65536, size=(H, W), dtype=np.uint16)
    frozen(stack)
    for fam, k, video in combos():
        sym = oracle.predict_volume(stack, T, fam, k, video)
        got = decode_guarded(lfmlib, torch, sym, W, H, T, fam, k, video, what=(fam, k, video))
        assert np.array_equal(got, stack), (fam, k, video)


@pytest.mark.parametrize("path,W,H,T", SHAPES, ids=SHAPE_IDS)
def test_arbitrary_symbols(lfmlib, oracle, gpu, path, W, H, T):
    """Reference 2: arbitrary symbols decode to the oracle's unpredict_volume,
    every family, predictor and video setting."""
    torch = gpu
    assert lfmlib.unpredict_path(W, H, T) == path
    rng = np.random.default_rng(seed_of(W, H, T) ^ 0x5A5A)
    for k in range(1, 8):
        sym = frozen(arbitrary_symbols(rng, Z, H, W, k))
        for fam in FAMS:
            for video in ((0, 1) if fam == "tiles" else (0,)):
                exp = oracle.unpredict_volume(sym, T, fam, k, video)
                got = decode_guarded(lfmlib, torch, sym, W, H, T, fam, k, video, what=(fam, k, video))
                assert np.array_equal(got, exp), (fam, k, video)


@functools.lru_cache(maxsize=None)
def z0_reference(O, W, H, T):
    """Per predictor, for a tiles video stack of Z + 1 frames: (symbols, decoded
    frames) of both references, computed once per shape and read-only."""
    rng = np.random.default_rng(seed_of(W, H, T) ^ 0x7A30)
    stack = O.synthetic_lf(W, H, Z=Z + 1, T=T, seed=seed_of(W, H, T) + 1)[0, 0].copy()
    stack[2] = rng.integers(0, 65536, size=(H, W), dtype=np.uint16)
    frozen(stack)
    ref = {}
    for k in range(1, 8):
        fwd = frozen(O.predict_volume(stack, T, "tiles", k, 1))
        arb = frozen(arbitrary_symbols(rng, Z + 1, H, W, k))
        ref[k] = ((fwd, stack), (arb, frozen(O.unpredict_volume(arb, T, "tiles", k, 1))))
    return ref


# (first global frame, frames, previous frame passed, previous frame in front of d_out in one allocation)
Z0_MODES = {
    "z0_1-prev": [(1, Z, True, False)],
    "z0_1-prev_adjacent": [(1, Z, True, True)],        # as the file reader passes it
    "lone-prev": [(1, 1, True, False), (3, 1, True, False)],
    "lone-prev_adjacent": [(1, 1, True, True), (3, 1, True, True)],
    "z0_2-noprev": [(2, Z - 1, False, False), (2, 1, False, False)],
}


@pytest.mark.parametrize("mode", list(Z0_MODES))
@pytest.mark.parametrize("path,W,H,T", Z0_SHAPES, ids=Z0_IDS)
def test_first_frame_offset_and_previous_frame(lfmlib, oracle, gpu, path, W, H, T, mode):
    """Calls that start inside a video stack, as the decode pipeline issues them
    at every chunk and volume boundary: frames z0 .. of a CPU-decoded stack
    with the decoded frame z0 - 1 in d_prev (odd z0: frame 0 of the call is
    temporal), a lone temporal frame, and an even z0 without d_prev."""
    torch = gpu
    assert lfmlib.unpredict_path(W, H, T) == path
    ref = z0_reference(oracle, W, H, T)
    for k in range(1, 8):
        for name, (sym, dec) in zip(("forward", "arbitrary"), ref[k]):
            for z0, n, with_prev, adjacent in Z0_MODES[mode]:
                what = (name, k, z0, n)
                prev = dec[z0 - 1] if with_prev else None
                got = decode_guarded(lfmlib, torch, sym[z0:z0 + n], W, H, T, "tiles", k, 1, z0=z0, prev=prev,
                                     adjacent=adjacent, what=what)
                assert np.array_equal(got, dec[z0:z0 + n]), what


def test_error_paths_launch_nothing(lfmlib, oracle, gpu):
    """Each refusal is a return code with the output untouched; the spatial
    frame 0 of an angle / space video stack still decodes."""
    torch = gpu
    W, H, T = 16, 16, 13
    stack = frozen(oracle.synthetic_lf(W, H, Z=2, T=T, seed=11)[0, 0].copy())
    out = torch.full((2, H, W), 0x2525, dtype=torch.int16, device="cuda")
    prev = torch.from_numpy(stack[0].view(np.int16).copy()).cuda()
    sym = torch.from_numpy(oracle.predict_volume(stack, T, "tiles", 4, 1).view(np.int16)).cuda()

    def refused(code, nframes, T_, fam, video, z0, d_prev):
        with pytest.raises(lfmlib.LfmError, match="code %d$" % code):
            lfmlib.unpredict_device(sym, out, W, H, nframes, T_, fam, 4, video=video, z0=z0, d_prev=d_prev)
        torch.cuda.synchronize()
        assert bool((out == 0x2525).all()), "a refused call wrote pixels"

    refused(EINVAL, 1, T, "tiles", 1, 1, None)       # a temporal first frame without its predecessor
    refused(EINVAL, 2, 0, "tiles", 0, 0, None)
    refused(EINVAL, 2, 32, "tiles", 0, 0, None)
    for fam in ("angle", "space"):
        refused(ENOTINV, 1, T, fam, 1, 1, prev)       # ((I - pred) + P) >> 1 drops a bit
        for k in range(1, 8):                         # frame 0 of the video stack is spatial
            s = oracle.predict_volume(stack[:1], T, fam, k, 1)
            got = decode_guarded(lfmlib, torch, s, W, H, T, fam, k, 1, z0=0, what=(fam, k))
            assert np.array_equal(got, stack[:1]), (fam, k)


def test_two_streams_keep_chain_calls_apart(lfmlib, oracle, gpu):
    """Eight chain calls queued through lfm_hip_unpredict_async alternately on
    two streams, one synchronisation: every status word is clean and every
    call's pixels are the oracle's.  Calls in flight together take separate
    control blocks (ticket and progress words)."""
    torch = gpu
    env = dict(os.environ)
    A, B = (48, 200, 15, 5), (128, 129, 13, 3)
    order = [A, B, B, A, A, B, B, A]   # each shape four times, twice on either stream
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    status = torch.full((len(order),), -1, dtype=torch.int32).pin_memory()
    rng = np.random.default_rng(0x2575)
    calls = []
    for i, (W, H, T, n) in enumerate(order):
        assert lfmlib.unpredict_path(W, H, T) == CHAIN
        fam, k, video = [("tiles", 5, 1), ("angle", 2, 0), ("space", 7, 0), ("tiles", 3, 0)][i % 4]
        if i >= 4:
            k = 8 - k
        sym = arbitrary_symbols(rng, n, H, W, i)
        buf = torch.full((GUARD + n * H * W * 2 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        d_sym = torch.from_numpy(sym.view(np.int16)).cuda()
        calls.append((W, H, T, n, fam, k, video, sym, d_sym, buf))
    torch.cuda.synchronize()
    for i, (W, H, T, n, fam, k, video, sym, d_sym, buf) in enumerate(calls):
        lfmlib.unpredict_device_async(d_sym, buf.data_ptr() + GUARD, W, H, n, T, fam, k, video=video,
                                      status=status[i:i + 1], stream=streams[i % 2])
    torch.cuda.synchronize()
    for i, (W, H, T, n, fam, k, video, sym, d_sym, buf) in enumerate(calls):
        assert int(status[i]) == 0, (i, int(status[i]))   # no hand-over gave up
        lfmlib.unpredict_check(status[i:i + 1])
        got = check_guarded(buf, n, H, W, 0, None, None, (i, fam, k, video))
        assert np.array_equal(got, oracle.unpredict_volume(sym, T, fam, k, video)), (i, fam, k, video)
    assert dict(os.environ) == env
