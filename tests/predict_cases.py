"""Case lists for the forward predictor (lfm_predict.hip: predict_generic,
predict_ring, predict_cands, predict_vec, predict_vec_pair), a model of its
launch planner, the three inputs every shape runs on, and the wrong answers a
broken seam would give.  Shared by tests/test_predict_cases_cpu.py (the lists
are what they claim, without a GPU) and tests/test_predict_seams_gpu.py.

A case is one call shape: (list, T, W, H, frames, z0, video, candidates) and
the piece counts it runs with.  Piece count 0 is the planner's automatic count
(it depends on the device), CAP is a count so large that the planner's own cap
of H / (2 (T + 1)) pieces decides."""
import collections
import functools

import numpy as np

FAMS = ("tiles", "angle", "space")
INPUTS = ("lf", "noise", "carry")
CAP = 1 << 20

Case = collections.namedtuple("Case", "lst T W H n z0 video cands pieces")


def case_id(c):
    return "%s-T%d-%dx%dx%d-z%d-v%d" % (c.lst, c.T, c.W, c.H, c.n, c.z0, c.video)


# ------------------------------------------------------------- plan model --
# The planner's arithmetic (make_plan_shape and the dispatch in front of it),
# restated from the kernel shapes: strip pixels, rows per step, prefetch depth,
# threads per workgroup.
def _vec_shape(fam):      # VecShape: tiles 2 waves per row of 8, angle / space 1 of 4
    return dict(sw=1024, rs=4, pd=3, threads=576) if fam == "tiles" else dict(sw=512, rs=4, pd=3, threads=320)


def _pair_shape(fam):     # PairShape: 8 compute waves, 4 per frame, one 512-pixel strip
    return dict(sw=512, rs=4, pd=3, threads=576)


def _ring_shape(fam):     # RingShape: tiles 2 rows per wave and 2 steps ahead, else 1 and 3
    return dict(sw=512, rs=8, pd=2, threads=320) if fam == "tiles" else dict(sw=512, rs=4, pd=3, threads=320)


def _launch(kernel, first=0, nframes=0, pairs=0, strip=0, nstrip=0, rows_per_step=0, rows_per_piece=0, npiece=0, R=0,
            RP=0, halo=0, xcd_map=0, grid_x=0, grid_y=0, threads=0, lds_bytes=0):
    return dict(kernel=kernel, first=first, nframes=nframes, pairs=pairs, strip=strip, nstrip=nstrip,
                rows_per_step=rows_per_step, rows_per_piece=rows_per_piece, npiece=npiece, R=R, RP=RP, halo=halo,
                xcd_map=xcd_map, grid_x=grid_x, grid_y=grid_y, threads=threads, lds_bytes=lds_bytes)


def _ring_launch(kernel, W, H, T, nz, z0, video, shape, halo, pieces, first=0, nframes=None, pairs=0, rings=1,
                 grid_y=1):
    """make_plan_shape with a forced piece count."""
    sw, rs, pd = shape["sw"], shape["rs"], shape["pd"]
    any_temporal = bool(video) and (nz > 1 or (z0 & 1))
    R = rs * (pd + 1) + T + 1
    RP = rs * (pd + 1) if any_temporal else 0
    nstrip = -(-W // sw)
    npiece = min(max(1, pieces), max(1, H // (2 * (T + 1))))
    rows = -(-H // npiece)
    rows = -(-rows // rs) * rs
    npiece = -(-H // rows)
    groups = nz * npiece
    return _launch(kernel, first=first, nframes=nz if nframes is None else nframes, pairs=pairs, strip=sw,
                   nstrip=nstrip, rows_per_step=rs, rows_per_piece=rows, npiece=npiece, R=R, RP=RP, halo=halo,
                   xcd_map=int(groups % 8 == 0 and nstrip > 1), grid_x=groups * nstrip, grid_y=grid_y,
                   threads=shape["threads"], lds_bytes=(rings * R * (halo + sw) + RP * sw) * 2)


def _generic_launch(W, H, nz):
    return _launch("generic", nframes=nz, grid_x=min(-(-W * H * nz // 256), 4096), grid_y=1, threads=256)


def model_plan(W, H, n, T, fam, k, video=0, z0=0, cands=False, aligned=True, pieces=1):
    """What lfm.predict_plan reports with the piece count forced to `pieces`."""
    assert pieces > 0
    video &= 1
    if cands:
        n, video, z0 = 1, 0, 0
    elif k == 0:
        return [_launch("copy", nframes=n)]
    wide = aligned and W % 8 == 0 and W >= 32
    if cands:
        if not (wide and T <= 31):
            return [_generic_launch(W, H, 1) for _ in range(7)]
        return [_ring_launch("cands", W, H, T, 1, 0, 0, _ring_shape(fam), 16 if T <= 15 else 32, pieces, grid_y=7)]
    if wide and T in (13, 15):
        vs = _vec_shape(fam)
        if not (video and n >= 2):
            return [_ring_launch("vec", W, H, T, n, z0, video, vs, 16, pieces)]
        first = z0 & 1
        npairs = (n - first) // 2
        out = []
        if first:
            out.append(_ring_launch("vec", W, H, T, 1, z0, video, vs, 16, pieces))
        if npairs:
            out.append(_ring_launch("vec_pair", W, H, T, npairs, z0, 0, _pair_shape(fam), 16, pieces, first=first,
                                    nframes=2 * npairs, pairs=npairs, rings=2))
        if first + 2 * npairs < n:
            out.append(_ring_launch("vec", W, H, T, 1, z0 + n - 1, video, vs, 16, pieces, first=n - 1))
        return out
    if wide and T <= 31:
        return [_ring_launch("ring", W, H, T, n, z0, video, _ring_shape(fam), 16 if T <= 15 else 32, pieces)]
    return [_generic_launch(W, H, n)]


# fields of a launch that do not depend on the device (asserted with the automatic piece count too)
DEVICE_FREE = ("kernel", "first", "nframes", "pairs", "strip", "nstrip", "rows_per_step", "R", "RP", "halo", "grid_y",
               "threads", "lds_bytes")


def device_free(plans):
    return [{f: p[f] for f in DEVICE_FREE} for p in plans]


def pieces_of(launch, H):
    """(ys, ye) of every row piece of a launch."""
    r = launch["rows_per_piece"]
    return [(i * r, min((i + 1) * r, H)) for i in range(launch["npiece"])]


def launch_role(c, launch):
    """A launch's part in a video volume: 'temporal-first', 'pairs', 'spatial-last', or None."""
    if launch["kernel"] == "vec_pair":
        return "pairs"
    if launch["kernel"] == "vec" and c.video and launch["nframes"] == 1:
        if (c.z0 + launch["first"]) & 1:
            return "temporal-first" if launch["first"] == 0 else None
        return "spatial-last" if c.n >= 2 and launch["first"] == c.n - 1 else None
    return None


# ------------------------------------------------------------------ lists --
def _dedupe(seq):
    seen, out = set(), []
    for v in seq:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


V_WIDTHS = (32, 40, 504, 512, 520, 1016, 1024, 1032, 1536, 1544, 2048, 2056)
V_PIECES = (0, 1, 2, CAP)


def v_heights(T):
    return _dedupe([1, 2, 3, 4, 5, 12, 13, 16, 17, T, T + 1, T + 2, 2 * T + 1, 2 * (T + 1), 4 * (T + 1) - 1,
                    4 * (T + 1), 4 * (T + 1) + 1, 131, 300])


def list_v(T, group):
    """predict_vec.  group: 'widths', 'heights520', 'heights1032', 'stacks'."""
    if group == "widths":
        return [Case("V", T, W, 2 * T + 5, 1, 0, 0, False, V_PIECES) for W in V_WIDTHS]
    if group == "stacks":
        return [Case("V", T, 1032, 4 * (T + 1) + 3, n, 0, 0, False, V_PIECES) for n in (1, 3, 8)]
    W = {"heights520": 520, "heights1032": 1032}[group]
    return [Case("V", T, W, H, 1, 0, 0, False, V_PIECES) for H in v_heights(T)]


V_GROUPS = ("widths", "heights520", "heights1032", "stacks")
V_T = (13, 15)

P_FRAMES = ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 1), (5, 0), (8, 0), (16, 0))
P_WIDTHS = (504, 520, 1032)
P_PIECES = (0, 1, 2)


def p_heights(T):
    # 5: two steps, fewer than the pair kernel's prefetch depth (T - 1 rows are exactly PD steps)
    return (5, T - 1, 2 * T + 3, 4 * (T + 1) + 3)


def list_p(T, W, H):
    """predict_vec_pair and its single-frame companions: the video bit is set."""
    return [Case("P", T, W, H, n, z0, 1, False, P_PIECES) for n, z0 in P_FRAMES]


R_T = (1, 2, 3, 7, 12, 14, 16, 17, 30, 31)
R_WIDTHS = (32, 40, 504, 512, 520, 1032)
R_MODES = ((1, 0, 0), (3, 0, 1), (3, 1, 1))   # (frames, z0, video)
R_PIECES = (0, 1, 2)


def r_heights(T):
    return _dedupe([1, 7, 8, 9, T, T + 2, 4 * (T + 1) + 1, 131])


def list_r(T, W):
    """predict_ring."""
    return [Case("R", T, W, H, n, z0, video, False, R_PIECES) for H in r_heights(T) for n, z0, video in R_MODES]


# Lists R and C never make frames x pieces a multiple of 8 with a forced count; these do: eight
# pieces of 16, 32 or 64 rows, (T, W, H)
XCD_SHAPES = ((7, 1032, 128), (15, 1032, 256), (31, 1032, 512))
XCD_PIECES = (8,)


def list_r_xcd():
    """predict_ring with xcd_map on."""
    return [Case("R", T, W, H, n, z0, video, False, XCD_PIECES) for T, W, H in XCD_SHAPES if T != 15
            for n, z0, video in ((1, 0, 0), (3, 1, 1))]


def list_c_xcd():
    """predict_cands with xcd_map on."""
    return [Case("C", T, W, H, 1, 0, 0, True, XCD_PIECES) for T, W, H in XCD_SHAPES]


C_T = (2, 13, 15, 16, 31)
C_WIDTHS = (32, 520, 1032, 2048)
C_PIECES = (0, 1, 2)
C_GENERIC = ((45, 31, 13), (64, 40, 33))   # (W, H, T): the entry's per-predictor generic loop


def list_c(T):
    """predict_cands."""
    return [Case("C", T, W, H, 1, 0, 0, True, C_PIECES) for W in C_WIDTHS for H in _dedupe([T - 1, 2 * T + 3, 131])]


def list_c_generic():
    return [Case("C", T, W, H, 1, 0, 0, True, (0,)) for W, H, T in C_GENERIC]


G_T = (13, 32, 33, 100)
G_MODES = ((1, 0, 0), (2, 0, 1), (2, 1, 1))


def list_g(T):
    """predict_generic: W % 8 != 0, W < 32 or T > 31."""
    shapes = [(W, H) for W in (1, 7, 24, 31, 45, 516) for H in (1, 31, 70)]
    if T == 32:
        shapes += [(512, H) for H in (1, 31, 70)]
    return [Case("G", T, W, H, n, z0, video, False, (0,)) for W, H in shapes for n, z0, video in G_MODES]


# alignment: (case, fast kernels of its aligned plan)
A_CASES = (
    (Case("A", 13, 520, 31, 1, 0, 0, False, (0,)), ("vec",)),
    (Case("A", 15, 520, 33, 3, 1, 1, False, (0,)), ("vec", "vec_pair")),
    (Case("A", 7, 520, 33, 3, 1, 1, False, (0,)), ("ring",)),
    (Case("A", 13, 520, 29, 1, 0, 0, True, (0,)), ("cands",)),
)
A_OFFSETS = (2, 4, 8)
A_WHICH = ("in", "out", "prev", "all")


def all_cases():
    out = []
    for T in V_T:
        for g in V_GROUPS:
            out += list_v(T, g)
        for W in P_WIDTHS:
            for H in p_heights(T):
                out += list_p(T, W, H)
    for T in R_T:
        for W in R_WIDTHS:
            out += list_r(T, W)
    out += list_r_xcd()
    for T in C_T:
        out += list_c(T)
    out += list_c_generic() + list_c_xcd()
    for T in G_T:
        out += list_g(T)
    out += [c for c, _ in A_CASES]
    return out


# ----------------------------------------------------------------- inputs --
def frozen(a):
    a.setflags(write=False)
    return a


def seed_of(c):
    return (c.W * 1000003 + c.H * 1009 + c.T * 31 + c.n * 7 + c.z0) & 0x7FFFFFFF


def carry_stack(n, H, W):
    """Frames cycle (A, all 0xFFFF, all 0) and every other A is inverted.  A's
    rows come in groups of three, alternately 'rows 0x8000 / 0x7FFF' and
    'columns 0x0000 / 0xFFFF'.  A sum of neighbours that carries between the
    halves of a packed 16-bit pair, or an int16 residual that wraps, shows
    here.  The row groups come first: in a frame of one to three rows a strip
    start's only neighbour across the seam can be a single column (x - 1, or
    x - T at a lens start), which in the column pattern is zero for half of
    the T, and a stale (zeroed) halo would then go unseen."""
    y = np.arange(H)[:, None]
    x = np.arange(W)[None, :]
    cols = np.where(x & 1, 0xFFFF, 0x0000)
    rows = np.where(y & 1, 0x7FFF, 0x8000)
    A = np.where((y // 3) & 1, cols, rows).astype(np.uint16)
    out = np.empty((n, H, W), np.uint16)
    for z in range(n):
        if z % 3:
            out[z] = 0xFFFF if z % 3 == 1 else 0
        else:
            out[z] = ~A if (z // 3) & 1 else A
    return out


@functools.lru_cache(maxsize=8)
def _inputs_of(O, c):
    nt = c.n + c.z0   # with the raw frame in front of an odd z0
    rng = np.random.default_rng(seed_of(c))
    lf = O.synthetic_lf(c.W, c.H, Z=nt, T=c.T, seed=seed_of(c))[0, 0].copy()
    if nt > 1:
        lf[1] = rng.integers(0, 65536, size=(c.H, c.W), dtype=np.uint16)
    noise = rng.integers(0, 65536, size=(nt, c.H, c.W), dtype=np.uint16)
    return {"lf": frozen(lf), "noise": frozen(noise), "carry": frozen(carry_stack(nt, c.H, c.W))}


def case_input(O, c, kind):
    """The case's whole stack (z0 + n frames, read-only): frames [z0:] go to
    d_in and, for an odd z0, frame z0 - 1 to d_prev."""
    return _inputs_of(O, c._replace(pieces=()))[kind]


def expected(O, c, full, fam, k):
    """The oracle's symbols of the call's frames: (n, H, W), or (7, H, W) for candidates (k ignored)."""
    if c.cands:
        return np.stack([O.predict_frame(full[0], None, c.T, fam, kk, 0) for kk in range(1, 8)])
    return O.predict_volume(full, c.T, fam, k, c.video)[c.z0:]


# ------------------------------------------------------------ sensitivity --
def _differs(O, c, full, broken, region, fams_k, good):
    """Per family: some predictor's oracle symbols of `broken` differ from
    those of `full` inside `region` (a slice triple over (frame, y, x)).
    good: the caller's dict of `full`'s symbols by (family, predictor)."""
    missing = []
    for fam in FAMS:
        for k in fams_k:
            if (fam, k) not in good:
                good[fam, k] = expected(O, c, full, fam, k)
            if not np.array_equal(good[fam, k][region], expected(O, c, broken, fam, k)[region]):
                break
        else:
            missing.append(fam)
    return missing


def stale_columns_missed(O, c, full, xs, halo, good):
    """The `halo` columns left of a strip start xs read as zeros by that strip:
    families in which no predictor's symbols at x >= xs change."""
    broken = full.copy()
    broken[:, :, max(0, xs - halo):xs] = 0
    return _differs(O, c, full, broken, (slice(None), slice(None), slice(xs, None)), range(1, 8), good)


def stale_rows_missed(O, c, full, ys, good):
    """The T + 1 rows above a piece start ys read as zeros by that piece."""
    broken = full.copy()
    broken[:, max(0, ys - c.T - 1):ys, :] = 0
    return _differs(O, c, full, broken, (slice(None), slice(ys, None), slice(None)), range(1, 8), good)


def wrong_previous_missed(O, c, full, z):
    """Temporal frame z of the whole stack takes P from itself (the frame
    pair's other ring, or d_in where d_prev belongs) instead of frame z - 1."""
    missing = []
    for fam in FAMS:
        for k in range(1, 8):
            good = O.predict_frame(full[z], full[z - 1], c.T, fam, k, 1)
            if not np.array_equal(good, O.predict_frame(full[z], full[z], c.T, fam, k, 1)):
                break
        else:
            missing.append(fam)
    return missing
