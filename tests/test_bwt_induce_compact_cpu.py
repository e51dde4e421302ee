"""A NumPy model of the two-stage BWT's compact induction scan, checked against
a naive sort of all rotations.

One rotation type is sorted, the other ("placed") is put in order by one scan
of the sorted order.  A placed rotation p induces p - 1 only when p - 1 is
placed too: it is "live".  The scan visits only the sorted rotations and the
live ones, through a compact index: per bucket in scan order, first the slots
of its live rotations, then its sorted rotations.  Every induced rotation's
BWT symbol goes straight to ll[] at its final position; only a live one gets
an entry in the compact index.

The model below is sequential and written from that description alone: types,
live[] by the byte rule, the compact layout, the entries' fields, the `dest`
(head) and compact (chead) counters.  It also provides the stream shapes and
the mode rule for the GPU tests of the same scan (test_bwt_induce_compact_gpu).
"""
import numpy as np
import pytest

SORT_A, SORT_B, FULL = 0, 1, 2  # which rotations go through the sort
PLACED = 1 << 23
PEND = (0xFFFFFFFF, 0)


# ------------------------------------------------------------- the text --
def rle1(data):
    """bzip2's first run-length step: a run of 4..255 equal bytes becomes 4
    bytes and a count of the rest.  The BWT sees this text."""
    data = bytes(data)
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 255:
            j += 1
        run = j - i
        out += data[i:i + 1] * min(run, 4)
        if run >= 4:
            out.append(run - 4)
        i = j
    return np.frombuffer(bytes(out), np.uint8).copy()


def is_periodic(T):
    T = np.asarray(T, np.uint8)
    n = len(T)
    return any(n % d == 0 and np.array_equal(T, np.roll(T, d)) for d in range(1, n // 2 + 1))


def placed_types(Tp):
    """Tp: the text with bytes in scan terms.  Rotation i is placed by the scan
    when Tp[i] > Tp[i+1], or they are equal and i + 1 is placed (cyclic)."""
    n = len(Tp)
    t = Tp.astype(np.int16)
    d = np.sign(t - np.roll(t, -1))
    nz = np.flatnonzero(d)
    assert len(nz), "a constant text is periodic"
    nxt = nz[np.searchsorted(nz, np.arange(n)) % len(nz)]
    return d[nxt] > 0


def scan_view(T, mode):
    """(mirror, placed[]) of a text in `mode`: kModeSortA sorts the A rotations
    and scans right to left with mirrored bytes, kModeSortB sorts the B ones."""
    mir = 255 if mode == SORT_A else 0
    return mir, placed_types(np.asarray(T, np.uint8) ^ mir)


def live_rule(T, mode):
    """The byte rule: would rotation k, if placed, induce k - 1?"""
    prev = np.roll(T, 1)
    return prev <= T if mode == SORT_A else prev >= T


def kernel_mode(T):
    """The mode the encoder picks: the A rotations are sorted unless the B ones
    are fewer by 1/8; a type still undecided after 8 equal bytes (9 equal
    bytes in a row) sends the stream through the sort whole."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    ext = np.concatenate([T, T[:8]])
    same = np.ones(n, bool)
    for d in range(1, 9):
        same &= ext[d:d + n] == T
    if same.any():
        return FULL
    _, placed = scan_view(T, SORT_A)
    nb = int(placed.sum())
    return SORT_A if nb * 8 >= (n - nb) * 7 else SORT_B


def compact_length(T, mode):
    T = np.asarray(T, np.uint8)
    _, placed = scan_view(T, mode)
    return int((~placed).sum() + (placed & live_rule(T, mode)).sum())


def rot0_role(T, mode):
    T = np.asarray(T, np.uint8)
    _, placed = scan_view(T, mode)
    if not placed[0]:
        return "sorted"
    return "live" if live_rule(T, mode)[0] else "dead"


# ------------------------------------------------------------ reference --
def naive_bwt(T):
    T = np.asarray(T, np.uint8)
    n = len(T)
    tb = T.tobytes() * 2
    sa = sorted(range(n), key=lambda i: tb[i:i + n])
    u2s = np.cumsum(np.bincount(T, minlength=256) > 0) - 1
    ll = u2s[T[(np.array(sa) - 1) % n]].astype(np.uint8)
    return ll, sa.index(0)


# ---------------------------------------------------------------- model --
def model(T, mode):
    """ll[], origPtr and counts of the compact scan of text T in `mode`."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    tl = T.tolist()

    def t(k):  # cyclic
        return tl[k % n]

    rev = mode == SORT_A
    mir, placed = scan_view(T, mode)
    u2s = (np.cumsum(np.bincount(T, minlength=256) > 0) - 1).tolist()

    # step 1: per first byte, the sorted, the placed and the live rotations
    nsort = np.bincount(T[~placed], minlength=256).tolist()
    nplaced = np.bincount(T[placed], minlength=256).tolist()
    live = np.bincount(T[placed & live_rule(T, mode)], minlength=256).tolist()

    # the sort stage: the sorted-type rotations in their final order
    tb = T.tobytes() * 2
    sa = sorted(np.flatnonzero(~placed).tolist(), key=lambda i: tb[i:i + n])

    # step 2: the layouts.  Final order: bucket c holds its A rotations, then
    # its B rotations.  Scan order: position v = q (kModeSortB) or n - 1 - q,
    # bucket u = c ^ mir, the placed part first.
    tq, s0, q, j = [0] * 256, [0] * 256, 0, 0
    for c in range(256):
        tq[c] = q + (nplaced[c] if mode == SORT_B else 0)
        s0[c] = j
        q += nsort[c] + nplaced[c]
        j += nsort[c]
    head, hlim, cs, clim, v, k = [0] * 256, [0] * 256, [0] * 256, [0] * 256, 0, 0
    for u in range(256):
        c = u ^ mir
        head[u], hlim[u] = v, v + nplaced[c]
        cs[u], clim[u] = k, k + live[c]
        v += nplaced[c] + nsort[c]
        k += live[c] + nsort[c]
    nc = k
    chead = list(cs)
    enter = {}  # compact index at which the scan enters a bucket's sorted part
    for u in range(256):
        enter.setdefault(clim[u], []).append(u)

    # step 3: the sorted entries, their symbols, the pending live slots
    ll = [None] * n
    orig = None
    ent = [None] * nc
    for u in range(256):
        for x in range(cs[u], clim[u]):
            ent[x] = PEND
    for j, i in enumerate(sa):
        c = t(i)
        r = j - s0[c]
        assert 0 <= r < nsort[c]
        qq = tq[c] + r
        assert ll[qq] is None
        ll[qq] = u2s[t(i - 1)]
        if i == 0:
            orig = qq
        u = c ^ mir
        x = clim[u] + (nsort[c] - 1 - r if rev else r)
        assert ent[x] is None
        ent[x] = (i | 3 << 20 | t(i - 1) << 24, t(i - 2) | t(i - 3) << 8 | t(i - 4) << 16 | c << 24)

    # step 4: the scan
    written = 0
    for v in range(nc):
        for u in enter.get(v, ()):
            assert chead[u] == clim[u], ("live slots of bucket", u, chead[u], clim[u])
        e = ent[v]
        assert e is not None and e != PEND, ("compact index not filled", v)
        lo, hi = e
        i, nprev = lo & 0xFFFFF, (lo >> 20) & 7
        b, u = (lo >> 24) ^ mir, (hi >> 24) ^ mir
        if not (b > u or (b == u and lo & PLACED)):
            continue
        p = i - 1 if i else n - 1
        if nprev >= 1:  # the carried byte
            y = hi & 0xFF
            plo = p | (nprev - 1) << 20 | PLACED | y << 24
            phi = (hi >> 8) & 0xFFFF | lo & 0xFF000000
        else:           # a chain longer than the carried bytes: the text
            y = t(p - 1)
            plo = p | 3 << 20 | PLACED | y << 24
            phi = t(p - 2) | t(p - 3) << 8 | t(p - 4) << 16 | lo & 0xFF000000
        assert y == t(p - 1) and lo >> 24 == t(p)
        dest = head[b]
        head[b] += 1
        assert dest < hlim[b]
        qq = n - 1 - dest if rev else dest
        assert ll[qq] is None
        ll[qq] = u2s[y]
        if p == 0:
            assert orig is None
            orig = qq
        if (y ^ mir) >= b:  # live: it will induce in its turn
            x = chead[b]
            chead[b] += 1
            assert v < x < clim[b] and ent[x] == PEND
            ent[x] = (plo, phi)
            written += 1
    assert head == hlim and chead == clim
    assert written == sum(live), ("live count", sum(live), "written", written)
    assert None not in ll and orig is not None
    return np.array(ll, np.uint8), orig, {"nc": nc, "live": sum(live), "placed": int(placed.sum())}


def check(T, mode):
    ll, orig, info = model(T, mode)
    ll_ref, orig_ref = naive_bwt(T)
    assert orig == orig_ref, (mode, orig, orig_ref)
    assert np.array_equal(ll, ll_ref), mode
    assert info["nc"] == compact_length(T, mode)
    return info


# --------------------------------------------------------- stream shapes --
def bench_like(n, seed, p=0.05, swap=False):
    """16-bit little-endian symbols, geometric values with zeros: the placed
    rotations start at the high bytes and few of them are live."""
    rng = np.random.default_rng(seed)
    v = (rng.geometric(p, (n + 1) // 2) - 1).astype("<u2")
    if swap:
        v = v.byteswap()
    return v.view(np.uint8)[:n].copy()


def ascending_runs(n, seed):
    """Strictly ascending runs of 3..20 bytes: nearly every placed rotation is
    live, in chains longer than the bytes an entry carries."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x = int(rng.integers(0, 150))
        for _ in range(int(rng.integers(3, 21))):
            out.append(x)
            x += int(rng.integers(1, 5))
    return np.array(out[:n], np.uint8)


def descending_runs(n, seed):
    return (255 - ascending_runs(n, seed)).astype(np.uint8)


def triples_b(n, seed):
    """(0, x, y) with x > y > 0: one rotation in three is of type B."""
    rng = np.random.default_rng(seed)
    k = (n + 2) // 3
    y = rng.integers(1, 200, k)
    x = y + rng.integers(1, 56, k)
    return np.stack([np.zeros(k, np.int64), x, y], 1).reshape(-1)[:n].astype(np.uint8)


def threes(n, seed):
    """Bytes in threes (c c c, the next c different): chains inside one bucket
    that land in the slice being scanned."""
    rng = np.random.default_rng(seed)
    k = (n + 2) // 3
    c = rng.integers(0, 8, k)
    for i in range(1, k):
        if c[i] == c[i - 1]:
            c[i] = (c[i] + 1 + rng.integers(0, 7)) % 8
    return np.repeat(c * 31 + 2, 3)[:n].astype(np.uint8)


def rot0_in_role(n, seed, role):
    """Rotation 0 as a sorted, a dead or a live rotation of a kModeSortA
    stream (16 symbols): by the first two bytes and the last one."""
    rng = np.random.default_rng(seed)
    T = rng.integers(1, 15, n).astype(np.uint8)
    T[0], T[1], T[-1] = {"sorted": (15, 0, 7), "dead": (1, 15, 9), "live": (5, 15, 2)}[role]
    return T


def all_bytes(n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(256), rng.integers(0, 256, n - 256)]).astype(np.uint8)


def five_bytes(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 5, n)
    for i in range(3, n):  # no run of four: the first run-length step adds no count bytes
        if k[i] == k[i - 1] == k[i - 2] == k[i - 3]:
            k[i] = (k[i] + 1 + rng.integers(0, 4)) % 5
    return np.array([3, 70, 71, 200, 255], np.uint8)[k]


# (name, raw stream, the mode it must run in, or None); the lengths' seeds are
# chosen so that the compact lengths sit on, before and after slice and block
# edges (LENGTH_CASES: length, seed, p, compact length)
LENGTH_CASES = [
    (511, 61, 0.2, 319), (512, 99, 0.03, 257), (513, 61, 0.2, 320), (1023, 274, 0.1, 575), (1025, 274, 0.1, 576),
    (4097, 205, 0.04, 2113), (20000, 78, 0.08, 10751), (20000, 109, 0.08, 10752), (20000, 34, 0.08, 10753),
]


def shapes(cut=None):
    """The stream shapes of the GPU tests; cut: at most that many bytes."""
    def c(n):
        return n if cut is None else min(n, cut)
    out = [
        ("bench_like", bench_like(c(20000), 1), SORT_A),
        ("bench_like_swapped", bench_like(c(20000), 1, swap=True), None),
        ("ascending_runs", ascending_runs(c(12000), 2), SORT_A),
        ("descending_runs", descending_runs(c(12000), 2), SORT_B),
        ("triples_b", triples_b(c(12000), 3), SORT_B),
        ("threes", threes(c(9000), 4), None),
        ("rot0_sorted", rot0_in_role(c(3000), 5, "sorted"), SORT_A),
        ("rot0_dead", rot0_in_role(c(3000), 5, "dead"), SORT_A),
        ("rot0_live", rot0_in_role(c(3000), 5, "live"), SORT_A),
        ("all_bytes", all_bytes(c(8000), 6), None),
        ("five_bytes", five_bytes(c(8000), 7), None),
    ]
    for n, seed, p, nc in LENGTH_CASES:
        out.append(("len_%d_nc_%d" % (n, nc), bench_like(c(n), seed, p), SORT_A))
    return out


# ---------------------------------------------------------------- tests --
ALPHABETS = (2, 3, 4, 16, 256)


def random_texts(count, seed):
    rng = np.random.default_rng(seed)
    for k in range(count):
        a = ALPHABETS[k % len(ALPHABETS)]
        while True:
            n = int(rng.integers(2, 401))
            T = rng.integers(0, a, n).astype(np.uint8)
            if a < 256 and k % 2:  # not only the lowest byte values
                T = (T * (255 // (a - 1))).astype(np.uint8)
            if not is_periodic(T):
                break
        yield T


@pytest.mark.parametrize("part", range(4))
def test_compact_scan_matches_naive_sort_on_random_texts(part):
    """3 200 seeded random non-periodic texts, lengths 2..400, alphabets of 2,
    3, 4, 16 and 256 symbols, both modes forced on each."""
    n_live = n_placed = 0
    for T in random_texts(800, 0x1DC0 + part):
        for mode in (SORT_A, SORT_B):
            info = check(T, mode)
            n_live += info["live"]
            n_placed += info["placed"]
    assert 0 < n_live < n_placed  # both live and dead placed rotations were met


def test_tiny_texts_exhaustively():
    """Every non-periodic text of 2..7 symbols over 3 symbols, both modes."""
    for n in range(2, 8):
        for k in range(3 ** n):
            T = np.array([(k // 3 ** d) % 3 for d in range(n)], np.uint8)
            if not is_periodic(T):
                check(T, SORT_A)
                check(T, SORT_B)


@pytest.mark.parametrize("name,raw,want", shapes(5000), ids=[s[0] for s in shapes(5000)])
def test_compact_scan_on_the_gpu_tests_shapes(name, raw, want):
    """The GPU tests' stream shapes, cut to 5 000 bytes: the model in the mode
    the encoder picks, and in the other one."""
    T = rle1(raw)
    assert not is_periodic(T)
    mode = kernel_mode(T)
    for m in (SORT_A, SORT_B):
        info = check(T, m)
        if m == mode:
            print("%s: n %d mode %d compact length %d live %d placed %d" %
                  (name, len(T), m, info["nc"], info["live"], info["placed"]))


def test_shapes_are_what_they_claim():
    """Full-size shapes: the mode each must run in, rotation 0's three roles,
    mostly-dead and mostly-live streams, identity and non-identity byte maps."""
    got = {name: (rle1(raw), want) for name, raw, want in shapes()}
    for name, (T, want) in got.items():
        assert want is None or kernel_mode(T) == want, name
    for role in ("sorted", "dead", "live"):
        T = got["rot0_" + role][0]
        assert rot0_role(T, kernel_mode(T)) == role
    def live_share(name):
        T = got[name][0]
        m = kernel_mode(T)
        _, placed = scan_view(T, m)
        return (placed & live_rule(T, m)).sum() / placed.sum()
    assert live_share("bench_like") < 0.1
    assert live_share("ascending_runs") > 0.85 and live_share("descending_runs") > 0.85
    assert len(np.unique(got["all_bytes"][0])) == 256 and len(np.unique(got["five_bytes"][0])) == 5


def test_length_cases_cover_slice_and_block_edges():
    """The compact lengths of the length cases fall on, before and after an
    edge of a 64-index slice and of a 512-index block of the scan."""
    ncs = []
    for n, seed, p, nc in LENGTH_CASES:
        T = rle1(bench_like(n, seed, p))
        got = compact_length(T, kernel_mode(T))
        print("length %d: text %d bytes, compact length %d" % (n, len(T), got))
        assert got == nc and kernel_mode(T) == SORT_A
        ncs.append(got)
    assert {n for n, _, _, _ in LENGTH_CASES} == {511, 512, 513, 1023, 1025, 4097, 20000}
    assert {0, 1, 511} <= {x % 512 for x in ncs}
    assert {0, 1, 63} <= {x % 64 for x in ncs if x % 512 not in (0, 1, 511)}
