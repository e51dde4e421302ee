"""The named case lists of the GPU bzip2 decoder tests, shared by
test_bz2_craft_cpu.py (their premises, against libbzip2 on the host) and
test_bunzip2_gpu.py.  TEST INFRASTRUCTURE ONLY."""
import functools
import random

from bz2_craft import BLOCK_MAGIC, EOS_MAGIC, craft, is_periodic, patch_bits, rle1, sorted_rotations


def noruns(n, seed, alphabet=256):
    """n bytes, no two cyclically adjacent ones equal, not periodic: RLE1 is
    the identity for every rotation and the rotations are all different."""
    rnd = random.Random(seed)
    while True:
        t = []
        for i in range(n):
            c = rnd.randrange(alphabet)
            while (t and c == t[-1]) or (i == n - 1 and n > 1 and c == t[0]):
                c = rnd.randrange(alphabet)
            t.append(c)
        t = bytes(t)
        if n <= 1 or not is_periodic(t):
            return t


SWEEP_LENGTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                 9000, 100, 400, 900, 1800, 3000)  # the last five: one per libbzip2 group-count band (random bytes)


def sweep_inputs():
    rnd = random.Random(11)
    out = []
    for n in SWEEP_LENGTHS:
        out.append(bytes(rnd.randrange(256) for _ in range(n)))
        out.append(bytes(rnd.randrange(4) for _ in range(n)))
    return out


def rle_seam_inputs(fill):
    """For k = 0 .. 47: k bytes without repeats, then runs of 4 (count byte 0,
    the run's own value), 5, 8, 9 of byte 5 (count byte 5), 255 of byte 251
    (count byte 251), 256, 259, 510 and a run of 7 ending the block, `fill`
    bytes without repeats between the runs (fill 0: the text after RLE1 stays
    below 1024 bytes and most lanes hold nothing)."""
    runs = [(0, 4), (17, 5), (33, 8), (5, 9), (251, 255), (65, 256), (66, 259), (67, 510), (68, 7)]
    out = []
    for k in range(48):
        rnd = random.Random(1000 * fill + k)

        def plain(m, avoid):
            t = []
            while len(t) < m:
                c = rnd.randrange(100, 250)
                if c != (t[-1] if t else avoid):
                    t.append(c)
            return bytes(t)
        d = plain(k, -1)
        for b, m in runs:
            d += bytes([b]) * m
            if (b, m) != runs[-1]:
                d += plain(fill, b)
        out.append(d)
    return out


def periodic_inputs():
    return [b"ab" * 300, bytes([7, 9]) * 5000, bytes([1, 1, 1, 2]) * 3000, bytes(i % 251 for i in range(251 * 40))]


MARKER_NS = (1, 2, 127, 128, 129, 300, 1000, 4000)


@functools.lru_cache(maxsize=None)
def marker_cases():
    """[(text, stream, info)]: for every n and every regular marker row 128 m
    of its block, a text whose inverse-BWT walk starts on that row."""
    out = []
    for n in MARKER_NS:
        t = noruns(n, 77 + n)
        rot = sorted_rotations(t)
        for m in range((n + 127) // 128):
            s = (rot[128 * m] - 1) % n
            text = t[s:] + t[:s]
            out.append((text,) + craft(text, level=1))
    return out


def _search(make, ok, what):
    for k in range(400):
        data = make(k)
        stream, info = craft(data)
        if ok(info):
            return data, stream, info
    raise AssertionError("no input found for " + what)


@functools.lru_cache(maxsize=None)
def crafted_good():
    """[(name, data, stream, info, on_device)]: valid streams libbzip2's
    compressor would not write.  on_device: the GPU decoder decodes it (flag
    0); otherwise it hands the stream to the host (flag 1), see
    test_bunzip2_gpu.test_crafted_good."""
    rnd = random.Random(5)
    small = bytes(rnd.randrange(20) + 60 for _ in range(420))
    cases = []

    def add(name, data, on_device=True, **kw):
        stream, info = craft(data, **kw)
        cases.append((name, data, stream, info, on_device))
        return info

    alpha = len(set(rle1(small))) + 2
    for g in range(2, 7):  # table t is flat at 5 + t bits: tables differ, 9 and 10 bits pass the lookup table
        add("groups%d" % g, small, ngroups=g, lengths=[[5 + t] * alpha for t in range(g)])
    add("all20", small, ngroups=2, lengths=[[20] * alpha] * 2)
    add("len17to20", small, ngroups=3, lengths=[[17 + (k + t) % 4 for k in range(alpha)] for t in range(3)])
    add("flat9", small, ngroups=2, lengths=[[9] * alpha] * 2)
    for r in (0, 1):
        d, s, i = _search(lambda k: small[:150 + k], lambda i: i["nsym"] % 50 == r, "nsym %% 50 == %d" % r)
        cases.append(("nsym_mod50_%d" % r, d, s, i, True))
    d, s, i = _search(lambda k: noruns(k, 3, 40) + b"xy" * 150,
                      lambda i: any(nd >= 3 and a // 50 != (a + nd - 1) // 50 for a, nd in i["runs"]),
                      "run over a seam")
    cases.append(("run_straddle", d, s, i, True))
    add("ninuse1_n1", b"q")
    add("ninuse1_n5", bytes([5]) * 9, on_device=False)   # RLE1 text 5 5 5 5 5: constant, so periodic
    add("ninuse2", b"abaabbab")
    d, s, i = _search(lambda k: bytes(random.Random(k).sample(range(256), 256)) +
                      bytes(random.Random(k).randrange(256) for _ in range(2400)),
                      lambda i: i["ninuse"] == 256 and i["maxpos"] == 255, "MTF position 255")
    cases.append(("ninuse256", d, s, i, True))
    add("extra_sel5", small, extra_sel=5, on_device=False)  # EOB before the last selector
    return cases


@functools.lru_cache(maxsize=None)
def crafted_bad():
    """[(name, stream, flag)]: streams libbzip2 rejects, each aimed at one
    check of the GPU decoder; flag is what the decoder must answer."""
    data = noruns(300, 9, 50)
    base, info = craft(data, ngroups=2)
    b, n = info["bits"], info["n"]
    long_, long_info = craft(noruns(700, 10, 50), ngroups=2)
    mid = (b["symbols"] + (b["eos"] - b["symbols"]) // 2) // 8
    return [
        ("trunc13", base[:13], 1),
        ("trunc_symbols", base[:mid], 1),
        ("block_magic", patch_bits(base, b["magic"], 48, BLOCK_MAGIC ^ 1), 1),
        # (700 bytes: libbzip2 still decodes randomised blocks, and its table first flips byte 618)
        ("randomised", patch_bits(long_, long_info["bits"]["rand"], 1, 1), 1),
        ("orig_eq_n", craft(data, ngroups=2, orig_override=n)[0], 1),
        ("orig_max", craft(data, ngroups=2, orig_override=0xFFFFFF)[0], 1),
        ("ngroups1", patch_bits(base, b["ngroups"], 3, 1), 1),
        ("ngroups7", patch_bits(base, b["ngroups"], 3, 7), 1),
        ("nsel0", patch_bits(base, b["nsel"], 15, 0), 1),
        ("selector_unary", patch_bits(base, b["selectors"], 2, 3), 1),
        ("startlen0", patch_bits(base, b["tables"][0], 5, 0), 1),
        ("startlen21", patch_bits(base, b["tables"][0], 5, 21), 1),
        ("eos_magic", patch_bits(base, b["eos"], 48, EOS_MAGIC ^ 1), 1),
        ("combined_crc", patch_bits(base, b["ccrc"], 32, info["crc"] ^ 1), 1),
        ("crc_both", craft(data, ngroups=2, crc_override=info["crc"] ^ 0x80000000)[0], 2),
        ("orig_wrong", craft(data, ngroups=2, orig_override=(info["orig"] + 1) % n)[0], 2),
    ]


def chain_wraps(text, orig):
    """A model of bzd_walk's marker chain for the block `text` (after RLE1)
    with origPtr `orig`: True if a chain that only counts segments and bytes
    (off == n and k == nwalk), without noticing that it is back at its first
    segment, would accept the block although its LF permutation has several
    cycles.  tt as decompress.c builds it; a marker every 128 rows and v0."""
    n = len(text)
    rot = sorted_rotations(text)
    ll = [text[i - 1] for i in rot]
    cf, tt = {}, [0] * n
    for c in sorted(set(ll)):
        cf[c] = sum(1 for x in ll if x < c)
    for i, c in enumerate(ll):
        tt[cf[c]] = i
        cf[c] += 1
    seen, pos = 0, tt[orig]
    while True:  # the cycle of the start node
        seen, pos = seen + 1, tt[pos]
        if pos == tt[orig]:
            break
    if seen == n:
        return False
    v0, nm = tt[orig], (n + 127) // 128
    nodes = [128 * i for i in range(nm)] + ([v0] if v0 % 128 else [])
    ident = {node: i for i, node in enumerate(nodes)}
    mlen, mnext = [], []
    for node in nodes:
        pos, ln = tt[node], 1
        while pos not in ident:
            pos, ln = tt[pos], ln + 1
        mlen.append(ln)
        mnext.append(ident[pos])
    i, off, k = ident[v0], 0, 0
    while k < len(nodes) and off < n:
        off, i, k = off + mlen[i], mnext[i], k + 1
    return off == n and k == len(nodes)


@functools.lru_cache(maxsize=None)
def repeated_cases():
    """[(text, stream, wraps)]: a text w w of at most 128 bytes, or w w w of
    129 .. 256, once for each of the equal sorted rows its origPtr may name.
    With two (three) walkers, one per cycle, two (three) trips round the
    start's cycle visit as many segments and bytes as the block has
    (wraps: chain_wraps says so for this origPtr)."""
    out = []
    for r, m, seed in ((2, 2, 16), (2, 31, 1), (2, 64, 2), (3, 43, 3), (3, 85, 4)):
        text = noruns(m, seed, 200) * r
        rot = sorted_rotations(text)
        for j in range(r):
            orig = rot.index(j * m)
            out.append((text, craft(text, level=1, orig_override=orig)[0], chain_wraps(text, orig)))
    return out
