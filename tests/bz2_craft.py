"""A pure-Python writer of single-block bzip2 streams, written from the file
format, for the decoder tests: it can emit what libbzip2's compressor never
does (chosen group counts, selectors, code lengths up to 20, a wrong origPtr or
CRC) and reports the facts a test asserts on.  TEST INFRASTRUCTURE ONLY.

    stream, info = craft(data, level=9, ngroups=..., selectors=..., extra_sel=...,
                         lengths=..., orig_override=..., crc_override=...)

info: n (bytes after RLE1), text (those bytes), nsym (symbols, EOB included),
maxlen / minlen (longest / shortest code written), ninuse, maxpos (largest
move-to-front position used), orig, v0 (the sorted row of rotation 1: the node
the decoder's inverse BWT starts from), ngroups, nsel, runs ([(first symbol,
digits)] of the RUNA/RUNB runs), crc and bits (bit offset of every field).

tests/bz2_cases.py builds the decoder tests' case lists with it.
"""
import heapq

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090

_CRC = []
for _i in range(256):
    _c = _i << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04C11DB7 if _c & 0x80000000 else _c << 1) & 0xFFFFFFFF
    _CRC.append(_c)


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _CRC[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def rle1(data):
    """Runs of 4..255 equal bytes become 4 bytes and a count of 0..251."""
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 255:
            j += 1
        out += data[i:i + 1] * min(j - i, 4)
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def sorted_rotations(text):
    n, t2 = len(text), text + text
    return sorted(range(n), key=lambda i: t2[i:i + n])


def _mtf_runs(last, used):
    order, syms, runs, run, maxpos = list(used), [], [], 0, 0

    def flush(run):
        if run:
            runs.append((len(syms), 0))
        while run > 0:  # bijective base 2: RUNA = 1, RUNB = 2
            syms.append(0 if run & 1 else 1)
            run = (run - 1) >> 1 if run & 1 else (run - 2) >> 1
            runs[-1] = (runs[-1][0], runs[-1][1] + 1)

    for b in last:
        p = order.index(b)
        if p == 0:
            run += 1
            continue
        flush(run)
        run, maxpos = 0, max(maxpos, p)
        order.insert(0, order.pop(p))
        syms.append(p + 1)
    flush(run)
    syms.append(len(used) + 1)  # EOB
    return syms, runs, maxpos


def huff_lengths(freq, maxlen=17):
    f = [max(1, x) for x in freq]
    while True:
        heap = [(w, k, [k]) for k, w in enumerate(f)]
        heapq.heapify(heap)
        ln = [0] * len(f)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for k in a[2] + b[2]:
                ln[k] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(ln) <= maxlen:
            return ln
        f = [x // 2 + 1 for x in f]


def assign_codes(lengths):
    """Canonical codes, shortest first, symbols in order within a length."""
    codes, vec = [0] * len(lengths), 0
    for n in range(min(lengths), max(lengths) + 1):
        for k, l in enumerate(lengths):
            if l == n:
                codes[k] = vec
                vec += 1
        vec <<= 1
    return codes


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, nbits, v):
        assert 0 <= v < (1 << nbits)
        self.acc, self.n = (self.acc << nbits) | v, self.n + nbits

    def bytes(self):
        pad = -self.n % 8
        return ((self.acc << pad).to_bytes((self.n + pad) // 8, "big"))


def default_ngroups(nsym):
    return 2 if nsym < 200 else 3 if nsym < 600 else 4 if nsym < 1200 else 5 if nsym < 2400 else 6


def craft(data, level=9, ngroups=None, selectors=None, extra_sel=0, lengths=None, orig_override=None,
          crc_override=None):
    data = bytes(data)
    text = rle1(data)
    n = len(text)
    assert 0 < n <= 100000 * level - 19
    rot = sorted_rotations(text)
    t2 = text + text
    last = bytes(t2[i + n - 1] for i in rot)
    orig, v0 = rot.index(0), rot.index(1 % n)
    used = sorted(set(text))
    syms, runs, maxpos = _mtf_runs(last, used)
    alpha = len(used) + 2
    ngroups = default_ngroups(len(syms)) if ngroups is None else ngroups
    nused = (len(syms) + 49) // 50
    selectors = [g % ngroups for g in range(nused)] if selectors is None else list(selectors)
    assert len(selectors) == nused
    selectors += [0] * extra_sel
    if lengths is None:
        freq = [0] * alpha
        for s in syms:
            freq[s] += 1
        lengths = [huff_lengths(freq)] * ngroups
    assert len(lengths) == ngroups and all(len(ln) == alpha for ln in lengths)
    codes = [assign_codes(ln) for ln in lengths]
    crc = crc32(data) if crc_override is None else crc_override
    w, bits = _Bits(), {}

    def field(name, nbits, v):
        bits[name] = w.n
        w.put(nbits, v)

    w.put(24, 0x425A68)
    w.put(8, ord("0") + level)
    field("magic", 48, BLOCK_MAGIC)
    field("crc", 32, crc)
    field("rand", 1, 0)
    field("orig", 24, orig if orig_override is None else orig_override)
    rows = [sum(1 << (15 - j) for j in range(16) if 16 * i + j in used) for i in range(16)]
    w.put(16, sum(1 << (15 - i) for i in range(16) if rows[i]))
    for r in rows:
        if r:
            w.put(16, r)
    field("ngroups", 3, ngroups)
    field("nsel", 15, len(selectors))
    bits["selectors"] = w.n
    order = list(range(ngroups))
    for s in selectors:  # move-to-front position in unary
        p = order.index(s)
        order.insert(0, order.pop(p))
        w.put(p + 1, (1 << (p + 1)) - 2)
    bits["tables"] = []
    for ln in lengths:
        bits["tables"].append(w.n)
        curr = ln[0]
        w.put(5, curr)
        for l in ln:
            while curr != l:
                w.put(2, 2 if curr < l else 3)
                curr += 1 if curr < l else -1
            w.put(1, 0)
    bits["symbols"] = w.n
    maxlen, minlen = 0, 99
    for k, s in enumerate(syms):
        t = selectors[k // 50]
        w.put(lengths[t][s], codes[t][s])
        maxlen, minlen = max(maxlen, lengths[t][s]), min(minlen, lengths[t][s])
    field("eos", 48, EOS_MAGIC)
    field("ccrc", 32, crc)
    info = dict(n=n, text=text, nsym=len(syms), maxlen=maxlen, minlen=minlen, ninuse=len(used), maxpos=maxpos,
                orig=orig, v0=v0, ngroups=ngroups, nsel=len(selectors), runs=runs, crc=crc, bits=bits)
    return w.bytes(), info


# ------------------------------------------------- reading and patching --
def get_bits(stream, pos, nbits):
    v = int.from_bytes(stream[pos // 8:(pos + nbits + 7) // 8], "big")
    return (v >> (-(pos + nbits) % 8)) & ((1 << nbits) - 1)


def patch_bits(stream, pos, nbits, value):
    total = 8 * len(stream)
    v = int.from_bytes(stream, "big")
    sh = total - pos - nbits
    v = (v & ~(((1 << nbits) - 1) << sh)) | (value << sh)
    return v.to_bytes(len(stream), "big")


def parse(stream):
    """Header facts of any single-block stream (libbzip2's included)."""
    assert stream[:3] == b"BZh" and get_bits(stream, 32, 48) == BLOCK_MAGIC
    pos = 32 + 48 + 32 + 1
    orig = get_bits(stream, pos, 24)
    in16 = get_bits(stream, pos + 24, 16)
    pos += 40
    ninuse = 0
    for _ in range(bin(in16).count("1")):
        ninuse += bin(get_bits(stream, pos, 16)).count("1")
        pos += 16
    return dict(level=stream[3] - 48, crc=get_bits(stream, 80, 32), orig=orig, ninuse=ninuse,
                ngroups=get_bits(stream, pos, 3), nsel=get_bits(stream, pos + 3, 15))


def set_crcs(stream, crc):
    """The same stream with both CRC fields (block and combined) replaced."""
    ends = [8 * len(stream) - pad - 80 for pad in range(8)
            if get_bits(stream, 8 * len(stream) - pad - 80, 48) == EOS_MAGIC]
    assert len(ends) == 1
    return patch_bits(patch_bits(stream, 80, 32, crc), ends[0] + 48, 32, crc)


def is_periodic(text):
    return (text + text).find(text, 1) < len(text)
