"""One GPU-bzip2 batch of 1 936 streams of 147 456 bytes, alone on the device
(no second batch overlapping it): a short program for rocprofv3 kernel traces
of the MTF stage (mtf_last, mtf_prefix, mtf_win, rle2).  A parent build is
loaded through LFM_LIB.

usage: python scripts/mtf_probe.py config3|random [reps] [streams]
       python scripts/mtf_probe.py heads [blocks]

config3  the bench's config-3 symbols (angle, P4), as scripts/bz_probe.py
random   uniformly random bytes of the same geometry: every column position
         is a run head, the worst case of mtf_win's run-head walk
heads    no encode: downloads `blocks` (default 6) config-3 blocks spread over
         the batch, compresses them with the reference bzip2 on the host and
         prints the head fraction and the heads per 4 096-position segment of
         each reference column (bz2_dissect.bwt_column)"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("lightfieldmicroscopy_pc-bzip2_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(HERE, "..", p))
import lfm  # noqa: E402

X, Y, Z, T = 2048, 2048, 64, 15
BS = [96, 96, 8, 1, 1]
SEG = 4096
what = sys.argv[1] if len(sys.argv) > 1 else "config3"
assert what in ("config3", "random", "heads"), __doc__
torch.cuda.set_device(0)
lfm.require_gpu()
if what == "random":
    g = torch.Generator(device="cuda")
    g.manual_seed(0x4C464D03)
    sym = torch.randint(0, 256, (Z, Y, 2 * X), dtype=torch.uint8, device="cuda", generator=g).view(torch.int16)
else:
    d = torch.empty((Z, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d, X, Y, Z, T, t_index=0, idx0=0, seed=0x4C464D03)
    sym = torch.empty_like(d)
    lfm.predict_device(d, sym, X, Y, Z, T, "angle", 4)
torch.cuda.synchronize()

if what == "heads":
    import lfm_oracle
    from bz2_dissect import bwt_column, dissect, mvals

    nblocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    nb = [-(-a // b) for a, b in zip((X, Y, Z), BS[:3])]
    total = nb[0] * nb[1] * nb[2]
    bz = lfm_oracle.bzip2()
    fracs = []
    for k in np.linspace(0, 1935, nblocks).astype(int).tolist():
        i, j, z = k % nb[0], k // nb[0] % nb[1], k // (nb[0] * nb[1])
        blk = sym[z * BS[2]:(z + 1) * BS[2], j * BS[1]:(j + 1) * BS[1], i * BS[0]:(i + 1) * BS[0]].contiguous().cpu().numpy()
        dd = dissect(bz.compress(blk.tobytes(), 2))
        col = bwt_column(mvals(dd["syms"])[0], dd["used"])
        h = np.ones(len(col), bool)
        h[1:] = col[1:] != col[:-1]
        h[::SEG] = True
        per = [int(h[a:a + SEG].sum()) for a in range(0, len(col), SEG)]
        fracs.append(float(h.mean()))
        print("block %d of %d (%s bytes, %s): column %d, used symbols %d, head fraction %.4f, windows %d -> %d, heads per segment %s" %
              (k, total, blk.nbytes, bz.kind, len(col), len(dd["used"]), fracs[-1], -(-len(col) // 64),
               sum(-(-p // 64) for p in per), per), flush=True)
    print("head fraction over %d blocks: min %.4f mean %.4f max %.4f" % (len(fracs), min(fracs), sum(fracs) / len(fracs), max(fracs)))
    sys.exit(0)

reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
count = int(sys.argv[3]) if len(sys.argv) > 3 else 1936
for r in range(reps):
    t0 = time.time()
    out, flags = lfm.bzip2_device(sym, [X, Y, Z, 1, 1], BS, 2, count=count)
    torch.cuda.synchronize()
    print("%s rep %d: %.2f ms wall (incl. workspace alloc + D2H), %d host-flagged, %d bytes" %
          (what, r, 1e3 * (time.time() - t0), sum(flags), sum(len(o) for o in out if o)), flush=True)
    st = (ctypes.c_float * 5)()
    if lfm.lib().lfm_hip_bzip2_last_stage_ms(st) == 0:
        print("  stages ms: rle1 %.3f bwt %.3f mtf %.3f huffman %.3f emit %.3f" % tuple(st), flush=True)
