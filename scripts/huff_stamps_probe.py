"""Phase stamps of the Huffman stage's latency chains, from a liblfm.so built
with -DLFM_HUFF_STAMPS (make HIPFLAGS+=..., see csrc/lfm_bzip2.hip HuffStamps;
point LFM_LIB at it): one GPU-bzip2 batch of config-3 symbols as in
scripts/bz_probe.py, then the medians over the workgroups of the clock ticks
each phase of huff_lengths_heap and each half of huff_final took, and each
phase's share of its kernel's sum.  A workgroup's value of a phase is the
largest over its lanes and over the batch's four huff_lengths_heap launches,
taken apart from the other phases', and the medians are summed over phases:
the sum is not one launch's chain and the shares are approximate.
usage: python scripts/huff_stamps_probe.py [out.json] [streams]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lightfieldmicroscopy_pc-bzip2_amd"))
import lfm  # noqa: E402

X, Y, Z, T = 2048, 2048, 64, 15
WGS, SLOTS = 4096, 8
HEAP = ("fill_and_freq_loads", "inserts", "pref_build", "merge_trips", "depth_pass", "length_stores")
FINAL = ("selector_wave", "table0_wave")
out_path = sys.argv[1] if len(sys.argv) > 1 else None
count = int(sys.argv[2]) if len(sys.argv) > 2 else 1936
torch.cuda.set_device(0)
lfm.require_gpu()
fn = getattr(lfm.lib(), "lfm_hip_huff_stamps", None)
if fn is None:
    sys.exit("this liblfm.so was built without -DLFM_HUFF_STAMPS")
d = torch.empty((Z, Y, X), dtype=torch.int16, device="cuda")
lfm.synth_device(d, X, Y, Z, T, t_index=0, idx0=0, seed=0x4C464D03)
sym = torch.empty_like(d)
lfm.predict_device(d, sym, X, Y, Z, T, "angle", 4)
torch.cuda.synchronize()
buf = np.zeros((2, WGS, SLOTS), dtype=np.uint64)
ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))
res = {}
for rep in range(2):  # the first call warms up; the second is reported
    lfm.bzip2_device(sym, [X, Y, Z, 1, 1], [96, 96, 8, 1, 1], 2, count=count)
    torch.cuda.synchronize()
    if fn(ptr) != 0:
        sys.exit("lfm_hip_huff_stamps failed")
for row, names in ((0, HEAP), (1, FINAL)):
    live = buf[row][buf[row].sum(axis=1) > 0]
    med = [float(np.median(live[:, p])) for p in range(len(names))]
    total = sum(med) if row == 0 else None
    for p, name in enumerate(names):
        res[name] = {"median_ticks": med[p], "workgroups": int(len(live))}
        if total:
            res[name]["share"] = round(med[p] / total, 4)
    print(("huff_lengths_heap" if row == 0 else "huff_final"), {n: res[n] for n in names}, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
