#!/usr/bin/env python3
"""lfm_hip_crop_region on boxes of a config-3-sized image (2048 x 2048 x 64
uint16): ms per call (HIP events around 20 calls after 3 warm-up calls) and
GB/s of bytes read + written, next to torch's strided copy of the same box.
One JSON line per box (profiles/crop_region_probe.jsonl)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "lightfieldmicroscopy_pc-bzip2_amd"))
import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, Z = 2048, 2048, 64
src = torch.randint(-30000, 30000, (1, 1, Z, Y, X), dtype=torch.int16, device="cuda")


def timed(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it


for name, lb, n in (("identity", [0, 0, 0], [X, Y, Z]), ("aligned16", [128, 64, 0], [1792, 1900, Z]),
                    ("rel8_4byte", [100, 50, 0], [1800, 1950, Z]), ("odd_mixed", [101, 50, 0], [1799, 1950, Z]),
                    ("narrow64px", [512, 0, 0], [64, Y, Z]), ("narrow8px", [512, 0, 0], [8, Y, Z])):
    dst = torch.empty((1, 1, n[2], n[1], n[0]), dtype=torch.int16, device="cuda")
    ms = timed(lambda: lfm.crop_device(src, [X, Y, Z, 1, 1], lb + [0, 0], n + [1, 1], 2, dst))
    view = src[:, :, lb[2]:lb[2] + n[2], lb[1]:lb[1] + n[1], lb[0]:lb[0] + n[0]]
    ok = bool(torch.equal(dst, view))
    ms_t = timed(lambda: dst.copy_(view))
    gb = 2 * dst.numel() * 2 / 1e9
    print(json.dumps({"box": name, "lb": lb, "n": n, "crop_ms": round(ms, 4), "crop_GBps": round(gb / ms * 1e3, 1),
                      "torch_copy_ms": round(ms_t, 4), "torch_GBps": round(gb / ms_t * 1e3, 1), "equal": ok}), flush=True)
