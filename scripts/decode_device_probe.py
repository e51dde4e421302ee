#!/usr/bin/env python3
"""Host- against device-destination decode of the config-3 file (2048 x 2048 x
64 uint16, Nnum 15, angle, auto-selected predictor; built on the device with
synth_device + Encoder as bench.py --full does).

After 3 warm-up pairs, N timed pairs, interleaved so both readers see the same
machine state:
  host:   lfm.decode(buf) into a fresh host array (the reader bench.py times)
  device: lfm.decode_device(buf, out=preallocated) + torch.cuda.synchronize()
Prints one JSON line: both run lists, medians, min / max, the lfm_decode_stats
of the last device call and whether every result was exact.

    python scripts/decode_device_probe.py [--pairs 12] [--frames 64] > profiles/decode_device_config3.jsonl
LFM_DECODE_TIMING=1 adds the two pipelines' timelines on stderr."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, T, SEED = 2048, 2048, 15, 0x4C464D03


def threads():
    v = os.environ.get("LFM_NUM_THREADS")
    if v and v.isdigit() and int(v) > 0:
        return int(v)
    n = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    if args.pairs < 10:
        ap.error("at least 10 timed pairs")
    lfm.require_gpu()
    lfm.set_family("angle")
    nt = threads()
    d_img = torch.empty((args.frames, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d_img, X, Y, args.frames, T, z0=0, seed=SEED)
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device(), num_threads=nt)
    buf, est = enc.encode(d_img, header_version=0, nnum=T)
    enc.close()  # a reader's process holds no encoder
    ref = d_img.cpu().numpy().view(np.uint16)
    out = torch.empty((1, 1, args.frames, Y, X), dtype=torch.int16, device="cuda")
    host_ms, dev_ms, exact, st = [], [], True, None
    for i in range(args.warmup + args.pairs):
        t0 = time.perf_counter()
        img = lfm.decode(buf, num_threads=nt)
        t1 = time.perf_counter()
        exact = exact and bool(np.array_equal(img.reshape(ref.shape), ref))
        del img
        out.fill_(0x5555)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        _, st = lfm.decode_device(buf, out=out, num_threads=nt, return_stats=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        exact = exact and bool(torch.equal(out.view(d_img.shape), d_img))
        if i >= args.warmup:
            host_ms.append((t1 - t0) * 1e3)
            dev_ms.append((t3 - t2) * 1e3)
    px = X * Y * args.frames

    def summary(v):
        m = float(np.median(v))
        return {"median_ms": round(m, 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
                "Mpixel_per_s": round(px / m / 1e3, 1), "runs_ms": [round(x, 2) for x in v]}

    line = {"probe": "decode_device_config3",
            "workload": "%dx%dx%d uint16, Nnum %d, angle, auto (predictor %d), %d .lfm bytes"
                        % (X, Y, args.frames, T, est["chosen"], len(buf)),
            "gpu": torch.cuda.get_device_name(0), "threads": nt, "warmup_pairs": args.warmup,
            "timed_pairs": args.pairs, "order": "interleaved: host, device, host, device, ...",
            "host": summary(host_ms), "device": summary(dev_ms),
            "device_over_host": round(float(np.median(dev_ms)) / float(np.median(host_ms)), 3),
            "device_stats": st, "d2h_bytes": st["d2h_bytes"], "exact": exact}
    print(json.dumps(line), flush=True)
    if not exact or st["d2h_bytes"] != 0 or st["path"] != 0:
        sys.exit(1)


if __name__ == "__main__":
    main()
