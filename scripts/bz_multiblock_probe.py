#!/usr/bin/env python3
"""GPU bzip2 of multi-block streams against their hand-back to the host
library, on the config-3 stack (2048 x 2048 x 64 uint16, Nnum 15, angle,
auto-selected predictor, built on the device with synth_device) written with
1 MiB blocks: block_size [256, 256, 8, 1, 1], bzip2 level 9, every stream
longer than one bzip2 block.

After 3 warm-up pairs, N >= 10 timed pairs, interleaved so both legs see the
same machine state:
  on:   lfm.set_bzip2_multiblock(True)   the device cuts, compresses and joins
  off:  lfm.set_bzip2_multiblock(False)  the parent's path: libbz2 on the host
Writes one JSON line (also printed): both legs' total_ms lists, medians, min /
max, their stream_counts() and whether every .lfm had the first one's SHA-256.

    python scripts/bz_multiblock_probe.py [--pairs 10] [--frames 64] [--out profiles/bz_multiblock_config3_1MiB.jsonl]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, T, SEED = 2048, 2048, 15, 0x4C464D03
BLOCK = [256, 256, 8, 1, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bz_multiblock_config3_1MiB.jsonl"))
    args = ap.parse_args()
    if args.pairs < 10:
        ap.error("at least 10 timed pairs")
    lfm.require_gpu()
    lfm.set_family("angle")
    d_img = torch.empty((args.frames, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d_img, X, Y, args.frames, T, z0=0, seed=SEED)
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device())
    ms = {True: [], False: []}
    counts, chosen, nbytes, first, same = {}, None, 0, None, True
    was = lfm.get_bzip2_multiblock()
    try:
        for i in range(args.warmup + args.pairs):
            for on in (True, False):
                lfm.set_bzip2_multiblock(on)
                buf, st = enc.encode(d_img, header_version=0, nnum=T, block_size=BLOCK, copy=False)
                digest = hashlib.sha256(buf).hexdigest()
                first = first or digest
                same = same and digest == first
                counts[on], chosen, nbytes = enc.stream_counts(), st["chosen"], len(buf)
                del buf
                if i >= args.warmup:
                    ms[on].append(st["total_ms"])
                print("pair %d %s: %.1f ms" % (i, "on" if on else "off", st["total_ms"]), file=sys.stderr, flush=True)
    finally:
        lfm.set_bzip2_multiblock(was)
        enc.close()
    px = X * Y * args.frames

    def summary(v):
        m = float(np.median(v))
        return {"median_ms": round(m, 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
                "Mpixel_per_s": round(px / m / 1e3, 1), "runs_ms": [round(x, 2) for x in v]}

    line = {"probe": "bz_multiblock_config3_1MiB",
            "workload": "%dx%dx%d uint16, Nnum %d, angle, auto (predictor %d), block %s, level 9, %d .lfm bytes"
                        % (X, Y, args.frames, T, chosen, "x".join(map(str, BLOCK)), nbytes),
            "gpu": torch.cuda.get_device_name(0), "warmup_pairs": args.warmup, "timed_pairs": args.pairs,
            "order": "interleaved: on, off, on, off, ...", "metric": "lfm_encode_stats.total_ms",
            "on": summary(ms[True]), "off": summary(ms[False]),
            "off_over_on": round(float(np.median(ms[False])) / float(np.median(ms[True])), 3),
            "stream_counts_on": counts[True], "stream_counts_off": counts[False],
            "sha256": first, "all_equal": same}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
