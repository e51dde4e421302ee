#!/usr/bin/env python3
"""GPU decode of multi-block streams against their decode by the host library,
on the config-3 stack (2048 x 2048 x 64 uint16, Nnum 15, angle, auto-selected
predictor, built on the device with synth_device) written with 1 MiB blocks:
block_size [256, 256, 8, 1, 1], bzip2 level 9, 512 streams of two bzip2 blocks.
The .lfm is encoded once (on the GPU) and decoded into a device tensor
(lfm.decode_device):
  on:   lfm.set_bunzip2_multiblock(True)   every stream decoded on the device
  off:  lfm.set_bunzip2_multiblock(False)  the parent's path: every stream
        flagged on the device and decoded by libbz2 on the calling thread
After the warm-up legs (--warmup on-legs and one off-leg), --pairs on-legs are
timed; an off-leg takes tens of seconds, so only --off-legs of them are timed,
spread evenly between the on-legs (--off-legs = --pairs: interleaved pairs).
Every decoded image is compared with the input on the device; the first of
each leg is also hashed.  Writes one JSON line (also printed, appended to
--out): both legs' total_ms lists, medians, min / max, host_blocks, digests.

    python scripts/bunzip2_multiblock_probe.py [--pairs 10] [--off-legs 3] [--out profiles/bunzip2_multiblock_config3_1MiB.jsonl]

--off-legs 0 --out "" decodes with the switch on only and writes no file (the
run a kernel trace is taken of).
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
    ap.add_argument("--pairs", type=int, default=10, help="timed on-legs")
    ap.add_argument("--off-legs", type=int, default=3, help="timed off-legs (<= pairs)")
    ap.add_argument("--warmup", type=int, default=2, help="on-legs before the timed ones")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bunzip2_multiblock_config3_1MiB.jsonl"))
    args = ap.parse_args()
    if args.pairs < 1 or not 0 <= args.off_legs <= args.pairs:
        ap.error("1 <= pairs, 0 <= off-legs <= pairs")
    lfm.require_gpu()
    lfm.set_family("angle")
    d_img = torch.empty((args.frames, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d_img, X, Y, args.frames, T, z0=0, seed=SEED)
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device())
    try:
        buf, est = enc.encode(d_img, header_version=0, nnum=T, block_size=BLOCK)
        counts = enc.stream_counts()
    finally:
        enc.close()
    want = hashlib.sha256(d_img.cpu().numpy().tobytes()).hexdigest()
    d_out = torch.empty((1, 1, args.frames, Y, X), dtype=torch.int16, device="cuda")  # (int16 stands in for uint16)
    ms, host_blocks, blocks, digest, exact = {True: [], False: []}, {}, {}, {}, True

    def leg(on, timed):
        nonlocal exact
        lfm.set_bunzip2_multiblock(on)
        d_out.zero_()
        torch.cuda.synchronize()
        _, st = lfm.decode_device(buf, out=d_out, return_stats=True)
        same = bool(torch.equal(d_out.reshape(d_img.shape), d_img))
        exact = exact and same
        if on not in digest:
            digest[on] = hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()
        host_blocks[on], blocks[on] = st["host_blocks"], st["blocks"]
        if timed:
            ms[on].append(st["total_ms"])
        print("%s %s: %.1f ms, host_blocks %d, exact %s" % ("timed" if timed else "warm-up", "on" if on else "off",
                                                            st["total_ms"], st["host_blocks"], same),
              file=sys.stderr, flush=True)

    # timed on-leg i is followed by an off-leg when i is one of off_legs evenly spread indices
    off_after = {int(round((j + 1) * args.pairs / args.off_legs)) - 1 for j in range(args.off_legs)}
    was = lfm.get_bunzip2_multiblock()
    try:
        for _ in range(args.warmup):
            leg(True, False)
        if args.off_legs:
            leg(False, False)
        for i in range(args.pairs):
            leg(True, True)
            if i in off_after:
                leg(False, True)
    finally:
        lfm.set_bunzip2_multiblock(was)
    px = X * Y * args.frames

    def summary(v):
        if not v:
            return None
        m = float(np.median(v))
        return {"median_ms": round(m, 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
                "Mpixel_per_s": round(px / m / 1e3, 1), "runs_ms": [round(x, 2) for x in v]}

    line = {"probe": "bunzip2_multiblock_config3_1MiB",
            "workload": "%dx%dx%d uint16, Nnum %d, angle, auto (predictor %d), block %s, level 9, %d .lfm bytes, "
                        "%d streams of %d bzip2 blocks in all"
                        % (X, Y, args.frames, T, est["chosen"], "x".join(map(str, BLOCK)), len(buf), counts["streams"],
                           counts["bzip2_blocks"]),
            "gpu": torch.cuda.get_device_name(0), "warmup_on_legs": args.warmup, "timed_on_legs": args.pairs,
            "timed_off_legs": args.off_legs,
            "order": "an off-leg after on-legs %s" % sorted(off_after), "metric": "lfm_decode_stats.total_ms "
            "(lfm_decode_memory_device into a device tensor)",
            "on": summary(ms[True]), "off": summary(ms[False]),
            "off_over_on": round(float(np.median(ms[False])) / float(np.median(ms[True])), 2) if ms[False] else None,
            "blocks": blocks.get(True), "host_blocks_on": host_blocks.get(True), "host_blocks_off": host_blocks.get(False),
            "sha256_input": want, "sha256_on": digest.get(True), "sha256_off": digest.get(False), "all_exact": exact}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if not exact or any(d != want for d in digest.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
