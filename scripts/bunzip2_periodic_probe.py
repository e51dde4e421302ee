#!/usr/bin/env python3
"""GPU decode of periodic bzip2 blocks against their decode by the host
library, on a config-3-sized unpredicted stack (2048 x 2048 x 64 uint16,
default 96 x 96 x 8 blocks, bzip2 level 2, 3 872 streams, predictor 0 forced):
  half:   every other block constant 0x0201 (bytes 01 02 01 02 ...: a text of
          period 2, the kind lfm.set_bunzip2_periodic is about), the rest noise
  noise:  the same noise everywhere: no periodic stream, every block takes the
          single-cycle path of bzd_walk whatever the switch says
Each .lfm is encoded once (on the GPU; the encoder hands periodic streams to
the host library, which takes a while) and decoded into a device tensor
(lfm.decode_device):
  off:  lfm.set_bunzip2_periodic(False)  the parent's path: periodic streams
        flagged on the device and decoded by libbz2 on the calling thread
  on:   lfm.set_bunzip2_periodic(True)   every stream decoded on the device
After one warm-up pair, --pairs interleaved (off, on) pairs are timed per
stack.  Every decoded image is compared with the input on the device.  Writes
one JSON line per stack (also printed, appended to --out): both legs' total_ms
lists, medians, min / max (the spread), host_blocks.

    python scripts/bunzip2_periodic_probe.py [--pairs 10] [--out profiles/bunzip2_periodic_config3.jsonl]

--fill N times the bare decoder instead (lfm_hip_bunzip2_blocks, switch on) on
N copies of one periodic stream (the 0x0201 block at level 2, and 880 000 bytes
of period 2 at level 9): the figure the fill of bzd_walk is judged by.  Run it
with LFM_LIB naming a library built with -DLFM_BZD_FILL_BYTES=1
(scripts/build_variant.sh) for the byte-store form; "library" in the line says
which one ran.
"""
import argparse
import bz2
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, T = 2048, 2048, 15
BLOCK = [96, 96, 8]


def summary(v, px=None):
    m = float(np.median(v))
    d = {"median_ms": round(m, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
         "runs_ms": [round(x, 3) for x in v]}
    if px:
        d["Mpixel_per_s"] = round(px / m / 1e3, 1)
    return d


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def stacks(frames):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x4C464D03)
    noise = torch.randint(0, 65536, (frames, Y, X), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    ax = [torch.arange(n, device="cuda") // b for n, b in ((frames, BLOCK[2]), (Y, BLOCK[1]), (X, BLOCK[0]))]
    const = (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]) % 2 == 0
    half = torch.where(const, torch.tensor(0x0201, dtype=torch.int16, device="cuda"), noise)
    return {"half": half, "noise": noise}


def engine(args):
    was = lfm.get_bunzip2_periodic()
    ok = True
    for name, d_img in stacks(args.frames).items():
        enc = lfm.Encoder(device=torch.cuda.current_device())
        try:
            buf, _ = enc.encode(d_img, header_version=8, nnum=T)  # request 8: predictor 0 forced
            counts = enc.stream_counts()
        finally:
            enc.close()
        d_out = torch.empty((1, 1) + tuple(d_img.shape), dtype=torch.int16, device="cuda")  # (int16 stands in for uint16)
        ms, host_blocks, blocks, exact = {True: [], False: []}, {}, {}, True

        def leg(on, timed):
            nonlocal exact
            lfm.set_bunzip2_periodic(on)
            d_out.zero_()
            torch.cuda.synchronize()
            _, st = lfm.decode_device(buf, out=d_out, return_stats=True)
            same = bool(torch.equal(d_out.reshape(d_img.shape), d_img))
            exact = exact and same
            host_blocks.setdefault(on, set()).add(st["host_blocks"])
            blocks[on] = st["blocks"]
            if timed:
                ms[on].append(st["total_ms"])
            print("%s %s %s: %.2f ms, host_blocks %d, exact %s" % (name, "timed" if timed else "warm-up",
                                                                  "on" if on else "off", st["total_ms"],
                                                                  st["host_blocks"], same), file=sys.stderr, flush=True)

        try:
            for i in range(args.pairs + 1):
                leg(False, i > 0)
                leg(True, i > 0)
        finally:
            lfm.set_bunzip2_periodic(was)
        px = X * Y * args.frames
        off, on = summary(ms[False], px), summary(ms[True], px)
        emit({"probe": "bunzip2_periodic_config3", "stack": name,
              "workload": "%dx%dx%d uint16, unpredicted (predictor 0), block %s, level 2, %d .lfm bytes, %d streams, "
                          "%d of them compressed by the host library (periodic)"
                          % (X, Y, args.frames, "x".join(map(str, BLOCK)), len(buf), counts["streams"],
                             counts["host_streams"]),
              "gpu": torch.cuda.get_device_name(0), "warmup_pairs": 1, "timed_pairs": args.pairs,
              "order": "off, on, off, on, ...",
              "metric": "lfm_decode_stats.total_ms (lfm_decode_memory_device into a device tensor)",
              "off": off, "on": on, "off_over_on": round(off["median_ms"] / on["median_ms"], 3),
              "on_minus_off_median_ms": round(on["median_ms"] - off["median_ms"], 3),
              "off_spread_ms": round(off["max_ms"] - off["min_ms"], 3),
              "blocks": blocks[True], "host_blocks_off": sorted(host_blocks[False]),
              "host_blocks_on": sorted(host_blocks[True]), "all_exact": exact}, args.out)
        ok = ok and exact
        del d_out
    return ok


def fill(args):
    L = lfm.lib()
    was = lfm.get_bunzip2_periodic()
    ok = True
    for nbytes, level, count in ((2 * 96 * 96 * 8, 2, args.fill), (880000, 9, max(1, args.fill // 8))):
        data = bytes([1, 2]) * (nbytes // 2)
        stream = bz2.compress(data, level)
        offs = (ctypes.c_uint64 * (count + 1))(*[i * len(stream) for i in range(count + 1)])
        pay = torch.frombuffer(bytearray(stream * count + bytes(64)), dtype=torch.uint8).cuda()
        ws_bytes = L.lfm_hip_bunzip2_workspace_bytes(count, nbytes)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out = torch.zeros(count * nbytes, dtype=torch.uint8, device="cuda")
        lens, flags = (ctypes.c_uint32 * count)(), (ctypes.c_uint32 * count)()
        want = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        ms = []
        lfm.set_bunzip2_periodic(True)
        try:
            for i in range(args.pairs + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = L.lfm_hip_bunzip2_blocks(pay.data_ptr(), offs, count, out.data_ptr(), nbytes, ws.data_ptr(),
                                              ws_bytes, lens, flags, None)
                dt = (time.perf_counter() - t0) * 1e3
                if rc != 0 or any(flags) or any(n != nbytes for n in lens):
                    raise SystemExit("decode failed: rc %d flags %s" % (rc, sorted(set(flags))))
                if i >= 2:
                    ms.append(dt)
        finally:
            lfm.set_bunzip2_periodic(was)
        exact = bool((out.view(count, nbytes) == want).all())
        ok = ok and exact
        emit({"probe": "bunzip2_periodic_fill", "library": os.path.relpath(lfm.LIB_PATH, REPO),
              "workload": "%d copies of one stream: %d bytes of period 2, level %d" % (count, nbytes, level),
              "gpu": torch.cuda.get_device_name(0), "metric": "wall ms of lfm_hip_bunzip2_blocks (synchronous)",
              "warmup": 2, "decode": summary(ms), "exact": exact}, args.out)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10, help="timed (off, on) pairs per stack; timed calls with --fill")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fill", type=int, default=0, help="time the bare decoder on this many periodic streams instead")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bunzip2_periodic_config3.jsonl"))
    args = ap.parse_args()
    if args.pairs < 1 or args.frames % BLOCK[2]:
        ap.error("1 <= pairs, frames a multiple of %d" % BLOCK[2])
    lfm.require_gpu()
    sys.exit(0 if (fill(args) if args.fill else engine(args)) else 1)


if __name__ == "__main__":
    main()
