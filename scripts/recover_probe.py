#!/usr/bin/env python3
"""Recovery probe (GPU machine): lfm.recover of an unclosed file of the
config-3 device stack of stream_probe.py (2048 x 2048 x 64 uint16, Nnum 15,
angle, auto-selected predictor).

The stack is appended in 8 one-layer appends to a lfm.Writer opened for 72
frames, flushed, and the still-open file copied (what a killed process leaves);
the copy is recovered into a second file with verify=True (every stream through
the GPU bzip2 decoder) and with verify=False, 1 warm-up and 5 timed rounds each,
and the result hashed against Encoder.encode of the stack.

One JSON line:
    python scripts/recover_probe.py >> profiles/stream_writer_checkpoint_config3.jsonl"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, Z, T, SEED, CAPACITY = 2048, 2048, 64, 15, 0x4C464D03, 72


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the probe's files go (default: the temporary directory)")
    args = ap.parse_args()
    lfm.require_gpu()
    lfm.set_family("angle")
    d_img = torch.empty((Z, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d_img, X, Y, Z, T, z0=0, seed=SEED)
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device())
    buf, _ = enc.encode(d_img, header_version=0, nnum=T)
    want = hashlib.sha256(buf).hexdigest()
    size = len(buf)
    del buf
    enc.close()
    ms = {True: [], False: []}
    same, st = True, {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        live, crash, out = (os.path.join(d, n) for n in ("open.lfm", "crash.lfm", "out.lfm"))
        w = lfm.Writer(live, (CAPACITY, Y, X), predictor_request=0, nnum=T)
        for z in range(0, Z, 8):
            w.append(d_img[z:z + 8])
        t0 = time.perf_counter()
        committed = w.flush()
        flush_ms = (time.perf_counter() - t0) * 1e3
        shutil.copyfile(live, crash)
        w.abort()
        for i in range(1 + args.rounds):
            for verify in (True, False):
                t0 = time.perf_counter()
                s = lfm.recover(crash, out=out, verify=verify)
                t1 = time.perf_counter()
                same = same and sha(out) == want
                os.remove(out)
                if i:
                    ms[verify].append((t1 - t0) * 1e3)
                    st[verify] = s
    lfm.set_family("tiles")

    def summary(v):
        return {"median_ms": round(float(np.median(v)), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
                "runs_ms": [round(x, 2) for x in v]}

    print(json.dumps({"probe": "stream_recover_config3",
                      "workload": "%dx%dx%d uint16 device stack in a writer of capacity %d, Nnum %d, angle, auto, "
                                  "default blocks, %d .lfm bytes; recovered into a second file"
                                  % (X, Y, Z, CAPACITY, T, size),
                      "gpu": torch.cuda.get_device_name(0), "warmup_rounds": 1, "timed_rounds": args.rounds,
                      "committed": committed, "flush_ms": round(flush_ms, 2),
                      "note": "the file was just written: recovery reads it from the page cache",
                      "verify": summary(ms[True]), "no_verify": summary(ms[False]),
                      "verify_stats": st[True], "no_verify_stats": st[False], "sha256": want,
                      "files_identical": same}), flush=True)
    sys.exit(0 if same and committed == Z else 1)


if __name__ == "__main__":
    main()
