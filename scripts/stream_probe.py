#!/usr/bin/env python3
"""Streaming probe (GPU machine): lfm.Writer against the one-shot encoder, and
lfm.Reader against reading the whole file.

writer -- the config-3 device stack (2048 x 2048 x 64 uint16, Nnum 15, angle,
auto-selected predictor; lfm.synth_device) written three ways (and one more for reference) in one process:
  per_layer: lfm.Writer, 8 appends of 8 frames (one block layer each)
  one_append: lfm.Writer, one append of 64 frames
  one_shot:  Encoder.encode of the stack to memory, then the bytes written to
             a file (the path this change does not touch: the yardstick)
  one_shot_cold: the same on an Encoder made for the round, as each Writer
             makes its own (not one of the three compared: it separates the
             encoder's first-use cost from the streaming)
interleaved, 10 timed rounds after 2 warm-ups; every file is hashed against
the one-shot bytes.  All three write to the same directory (--dir, default the
system's temporary directory), so the file system is the same for all.

reader -- a 4-volume config-5-shaped file (4096 x 4096 x 32 x 1 x 4, video,
tiles, Nnum 13, auto), itself written with lfm.Writer one volume at a time:
  ranged: lfm.Reader.read of the last t-volume into a device tensor
  whole:  lfm.read_lfm_device of the whole file, then a slice
interleaved, 10 timed rounds after 2 warm-ups, with bytes_read against
file_bytes.

One JSON line per part:
    python scripts/stream_probe.py > profiles/stream_writer_config3.jsonl"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

import torch  # noqa: E402  (before liblfm: one HIP runtime)
import lfm  # noqa: E402

X, Y, Z, T, SEED = 2048, 2048, 64, 15, 0x4C464D03
X5, Y5, Z5, T5, SEED5, NVOL = 4096, 4096, 32, 13, 0x4C464D05, 4


def threads():
    v = os.environ.get("LFM_NUM_THREADS")
    if v and v.isdigit() and int(v) > 0:
        return int(v)
    n = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def summary(v, px=None):
    m = float(np.median(v))
    out = {"median_ms": round(m, 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
           "runs_ms": [round(x, 2) for x in v]}
    if px:
        out["Mpixel_per_s"] = round(px / m / 1e3, 1)
    return out


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def writer_part(args, nt, d):
    lfm.set_family("angle")
    d_img = torch.empty((Z, Y, X), dtype=torch.int16, device="cuda")
    lfm.synth_device(d_img, X, Y, Z, T, z0=0, seed=SEED)
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device(), num_threads=nt)
    paths = {k: os.path.join(d, "probe_%s.lfm" % k) for k in ("per_layer", "one_append", "one_shot", "one_shot_cold")}
    ms = {k: [] for k in paths}
    same, want, stats, calls = True, None, {}, {}
    for i in range(args.warmup + args.rounds):
        for k in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "one_shot":
                buf, _ = enc.encode(d_img, header_version=0, nnum=T, copy=False)
                with open(paths[k], "wb") as f:
                    f.write(buf)
            elif k == "one_shot_cold":
                # a writer owns a new encoder; so does this one-shot, to tell the
                # encoder's first-use cost (buffers, streams) from the streaming itself
                cold = lfm.Encoder(device=torch.cuda.current_device(), num_threads=nt)
                buf, _ = cold.encode(d_img, header_version=0, nnum=T, copy=False)
                with open(paths[k], "wb") as f:
                    f.write(buf)
                del buf
                cold.close()
            else:
                step = 8 if k == "per_layer" else Z
                each = []
                with lfm.Writer(paths[k], (Z, Y, X), predictor_request=0, nnum=T, num_threads=nt) as w:
                    for z in range(0, Z, step):
                        ta = time.perf_counter()
                        w.append(d_img[z:z + step])
                        each.append(round((time.perf_counter() - ta) * 1e3, 2))
                    ta = time.perf_counter()
                    w.close()
                    calls[k] = {"append_ms": each, "close_ms": round((time.perf_counter() - ta) * 1e3, 2)}
                stats[k] = w.stats
            t1 = time.perf_counter()
            if i >= args.warmup:
                ms[k].append((t1 - t0) * 1e3)
        digests = {k: sha(p) for k, p in paths.items()}
        want = want or digests["one_shot"]
        same = same and all(v == want for v in digests.values())
    enc.close()
    size = os.path.getsize(paths["one_shot"])
    for p in paths.values():
        os.remove(p)
    px = X * Y * Z
    line = {"probe": "stream_writer_config3",
            "workload": "%dx%dx%d uint16 device stack, Nnum %d, angle, auto, default blocks, %d .lfm bytes"
                        % (X, Y, Z, T, size),
            "gpu": torch.cuda.get_device_name(0), "threads": nt, "warmup_rounds": args.warmup,
            "timed_rounds": args.rounds, "order": "interleaved: per_layer, one_append, one_shot, one_shot_cold, ...",
            "timed": "open .. close of the file, the encode included; the page cache takes the bytes (no fsync)",
            "per_layer": summary(ms["per_layer"], px), "one_append": summary(ms["one_append"], px),
            "one_shot": summary(ms["one_shot"], px), "one_shot_cold": summary(ms["one_shot_cold"], px),
            "last_round_calls": calls,
            "per_layer_over_one_shot": round(float(np.median(ms["per_layer"]) / np.median(ms["one_shot"])), 3),
            "one_append_over_one_shot": round(float(np.median(ms["one_append"]) / np.median(ms["one_shot"])), 3),
            "writer_stats": stats, "sha256": want, "files_identical": same}
    print(json.dumps(line), flush=True)
    del d_img
    return same


def reader_part(args, nt, d):
    lfm.set_family("tiles")
    path = os.path.join(d, "probe_cfg5x%d.lfm" % NVOL)
    vol = torch.empty((1, Z5, Y5, X5), dtype=torch.int16, device="cuda")
    t0 = time.perf_counter()
    with lfm.Writer(path, (NVOL, 1, Z5, Y5, X5), predictor_request=0, video=1, nnum=T5, num_threads=nt) as w:
        for t in range(NVOL):
            lfm.synth_device(vol, X5, Y5, Z5, T5, t_index=t, idx0=t * Z5 * X5 * Y5, seed=SEED5)
            w.append(vol)  # (reads vol before it returns: the next synth may overwrite it)
    write_ms = (time.perf_counter() - t0) * 1e3
    last = vol.clone()  # volume NVOL - 1, the expected pixels
    del vol
    lb, ub = [0, 0, 0, 0, NVOL - 1], [X5 - 1, Y5 - 1, Z5 - 1, 0, NVOL - 1]
    out = torch.empty((1, 1, Z5, Y5, X5), dtype=torch.int16, device="cuda")
    ranged, whole, exact = [], [], True
    fetched = st = None
    for i in range(args.warmup + args.rounds):
        out.fill_(0x5555)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with lfm.Reader(path) as r:
            _, st = r.read(lb, ub, out=out, num_threads=nt, return_stats=True)
            fetched, file_bytes = r.bytes_read, r.file_bytes
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        exact = exact and bool(torch.equal(out.view(last.shape), last))
        t2 = time.perf_counter()
        full = lfm.read_lfm_device(path, num_threads=nt)
        piece = full[NVOL - 1:NVOL]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        exact = exact and bool(torch.equal(piece.view(torch.int16).reshape(last.shape), last))
        del full, piece
        if i >= args.warmup:
            ranged.append((t1 - t0) * 1e3)
            whole.append((t3 - t2) * 1e3)
    os.remove(path)
    line = {"probe": "stream_reader_config5x%d" % NVOL,
            "workload": "%dx%dx%dx1x%d uint16, video, tiles, Nnum %d, auto (predictor %d); last t-volume to a "
                        "device tensor" % (X5, Y5, Z5, NVOL, T5, w.stats["chosen"]),
            "gpu": torch.cuda.get_device_name(0), "threads": nt, "warmup_rounds": args.warmup,
            "timed_rounds": args.rounds, "order": "interleaved: ranged, whole, ...",
            "note": "the file was just written: both readers read it from the page cache",
            "file_bytes": file_bytes, "bytes_read": fetched, "bytes_read_fraction": round(fetched / file_bytes, 4),
            "ranged": summary(ranged), "whole_then_slice": summary(whole),
            "ranged_over_whole": round(float(np.median(ranged) / np.median(whole)), 3),
            "ranged_stats": st, "writer_ms": round(write_ms, 1), "writer_stats": w.stats, "exact": exact}
    print(json.dumps(line), flush=True)
    return exact and st["d2h_bytes"] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the probe's files go (default: the temporary directory)")
    ap.add_argument("--only", choices=("writer", "reader"), default=None)
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("at least 10 timed rounds")
    lfm.require_gpu()
    nt = threads()
    ok = True
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        if args.only != "reader":
            ok = writer_part(args, nt, d) and ok
        if args.only != "writer":
            ok = reader_part(args, nt, d) and ok
    lfm.set_family("tiles")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
