#!/usr/bin/env python3
"""Single-device decode against the multi-GPU reader (lfm.decode_multi) on the
config-3 file (2048 x 2048 x 64 uint16, Nnum 15, angle, auto) and on one
config-5 volume (4096 x 4096 x 32 uint16, video, Nnum 13, tiles, auto), both
built on the device with synth_device + Encoder as bench.py --full does.

Per workload, after 3 warm-up rounds, N timed rounds; a round decodes once with
every device list in turn, so all lists see the same machine state:
  single:    no list (lfm_decode_memory_multi is then the plain reader)
  [0, 0]:    two workers on device 0 -- a rehearsal of the path, not a gain
  2 / 4 / 8 distinct devices, where the box has them
Prints one JSON line per workload: run lists, medians, min / max, the
lfm_decode_multi_stats of the last call per list, and whether every result
was exact.

With --parent-lib PATH (a liblfm.so built from the parent commit) it first
checks the untouched path: config 3 through lfm.decode (lfm_decode_memory, no
list) with that library and with this tree's, in alternating fresh child
processes (LFM_LIB), 4 each with 3 warm-up and 3 timed decodes: 12 timed
decodes per library.  The line says whether this tree's median lies inside the
parent's own min .. max.

    python scripts/decode_multi_probe.py [--rounds 12] [--parent-lib PATH] > profiles/decode_multi_config3.jsonl
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd"))

WORKLOADS = {
    "config3": dict(X=2048, Y=2048, Z=64, T=15, seed=0x4C464D03, family="angle", header_version=0),
    "config5_volume": dict(X=4096, Y=4096, Z=32, T=13, seed=0x4C464D05, family="tiles", header_version=0x80),
}


def threads():
    v = os.environ.get("LFM_NUM_THREADS")
    if v and v.isdigit() and int(v) > 0:
        return int(v)
    n = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def summary(v, px):
    m = float(np.median(v))
    return {"median_ms": round(m, 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
            "Mpixel_per_s": round(px / m / 1e3, 1), "runs_ms": [round(x, 2) for x in v]}


def build(name):
    """(.lfm bytes, the stack as numpy [z, y, x], chosen predictor) of a workload."""
    import torch
    import lfm
    w = WORKLOADS[name]
    lfm.require_gpu()
    lfm.set_family(w["family"])
    d = torch.empty((w["Z"], w["Y"], w["X"]), dtype=torch.int16, device="cuda")
    lfm.synth_device(d, w["X"], w["Y"], w["Z"], w["T"], z0=0, seed=w["seed"])
    torch.cuda.synchronize()
    enc = lfm.Encoder(device=torch.cuda.current_device(), num_threads=threads())
    buf, est = enc.encode(d, header_version=w["header_version"], nnum=w["T"])
    enc.close()  # a reader's process holds no encoder
    lfm.release_encoders()
    ref = d.cpu().numpy().view(np.uint16)
    del d
    torch.cuda.empty_cache()
    return buf, ref, est["chosen"]


def gain(name, rounds, warmup):
    import torch
    import lfm
    buf, ref, chosen = build(name)
    nt = threads()
    ndev = torch.cuda.device_count()
    lists = [("single", []), ("workers_0_0", [0, 0])]
    lists += [("devices_%d" % n, list(range(n))) for n in (2, 4, 8) if ndev >= n]
    runs = {key: [] for key, _ in lists}
    stats, exact = {}, True
    for i in range(warmup + rounds):
        for key, devs in lists:
            lfm.set_decode_devices(devs)
            t0 = time.perf_counter()
            img, st = lfm.decode_multi(buf, num_threads=nt, return_stats=True)
            t1 = time.perf_counter()
            exact = exact and bool(np.array_equal(img.reshape(ref.shape), ref))
            del img
            st.pop("shards")
            stats[key] = st
            if i >= warmup:
                runs[key].append((t1 - t0) * 1e3)
    lfm.set_decode_devices(None)
    lfm.release_decoders()
    w = WORKLOADS[name]
    px = w["X"] * w["Y"] * w["Z"]
    single = float(np.median(runs["single"]))
    line = {"probe": "decode_multi_" + name,
            "workload": "%dx%dx%d uint16, Nnum %d, %s, header request 0x%02x (predictor %d), %d .lfm bytes"
                        % (w["X"], w["Y"], w["Z"], w["T"], w["family"], w["header_version"], chosen, len(buf)),
            "gpu": torch.cuda.get_device_name(0), "distinct_devices": ndev, "threads": nt, "warmup_rounds": warmup,
            "timed_rounds": rounds, "order": "interleaved: " + ", ".join(k for k, _ in lists) + ", ...",
            "rehearsal_only": ndev < 2, "exact": exact}
    for key, _ in lists:
        line[key] = dict(summary(runs[key], px), stats=stats[key],
                         over_single=round(float(np.median(runs[key])) / single, 3))
    print(json.dumps(line), flush=True)
    return exact


def child_build(path):
    buf, ref, _ = build("config3")
    with open(path, "wb") as f:
        f.write(buf)
    ref.tofile(path + ".raw")


def child_decode(path, runs, warmup):
    import lfm
    buf = open(path, "rb").read()
    ref = np.fromfile(path + ".raw", dtype=np.uint16)
    lfm.set_family(WORKLOADS["config3"]["family"])
    nt, ms, exact = threads(), [], True
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        img = lfm.decode(buf, num_threads=nt)
        t1 = time.perf_counter()
        exact = exact and bool(np.array_equal(img.reshape(-1), ref))
        del img
        if i >= warmup:
            ms.append((t1 - t0) * 1e3)
    print(json.dumps({"runs_ms": ms, "exact": exact}), flush=True)


def untouched(parent_lib):
    """lfm.decode of config 3 with no device list: the parent's library against this tree's."""
    here = os.path.join(REPO, "lightfieldmicroscopy_pc-bzip2_amd", "liblfm.so")
    runs = {"parent": [], "this": []}
    exact = True
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "config3.lfm")
        env = dict(os.environ)
        env.pop("LFM_DECODE_GPUS", None)
        subprocess.run([sys.executable, __file__, "--child-build", path], check=True, env=dict(env, LFM_LIB=here),
                       timeout=300)
        for _ in range(4):
            for key, lib in (("parent", parent_lib), ("this", here)):
                r = subprocess.run([sys.executable, __file__, "--child-decode", path], check=True, text=True,
                                   env=dict(env, LFM_LIB=lib), capture_output=True, timeout=300)
                got = json.loads(r.stdout.strip().splitlines()[-1])
                runs[key] += got["runs_ms"]
                exact = exact and got["exact"]
    w = WORKLOADS["config3"]
    px = w["X"] * w["Y"] * w["Z"]
    p, t = summary(runs["parent"], px), summary(runs["this"], px)
    inside = p["min_ms"] <= t["median_ms"] <= p["max_ms"]
    print(json.dumps({"probe": "decode_untouched_path_config3",
                      "what": "lfm.decode (lfm_decode_memory), no decode device list; 4 fresh child processes per "
                              "library, alternating parent / this tree, 3 warm-up + 3 timed decodes each",
                      "threads": threads(), "parent": p, "this": t,
                      "this_median_inside_parent_min_max": inside,
                      "this_median_not_above_parent_max": t["median_ms"] <= p["max_ms"], "exact": exact}), flush=True)
    return exact and inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", help="liblfm.so of the parent commit: also compare the untouched path")
    ap.add_argument("--no-gain", action="store_true", help="only the --parent-lib comparison")
    ap.add_argument("--child-build", help=argparse.SUPPRESS)
    ap.add_argument("--child-decode", help=argparse.SUPPRESS)
    ap.add_argument("--gain-child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gain_child:
        sys.exit(0 if gain(args.gain_child, args.rounds, args.warmup) else 1)
    if args.child_build:
        return child_build(args.child_build)
    if args.child_decode:
        return child_decode(args.child_decode, 3, 3)
    if args.rounds < 10:
        ap.error("at least 10 timed rounds")
    ok = True
    if args.parent_lib:
        ok = untouched(os.path.abspath(args.parent_lib)) and ok
    if not args.no_gain:
        # one child process per workload: each starts from a fresh device
        for name in WORKLOADS:
            r = subprocess.run([sys.executable, __file__, "--gain-child", name, "--rounds", str(args.rounds),
                                "--warmup", str(args.warmup)], timeout=900)
            ok = ok and r.returncode == 0
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
