#!/usr/bin/env python3
"""A/B timing of the flow kernel's candidate pruning: two builds, three inputs.

Times me_full_search_batch_device (16x16 SAD, +-32) on 16-frame 1080p batches of
  synth    bench.py's batch of the synthetic pair (bench.batch_frames),
  foreman  a 1920x1080 mosaic of Foreman frames 1 and 2 (tests/golden/frames):
           real content,
  noise    independent uniform noise: nothing to prune, the bypass's case,
with the libraries of --libs alternately (every run a fresh child process under
its own timeout; a failed child stops the rest), --rounds rounds.  A library is
a file name in motionestimation_amd/lib (ME_HIP_LIB), e.g. a build of the
parent commit copied there as libme_hip_parent.so.  Per (input, library): the
median and min-max of the per-call time over the rounds, and whether every
library's fields are equal array for array.  A tuning build
(libme_hip_tune.so; ME_PRUNE, ME_PRUNE_BYPASS, ME_PRUNE_SPLIT, ME_FLOW_SLOTS,
ME_FAIR_T pass through from the environment) also reports its live lane-task
fraction, bypassed items and executed wave-tasks by row-split class per call,
and (a build with me_debug_prune_split_hist) those of h = 16 items by the list
entries they held, n = 1 .. 64 (tasks_by_n), and by the rows a lane takes under
the rule ME_PRUNE_SPLIT selects (tasks_by_rows).
usage: python3 tools/sad_prune_ab.py --libs libme_hip_parent.so,libme_hip.so [--rounds 5]
       [--inputs synth,foreman,noise] [--ms 300]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, BLK, SPAN, F = 1920, 1080, 16, 32, 16


def frames_of(name):
    import numpy as np
    import bench
    from motionestimation_amd import synth
    if name == "synth":
        return bench.batch_frames(*synth.named_pair("1080p"), F)
    if name == "foreman":
        d = os.path.join(REPO, "tests", "golden", "frames")
        f1 = np.fromfile(os.path.join(d, "ForemanYF1.yuv"), np.uint8)[:352 * 288].reshape(288, 352)
        f2 = np.fromfile(os.path.join(d, "ForemanYF2.yuv"), np.uint8)[:352 * 288].reshape(288, 352)
        mos = lambda a: np.ascontiguousarray(np.tile(a, (4, 6))[:H, :W])  # noqa: E731
        return bench.batch_frames(mos(f1), mos(f2), F)
    if name == "noise":
        rng = np.random.default_rng(7)
        return [(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8))
                for _ in range(F)]
    raise SystemExit(f"unknown input {name}")


def split_rows(n, rule="1"):
    """Rows of the chunk's 13 a lane takes in a task of n list entries (csrc/me_geom.h
    flow_split_rows; rule "2": flow_split_rows_124, "0": no split)."""
    if rule == "0" or n > 32:
        return 13
    if rule == "2":
        return 4 if n <= 16 else 7
    return 1 if n <= 4 else 2 if n <= 9 else 3 if n <= 12 else 4 if n <= 16 else 7


def tasks_by_rows(by_n, rule="1"):
    out = {}
    for i, c in enumerate(by_n):
        r = str(split_rows(i + 1, rule))
        out[r] = out.get(r, 0) + c
    return out


def child(a):
    import numpy as np
    import torch
    import motionestimation_amd as me
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    eng = me.Engine(devices=[0])
    L = me._lib.lib()
    frames = frames_of(a.child)
    nb = me.num_blocks(W, H, BLK)
    ref_t = torch.from_numpy(np.stack([r for r, _ in frames])).to(dev)
    cur_t = torch.from_numpy(np.stack([c for _, c in frames])).to(dev)
    mv = torch.empty((F * nb, 2), dtype=torch.int16, device=dev)
    co = torch.empty(F * nb, dtype=torch.int32, device=dev)
    run = eng.prepared_batch_search(ref_t, 0, cur_t, 0, W, H, BLK, SPAN, "sad", 0, (H + BLK - 1) // BLK, mv, co)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        for _ in range(4):
            run()
        torch.cuda.synchronize()
    stats = None
    if hasattr(L, "me_debug_prune_stats"):
        L.me_debug_prune_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        out = (ctypes.c_uint32 * 4)()
        L.me_debug_prune_stats(eng._h, out)  # zero the counts
        split = hasattr(L, "me_debug_prune_split_stats")
        out3 = (ctypes.c_uint32 * 3)()
        if split:
            L.me_debug_prune_split_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
            L.me_debug_prune_split_stats(eng._h, out3)
        hist = hasattr(L, "me_debug_prune_split_hist")
        out64 = (ctypes.c_uint32 * 64)()
        if hist:
            L.me_debug_prune_split_hist.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
            L.me_debug_prune_split_hist(eng._h, out64)
        run()
        torch.cuda.synchronize()
        L.me_debug_prune_stats(eng._h, out)
        stats = {"live": out[0], "total": out[1], "bypassed_items": out[2], "items": out[3],
                 "live_frac": out[0] / out[1] if out[1] else None}
        if split:  # executed wave-tasks run whole / with 2 / with 4 or more lanes per list entry
            L.me_debug_prune_split_stats(eng._h, out3)
            stats["tasks_p1_p2_p4"] = list(out3)
        if hist:  # ... of h = 16 items by list entries held, n = 1 .. 64, and by the rows a lane takes
            L.me_debug_prune_split_hist(eng._h, out64)
            stats["tasks_by_n"] = list(out64)
            stats["tasks_by_rows"] = tasks_by_rows(list(out64), os.environ.get("ME_PRUNE_SPLIT", "1"))
    reps = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.ms / 1e3:
        for _ in range(4):
            run()
        reps += 4
        torch.cuda.synchronize()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    eng.device_check()
    sha = hashlib.sha256(mv.cpu().numpy().tobytes() + co.cpu().numpy().tobytes()).hexdigest()
    print("AB " + json.dumps({"input": a.child, "lib": os.path.basename(me._lib.LIB_PATH), "ms_per_call": ms,
                              "calls": reps, "fields_sha256": sha, "prune": stats}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="libme_hip_parent.so,libme_hip.so")
    ap.add_argument("--inputs", default="synth,foreman,noise")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ms", type=float, default=300.0, help="timed wall per run")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    libs = a.libs.split(",")
    runs = {}
    for name in a.inputs.split(","):
        for rnd in range(a.rounds):
            for lib in libs:
                env = dict(os.environ, ME_HIP_LIB=lib)
                r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__),
                                    "--child", name, "--ms", str(a.ms)], capture_output=True, text=True, env=env)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")]
                if r.returncode != 0 or not line:
                    print(json.dumps({"failed": {"input": name, "lib": lib, "round": rnd, "rc": r.returncode,
                                                 "stderr": r.stderr[-1500:]}}), flush=True)
                    return 1  # nothing more runs after a failure
                d = json.loads(line[0][3:])
                print(json.dumps(dict(d, round=rnd)), flush=True)
                runs.setdefault((name, lib), []).append(d)
    ok = True
    for name in a.inputs.split(","):
        shas = {runs[(name, lib)][-1]["fields_sha256"] for lib in libs}
        equal = len(shas) == 1 and all(len({d["fields_sha256"] for d in runs[(name, lib)]}) == 1 for lib in libs)
        ok = ok and equal
        base = statistics.median(d["ms_per_call"] for d in runs[(name, libs[0])])
        for lib in libs:
            t = [d["ms_per_call"] for d in runs[(name, lib)]]
            med = statistics.median(t)
            print(json.dumps({"summary": name, "lib": lib, "median_ms": round(med, 4), "min_ms": round(min(t), 4),
                              "max_ms": round(max(t), 4), "speedup_vs_first": round(base / med, 3),
                              "fields_equal_across_libs": equal, "prune": runs[(name, lib)][-1]["prune"]}),
                  flush=True)
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
