#!/usr/bin/env python3
"""Time the partition search next to the two searches it replaces: 16 resident
1080p synthetic frames (bench.py's step: 16x16 blocks, +-32, SAD),
  (a) me_full_search_batch_device at B = 16,
  (b) the same at B = 8,
  (c) me_partition_search_device at lambda = 16,
each a step of its own.  HIP events around each step after a clock ramp, the
three arms alternating, the median over the steps.  (a) + (b) is what a caller
runs today for the 16x16 and 8x8 fields alone; (c) also yields the 16x8 and
8x16 fields and the mode, from half their abs-diffs.  Prints one JSON line and
fails unless frame 0's records equal tests/partition_ref.py's (about a minute
of numpy at 1080p; --no-check skips it).
usage: python3 tools/partition_time.py [--steps 40] [--frames 16] [--config 1080p] [--lam 16]
       [--no-check]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import motionestimation_amd as me  # noqa: E402
from motionestimation_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lam", type=int, default=16)
    ap.add_argument("--ramp-ms", type=float, default=300.0)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the numpy check of frame 0 (minutes at 4K +-64)")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (the line quotes a median)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    cfg, blk, span = bench.CONFIGS[a.config]
    ref, cur = synth.named_pair(cfg)
    h, w = ref.shape
    F = a.frames
    frames = bench.batch_frames(ref, cur, F)
    ref_t = torch.from_numpy(np.stack([r for r, _ in frames])).to(dev)
    cur_t = torch.from_numpy(np.stack([c for _, c in frames])).to(dev)
    half = blk // 2
    n16, n8 = me.num_blocks(w, h, blk), me.num_blocks(w, h, half)
    mv16 = torch.zeros((F * n16, 2), dtype=torch.int16, device=dev)
    co16 = torch.zeros(F * n16, dtype=torch.int32, device=dev)
    mv8 = torch.zeros((F * n8, 2), dtype=torch.int16, device=dev)
    co8 = torch.zeros(F * n8, dtype=torch.int32, device=dev)
    fields = me.PartitionFields.device(w, h, blk, F, device=dev)
    with me.Engine(devices=[0]) as eng:
        arms = {
            "full_b": eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, blk, span, "sad", 0,
                                                -(-h // blk), mv16, co16),
            "full_half": eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, half, span, "sad", 0,
                                                   -(-h // half), mv8, co8),
            "partition": eng.prepared_partition_search(ref_t, cur_t, blk, span, a.lam, fields),
        }
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.ramp_ms / 1e3:  # warm clock, every arm's code loaded
            for run in arms.values():
                run()
            torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.steps):
            for k, run in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        eng.device_check()
    med = {k: statistics.median(v) * 1e3 / F for k, v in ms.items()}
    lo = {k: min(v) * 1e3 / F for k, v in ms.items()}
    ok = hist = sum_j = sum_d = None
    if not a.no_check:
        import partition_ref as P
        want = P.search_frame(ref, cur, blk, span, a.lam)
        got = fields.numpy()
        n = P.counts(w, h, blk)
        ok = all(np.array_equal(got.mv[k][:n[k]], want.mv[k]) and
                 np.array_equal(got.cost[k][:n[k]], want.cost[k]) for k in range(4))
        ok = bool(ok and np.array_equal(got.mode[:n[0]], want.mode) and
                  np.array_equal(got.mode_cost[:n[0]], want.mode_cost))
        # the partition search's 2Nx2N field is arm (a)'s
        ok = bool(ok and np.array_equal(mv16[:n16].cpu().numpy(), want.mv[0]))
        hist, sum_j, sum_d = P.summary(want, a.lam)
    variant = me.partition_kernel_variant(w, h, ref_t.stride(-2), blk, span)
    print(json.dumps({
        "tool": "partition_time", "config": a.config, "width": w, "height": h, "block": blk,
        "range": span, "cost": "sad", "lambda": a.lam, "frames_per_step": F, "steps": a.steps,
        # each arm's spread over the steps (us per frame), next to the medians below
        "us_per_frame_p10_p90": {k: [round(sorted(v)[int(q * a.steps)] * 1e3 / F, 2) for q in (0.1, 0.9)]
                                 for k, v in ms.items()},
        "kernel_variant": {0: "generic", 1: "fast"}.get(variant, "rejected"),
        "full_b_us_per_frame": round(med["full_b"], 2),
        "full_half_us_per_frame": round(med["full_half"], 2),
        "partition_us_per_frame": round(med["partition"], 2),
        "full_b_us_per_frame_min": round(lo["full_b"], 2),
        "full_half_us_per_frame_min": round(lo["full_half"], 2),
        "partition_us_per_frame_min": round(lo["partition"], 2),
        "partition_over_both": round(med["partition"] / (med["full_b"] + med["full_half"]), 3),
        "partition_over_full_b": round(med["partition"] / med["full_b"], 3),
        "requirement_partition_le_both": bool(med["partition"] <= med["full_b"] + med["full_half"]),
        "frame0_equals_partition_ref": ok, "frame0_mode_histogram": hist,
        "frame0_sum_j": sum_j, "frame0_sum_distortion": sum_d,
        "device": torch.cuda.get_device_name(0)}), flush=True)
    if ok is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
