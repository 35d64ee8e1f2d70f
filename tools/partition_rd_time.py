#!/usr/bin/env python3
"""Time the rate-constrained partition search next to the calls it replaces:
16 resident synthetic frames (bench.py's step: 16x16 macroblocks, SAD; 1080p
+-32, or --config 4k at +-64), lambda = 16, zero predictor,
  (b16) me_rd_search_device at B = 16,
  (b8)  me_rd_search_device at B = 8,
  (c)   me_partition_search_device,
  (d)   me_partition_rd_search_device,
each a step of its own.  HIP events around each step after a clock ramp, the
four arms alternating, the median over the steps.  Requirement: (d) <= (b16) +
(b8), the two calls a caller would otherwise run for a rate-distortion-optimal
shape.  Prints one JSON line and fails unless frame 0's records of (d) equal
tests/partition_rd_ref.py's on --check-blocks evenly spaced macroblocks and the
four corners (search_macroblock: the definition, macroblock by macroblock, all
nine partitions and the mode; 0 skips the check).
usage: python3 tools/partition_rd_time.py [--steps 40] [--frames 16] [--config 1080p|4k]
       [--lam 16] [--check-blocks 256]"""
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

# VALU instructions per candidate group (one dy row of a lane: 4 dx x 9
# partitions), counted in the compiled gfx950 kernels' epilogues (DESIGN.md
# "Rate-constrained partition search"): 64 qsads in both, then (c) 96.7 in the
# masked epilogue, the one that runs (56.5 in the unmasked one), (d) 102.5 in
# its only epilogue.  The prediction takes every VALU instruction at one cost.
GROUP_C, GROUP_C_UNMASKED, GROUP_D = 64 + 96.7, 64 + 56.5, 64 + 102.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lam", type=int, default=16)
    ap.add_argument("--ramp-ms", type=float, default=300.0)
    ap.add_argument("--check-blocks", type=int, default=256)
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
    n16, n8 = me.num_blocks(w, h, blk), me.num_blocks(w, h, blk // 2)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    rd = {n: (z((F * n, 2), torch.int16), z(F * n, torch.int32), z(F * n, torch.int32),
              z(F * n, torch.uint8), z((F * n, 2), torch.int16)) for n in (n16, n8)}
    part = me.PartitionFields.device(w, h, blk, F, device=dev)
    fields = me.PartitionRdFields.device(w, h, blk, F, device=dev)
    pred = z((F * n16, 2), torch.int16)
    with me.Engine(devices=[0]) as eng:
        arms = {
            "rd16": eng.prepared_rd_search(ref_t, cur_t, blk, span, a.lam, *rd[n16]),
            "rd8": eng.prepared_rd_search(ref_t, cur_t, blk // 2, span, a.lam, *rd[n8]),
            "partition": eng.prepared_partition_search(ref_t, cur_t, blk, span, a.lam, part),
            "partition_rd": eng.prepared_partition_rd_search(ref_t, cur_t, blk, span, a.lam,
                                                             fields, pred),
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
    cells = me.partition_counts(w, h, blk)
    got = fields.numpy()
    ok, checked = None, 0
    if a.check_blocks > 0:
        import partition_rd_ref as Q
        nbx = -(-w // blk)
        pick = set(np.linspace(0, n16 - 1, min(a.check_blocks, n16)).astype(int).tolist())
        pick |= {0, nbx - 1, n16 - nbx, n16 - 1}
        ok = True
        for b in sorted(pick):
            rec, mode, cost = Q.search_macroblock(ref, cur, blk, span, a.lam, None, b % nbx,
                                                  b // nbx)
            ok = ok and (mode, cost) == (int(got.mode[b]), int(got.mode_cost[b]))
            for (k, c), want in rec.items():
                ok = ok and want == (tuple(int(v) for v in got.mv[k][c]), int(got.cost[k][c]),
                                     int(got.dist[k][c]), int(got.bits[k][c]))
        ok, checked = bool(ok), len(pick)
    variant = me.partition_rd_kernel_variant(w, h, ref_t.stride(-2), blk, span, a.lam)
    both = med["rd16"] + med["rd8"]
    print(json.dumps({
        "tool": "partition_rd_time", "config": a.config, "width": w, "height": h, "block": blk,
        "range": span, "cost": "sad", "lambda": a.lam, "frames_per_step": F, "steps": a.steps,
        # each arm's spread over the steps (us per frame), next to the medians below
        "us_per_frame_p10_p90": {k: [round(sorted(v)[int(q * a.steps)] * 1e3 / F, 2) for q in (0.1, 0.9)]
                                 for k, v in ms.items()},
        "kernel_variant": {0: "generic", 1: "fast"}.get(variant, "rejected"),
        "rd16_us_per_frame": round(med["rd16"], 2),
        "rd8_us_per_frame": round(med["rd8"], 2),
        "partition_us_per_frame": round(med["partition"], 2),
        "partition_rd_us_per_frame": round(med["partition_rd"], 2),
        "rd16_us_per_frame_min": round(lo["rd16"], 2),
        "rd8_us_per_frame_min": round(lo["rd8"], 2),
        "partition_us_per_frame_min": round(lo["partition"], 2),
        "partition_rd_us_per_frame_min": round(lo["partition_rd"], 2),
        "rd16_plus_rd8_us_per_frame": round(both, 2),
        "partition_rd_over_rd16_plus_rd8": round(med["partition_rd"] / both, 3),
        "requirement_partition_rd_le_rd16_plus_rd8": bool(med["partition_rd"] <= both),
        "partition_rd_over_partition": round(med["partition_rd"] / med["partition"], 3),
        "partition_rd_over_partition_by_instruction_count": round(GROUP_D / GROUP_C, 3),
        "partition_rd_over_partition_by_instruction_count_unmasked":
            round(GROUP_D / GROUP_C_UNMASKED, 3),
        "frame0_equals_partition_rd_ref": ok, "frame0_macroblocks_checked": checked,
        "frame0_mode_histogram": np.bincount(got.mode[:n16], minlength=4).tolist(),
        "frame0_sum_mode_cost": int(got.mode_cost[:n16].astype(np.int64).sum()),
        "frame0_sum_dist": [int(got.dist[k][:cells[k]].astype(np.int64).sum()) for k in range(4)],
        "frame0_sum_bits": [int(got.bits[k][:cells[k]].astype(np.int64).sum()) for k in range(4)],
        "device": torch.cuda.get_device_name(0)}), flush=True)
    if ok is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
