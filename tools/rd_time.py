#!/usr/bin/env python3
"""Time the rate-constrained search next to the searches on either side of it:
16 resident synthetic frames (bench.py's step: 16x16 blocks, SAD; 1080p +-32, or
--config 4k at +-64),
  (a) me_full_search_batch_device at B = 16,
  (b) me_rd_search_device at lambda = 16 with a zero predictor,
  (c) me_partition_search_device at lambda = 16,
each a step of its own.  HIP events around each step after a clock ramp, the
three arms alternating, the median over the steps.  (b) evaluates every
candidate; so does (c), and (a) where its planner does not prune (4K +-64).
Prints one JSON line and fails unless frame 0's records of (b) equal
tests/rd_ref.py's on --check-blocks evenly spaced blocks and the four corners
(search_block: the definition, block by block; 0 skips the check).
usage: python3 tools/rd_time.py [--steps 40] [--frames 16] [--config 1080p|4k] [--lam 16]
       [--check-blocks 256]"""
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
    n = me.num_blocks(w, h, blk)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    mv_a, co_a = z((F * n, 2), torch.int16), z(F * n, torch.int32)
    mv_b, j_b, d_b = z((F * n, 2), torch.int16), z(F * n, torch.int32), z(F * n, torch.int32)
    r_b = z(F * n, torch.uint8)
    pred = z((F * n, 2), torch.int16)
    fields = me.PartitionFields.device(w, h, blk, F, device=dev)
    with me.Engine(devices=[0]) as eng:
        arms = {
            "full": eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, blk, span, "sad", 0,
                                              -(-h // blk), mv_a, co_a),
            "rd": eng.prepared_rd_search(ref_t, cur_t, blk, span, a.lam, mv_b, j_b, d_b, r_b, pred),
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
    mv, j, d, r = (mv_b[:n].cpu().numpy(), j_b[:n].cpu().numpy().view(np.uint32),
                   d_b[:n].cpu().numpy().view(np.uint32), r_b[:n].cpu().numpy())
    ok, checked = None, 0
    if a.check_blocks > 0:
        import rd_ref as R
        nbx, nby = -(-w // blk), -(-h // blk)
        pick = set(np.linspace(0, n - 1, min(a.check_blocks, n)).astype(int).tolist())
        pick |= {0, nbx - 1, n - nbx, n - 1}
        ok = True
        for b in sorted(pick):
            want = R.search_block(ref, cur, blk, span, a.lam, None, b % nbx, b // nbx)
            ok = ok and want == (tuple(int(v) for v in mv[b]), int(j[b]), int(d[b]), int(r[b]))
        ok, checked = bool(ok), len(pick)
    variant = me.rd_kernel_variant(w, h, ref_t.stride(-2), blk, span, a.lam)
    zero = int(((mv[:, 0] == 0) & (mv[:, 1] == 0)).sum())
    print(json.dumps({
        "tool": "rd_time", "config": a.config, "width": w, "height": h, "block": blk,
        "range": span, "cost": "sad", "lambda": a.lam, "frames_per_step": F, "steps": a.steps,
        # each arm's spread over the steps (us per frame), next to the medians below
        "us_per_frame_p10_p90": {k: [round(sorted(v)[int(q * a.steps)] * 1e3 / F, 2) for q in (0.1, 0.9)]
                                 for k, v in ms.items()},
        "kernel_variant": {0: "generic", 1: "fast"}.get(variant, "rejected"),
        "full_us_per_frame": round(med["full"], 2),
        "rd_us_per_frame": round(med["rd"], 2),
        "partition_us_per_frame": round(med["partition"], 2),
        "full_us_per_frame_min": round(lo["full"], 2),
        "rd_us_per_frame_min": round(lo["rd"], 2),
        "partition_us_per_frame_min": round(lo["partition"], 2),
        "rd_over_full": round(med["rd"] / med["full"], 3),
        "rd_over_partition": round(med["rd"] / med["partition"], 3),
        "requirement_rd_le_partition": bool(med["rd"] <= med["partition"]),
        "frame0_equals_rd_ref": ok, "frame0_blocks_checked": checked,
        "frame0_sum_j": int(j.astype(np.int64).sum()),
        "frame0_sum_distortion": int(d.astype(np.int64).sum()),
        "frame0_sum_bits": int(r.astype(np.int64).sum()), "frame0_zero_vectors": zero,
        "frame0_full_search_sum_sad": int(co_a[:n].cpu().numpy().view(np.uint32).astype(np.int64).sum()),
        "device": torch.cuda.get_device_name(0)}), flush=True)
    if ok is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
