#!/usr/bin/env python3
"""Time the quarter-pel refinement next to the search it follows: 16 resident
1080p synthetic frames (bench.py's step: 16x16 blocks, +-32, SAD), the batched
search alone and then the search plus me_refine_qpel_device on the same stream.
HIP events around each step after a clock ramp, the two arms alternating, the
median over the steps.  Prints one JSON line; the refinement's time is the
difference of the two medians, its algorithmic HBM bytes are both planes once
plus the records (integer field in, quarter-pel field and costs out).
usage: python3 tools/qpel_time.py [--steps 40] [--frames 16] [--cost sad] [--config 1080p]
The line also says whether frame 0's refined field equals the numpy oracle's
(tests/qpel_ref.py) on the searched field."""
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
    ap.add_argument("--cost", default="sad")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--ramp-ms", type=float, default=300.0)
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
    nb = me.num_blocks(w, h, blk)
    nby = (h + blk - 1) // blk
    mv = torch.zeros((F * nb, 2), dtype=torch.int16, device=dev)
    q = torch.zeros((F * nb, 2), dtype=torch.int16, device=dev)
    co = torch.zeros(F * nb, dtype=torch.int32, device=dev)
    qco = torch.zeros(F * nb, dtype=torch.int32, device=dev)
    with me.Engine(devices=[0]) as eng:
        search = eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, blk, span, a.cost, 0, nby,
                                           mv, co)
        refine = eng.prepared_refine_qpel(ref_t, cur_t, blk, a.cost, mv, q, qco)
        arms = {"search": lambda: search(), "search_refine": lambda: (search(), refine())}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.ramp_ms / 1e3:  # warm clock, both arms' code loaded
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
        path = eng.last_search_path()
    med = {k: statistics.median(v) for k, v in ms.items()}
    refine_us = (med["search_refine"] - med["search"]) * 1e3 / F
    search_us = med["search"] * 1e3 / F
    hbm = 2 * w * h + nb * (4 + 4 + 4)  # both planes once, mv in, q and cost out
    import qpel_ref
    oq, oc = qpel_ref.refine(ref, cur, blk, mv[:nb].cpu().numpy(), a.cost)
    ok = bool(np.array_equal(q[:nb].cpu().numpy(), oq) and
              np.array_equal(qco[:nb].cpu().numpy().view(np.uint32), oc))
    frac = float(np.mean((oq % 4 != 0).any(axis=1)))
    print(json.dumps({
        "tool": "qpel_time", "config": a.config, "width": w, "height": h, "block": blk,
        "range": span, "cost": a.cost, "frames_per_step": F, "steps": a.steps,
        "search_path": path,
        "search_us_per_frame": round(search_us, 2),
        "search_refine_us_per_frame": round(med["search_refine"] * 1e3 / F, 2),
        "refine_us_per_frame": round(refine_us, 2),
        "refine_share_of_search": round(refine_us / search_us, 3),
        "search_us_per_frame_min": round(min(ms["search"]) * 1e3 / F, 2),
        "search_refine_us_per_frame_min": round(min(ms["search_refine"]) * 1e3 / F, 2),
        # the spread of the steps, for an A/B of two builds
        "search_refine_us_per_frame_p10_p90": [
            round(sorted(ms["search_refine"])[int(p * a.steps)] * 1e3 / F, 2) for p in (0.1, 0.9)],
        "refine_hbm_bytes_per_frame": hbm,
        "refine_hbm_gb_per_s": round(hbm / (refine_us * 1e-6) / 1e9, 1) if refine_us > 0 else None,
        "frame0_equals_oracle": ok, "frame0_fractional_blocks": round(frac, 3),
        "device": torch.cuda.get_device_name(0)}), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
