#!/usr/bin/env python3
"""Time the bi-prediction kernel next to the quarter-pel refinement it follows:
16 resident 1080p synthetic frames (bench.py's step: 16x16 blocks, +-32, SAD),
per step on one stream the two batched searches (ref0 and ref1 against cur) and
their two refinements, and then the same plus me_bipred_device.  HIP events
around each step after a clock ramp, the arms alternating, the median over the
steps.  A third arm (the two searches alone) gives the refinement's time in the
same run: the yardstick, since it stages one window per block where the
bi-prediction stages two.  Prints one JSON line.
usage: python3 tools/bipred_time.py [--steps 40] [--frames 16] [--cost sad] [--config 1080p]
ref1 of frame f is the reference of frame f + 1 of the batch (another shift of
the same scene).  The line also says whether frame 0's result equals the numpy
oracle's (tests/bipred_ref.py) on the refined fields."""
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
    refs = [r for r, _ in frames]
    ref0_t = torch.from_numpy(np.stack(refs)).to(dev)
    ref1_t = torch.from_numpy(np.stack(refs[1:] + refs[:1])).to(dev)
    cur_t = torch.from_numpy(np.stack([c for _, c in frames])).to(dev)
    nb = me.num_blocks(w, h, blk)
    nby = (h + blk - 1) // blk
    i16 = lambda: torch.zeros((F * nb, 2), dtype=torch.int16, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    q0, q1, o0, o1 = i16(), i16(), i16(), i16()
    co, c0, c1, bc, c3 = i32(F * nb), i32(F * nb), i32(F * nb), i32(F * nb), i32(F * nb, 3)
    mode = torch.zeros(F * nb, dtype=torch.uint8, device=dev)
    with me.Engine(devices=[0]) as eng:
        search0 = eng.prepared_batch_search(ref0_t, 0, cur_t, 0, w, h, blk, span, a.cost, 0, nby,
                                            q0, co)
        search1 = eng.prepared_batch_search(ref1_t, 0, cur_t, 0, w, h, blk, span, a.cost, 0, nby,
                                            q1, co)
        refine0 = eng.prepared_refine_qpel(ref0_t, cur_t, blk, a.cost, q0, None, c0)
        refine1 = eng.prepared_refine_qpel(ref1_t, cur_t, blk, a.cost, q1, None, c1)
        bipred = eng.prepared_bipred(ref0_t, ref1_t, cur_t, blk, a.cost, q0, q1, mode, o0, o1, bc, c3)
        arms = {"search": lambda: (search0(), search1()),
                "search_refine": lambda: (search0(), refine0(), search1(), refine1()),
                "search_refine_bipred": lambda: (search0(), refine0(), search1(), refine1(),
                                                 bipred())}
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
        path = eng.last_search_path()
    med = {k: statistics.median(v) * 1e3 / F for k, v in ms.items()}  # us per frame
    bipred_us = med["search_refine_bipred"] - med["search_refine"]
    refine_us = (med["search_refine"] - med["search"]) / 2  # one refinement
    # all three planes once, both fields in and out, mode, cost and cost3 out
    hbm = 3 * w * h + nb * (4 * 4 + 1 + 4 + 12)
    import bipred_ref
    host = lambda t: t[:nb].cpu().numpy()
    want = bipred_ref.bipred(refs[0], refs[1], frames[0][1], blk, host(q0), host(q1), a.cost, 1)
    got = (host(o0), host(o1), host(mode), host(bc).view(np.uint32), host(c3).view(np.uint32))
    ok = all(np.array_equal(g, x) for g, x in zip(got, want))
    hist = np.bincount(want[2], minlength=3)
    print(json.dumps({
        "tool": "bipred_time", "config": a.config, "width": w, "height": h, "block": blk,
        "range": span, "cost": a.cost, "frames_per_step": F, "steps": a.steps,
        # each arm's spread over the steps (us per frame), next to the medians below
        "us_per_frame_p10_p90": {k: [round(sorted(v)[int(q * a.steps)] * 1e3 / F, 2) for q in (0.1, 0.9)]
                                 for k, v in ms.items()},
        "search_path": path,
        "search_us_per_frame": round(med["search"], 2),
        "search_refine_us_per_frame": round(med["search_refine"], 2),
        "search_refine_bipred_us_per_frame": round(med["search_refine_bipred"], 2),
        "refine_us_per_frame": round(refine_us, 2),
        "bipred_us_per_frame": round(bipred_us, 2),
        "bipred_over_refine": round(bipred_us / refine_us, 3) if refine_us > 0 else None,
        "search_refine_us_per_frame_min": round(min(ms["search_refine"]) * 1e3 / F, 2),
        "search_refine_bipred_us_per_frame_min":
            round(min(ms["search_refine_bipred"]) * 1e3 / F, 2),
        "bipred_hbm_bytes_per_frame": hbm,
        "bipred_hbm_gb_per_s": round(hbm / (bipred_us * 1e-6) / 1e9, 1) if bipred_us > 0 else None,
        "frame0_equals_oracle": bool(ok),
        "frame0_modes_l0_l1_bi": [int(v) for v in hist],
        "device": torch.cuda.get_device_name(0)}), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
