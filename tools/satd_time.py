#!/usr/bin/env python3
"""Time the SATD cost next to the SAD one in the quarter-pel refinement and the
bi-prediction: 16 resident 1080p synthetic frames (bench.py's step: 16x16
blocks, +-32), the integer searches always at SAD.  Arms, alternating step by
step on one stream:
  search                      the batched search (ref0 against cur)
  search_refine_sad / _satd   the search and me_refine_qpel_device at that cost
  pair_refine_sad / _satd     both searches (ref0, ref1) and both refinements
  pair_bipred_sad / _satd     the same and me_bipred_device at that cost
HIP events around each step after a clock ramp, the median over the steps (and
the 10th / 90th percentile of the steps, for A/B comparisons).  A kernel's time
is the difference of two medians.  Prints one JSON line.
usage: python3 tools/satd_time.py [--steps 40] [--frames 16] [--config 1080p] [--sad-only]
--sad-only leaves the SATD arms out (a library built before the cost existed,
loaded with ME_HIP_LIB, for an A/B of the SAD arms).  ref1 of frame f is the
reference of frame f + 1 of the batch.  The line also says whether frame 0's
SATD refinement and SATD bi-prediction equal the numpy oracle's
(tests/satd_ref.py)."""
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
    ap.add_argument("--ramp-ms", type=float, default=300.0)
    ap.add_argument("--sad-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 40:
        ap.error("--steps must be at least 40 (the line quotes a median and percentiles)")
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
    mv0, mv1 = i16(), i16()                      # the searched integer fields
    co = i32(F * nb)
    costs = ["sad"] if a.sad_only else ["sad", "satd"]
    # per cost: refined fields and their costs, bi-prediction outputs
    buf = {c: dict(q0=i16(), q1=i16(), c0=i32(F * nb), c1=i32(F * nb), o0=i16(), o1=i16(),
                   bc=i32(F * nb), c3=i32(F * nb, 3),
                   mode=torch.zeros(F * nb, dtype=torch.uint8, device=dev)) for c in costs}
    with me.Engine(devices=[0]) as eng:
        search0 = eng.prepared_batch_search(ref0_t, 0, cur_t, 0, w, h, blk, span, "sad", 0, nby,
                                            mv0, co)
        search1 = eng.prepared_batch_search(ref1_t, 0, cur_t, 0, w, h, blk, span, "sad", 0, nby,
                                            mv1, co)
        arms = {"search": lambda: search0()}
        for c in costs:
            b = buf[c]
            r0 = eng.prepared_refine_qpel(ref0_t, cur_t, blk, c, mv0, b["q0"], b["c0"])
            r1 = eng.prepared_refine_qpel(ref1_t, cur_t, blk, c, mv1, b["q1"], b["c1"])
            bi = eng.prepared_bipred(ref0_t, ref1_t, cur_t, blk, c, b["q0"], b["q1"], b["mode"],
                                     b["o0"], b["o1"], b["bc"], b["c3"])
            arms["search_refine_" + c] = lambda r0=r0: (search0(), r0())
            arms["pair_refine_" + c] = lambda r0=r0, r1=r1: (search0(), r0(), search1(), r1())
            arms["pair_bipred_" + c] = lambda r0=r0, r1=r1, bi=bi: (search0(), r0(), search1(),
                                                                    r1(), bi())
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
    us = {k: sorted(x * 1e3 / F for x in v) for k, v in ms.items()}  # us per frame, ascending
    med = {k: statistics.median(v) for k, v in us.items()}
    pct = lambda v, p: v[min(len(v) - 1, int(p * len(v)))]
    out = {"tool": "satd_time", "config": a.config, "width": w, "height": h, "block": blk,
           "range": span, "frames_per_step": F, "steps": a.steps, "search_path": path}
    for k in arms:
        out[k + "_us_per_frame"] = round(med[k], 2)
        out[k + "_us_per_frame_p10_p90"] = [round(pct(us[k], 0.1), 2), round(pct(us[k], 0.9), 2)]
    ok = True
    for c in costs:
        out[f"refine_{c}_us_per_frame"] = round(med["search_refine_" + c] - med["search"], 2)
        out[f"bipred_{c}_us_per_frame"] = round(med["pair_bipred_" + c] - med["pair_refine_" + c], 2)
    if not a.sad_only:
        out["refine_satd_over_sad"] = round(out["refine_satd_us_per_frame"] /
                                            out["refine_sad_us_per_frame"], 3)
        out["bipred_satd_over_sad"] = round(out["bipred_satd_us_per_frame"] /
                                            out["bipred_sad_us_per_frame"], 3)
        import qpel_ref
        import satd_ref
        host = lambda t: t[:nb].cpu().numpy()
        b = buf["satd"]
        imv0 = host(mv0)
        oq, oc = satd_ref.refine(refs[0], frames[0][1], blk, imv0)
        sq, _ = qpel_ref.refine(refs[0], frames[0][1], blk, imv0, "sad")
        ok_refine = bool(np.array_equal(host(b["q0"]), oq) and
                         np.array_equal(host(b["c0"]).view(np.uint32), oc))
        want = satd_ref.bipred(refs[0], refs[1], frames[0][1], blk, host(b["q0"]), host(b["q1"]), 1)
        got = (host(b["o0"]), host(b["o1"]), host(b["mode"]), host(b["bc"]).view(np.uint32),
               host(b["c3"]).view(np.uint32))
        ok_bipred = all(np.array_equal(g, x) for g, x in zip(got, want))
        ok = ok_refine and ok_bipred
        out["frame0_refine_equals_oracle"] = ok_refine
        out["frame0_bipred_equals_oracle"] = bool(ok_bipred)
        out["frame0_blocks_satd_differs_from_sad"] = round(float((oq != sq).any(axis=1).mean()), 3)
        out["frame0_modes_l0_l1_bi"] = [int(v) for v in np.bincount(want[2], minlength=3)]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
