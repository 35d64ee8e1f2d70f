#!/usr/bin/env python3
"""Time the partition-wise quarter-pel refinement next to what the block
refinement can do instead: 16 resident synthetic 1080p frames (bench.py's step:
16x16 macroblocks, +-32), lambda = 16, zero predictor,
  (search)          me_partition_rd_search_device alone,
  (search_sad/satd) the search, then me_partition_refine_qpel_device in place at
                    SAD / SATD; minus (search) it is the refinement's time,
  (refine_sad/satd) the refinement alone on the searched grids, as a cross-check
                    of that difference,
  (blocks_sad/satd) me_refine_qpel_rd_device at B on the 2Nx2N grid plus at B / 2
                    on the NxN grid: the only two shapes the block refinement
                    takes, half the pixels the partition-wise one refines,
each a step of its own.  HIP events around each step after a clock ramp, the
arms alternating, the median over the steps.  Goal: refinement <= 2.0 x blocks.
Prints one JSON line and fails unless frame 0's refined records equal
tests/partition_qpel_ref.py's (refine_rect: the definition, cell by cell) on
--check-blocks evenly spaced macroblocks and the four corners, the clipped
bottom row included (0 skips the check).  --content tiles times frames whose macroblocks mostly
hold several integer vectors (less window sharing) instead of bench.py's pan.
usage: python3 tools/partition_qpel_time.py [--steps 40] [--frames 16] [--config 1080p]
       [--lam 16] [--check-blocks 48] [--content pan|tiles] [--out FILE]"""
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

COSTS = ("sad", "satd")


def check_frame0(ref, cur, blk, lam, mv, got, cost, n_check):
    """got's records of the sampled macroblocks against the cell-by-cell
    restatement on the integer grids mv: (all equal, macroblocks checked)."""
    import partition_qpel_ref as PQ
    import partition_rd_ref as PR
    import partition_ref as P
    h, w = ref.shape
    g = P.grids(w, h, blk)
    nbx, nby = g[0]
    n = nbx * nby
    pick = set(np.linspace(0, n - 1, min(n_check, n)).astype(int).tolist())
    pick |= {0, nbx - 1, n - nbx, n - 1}
    ok = True
    for b in sorted(pick):
        bx, by = b % nbx, b // nbx
        x0, y0 = bx * blk, by * blk
        J = [lam * m for m in PR.MBITS]
        for gi, i, j, qx, qy, qw, qh in P._partitions(blk, min(blk, w - x0), min(blk, h - y0)):
            sx, sy = PR.REP[gi]
            c = (sy * by + j) * g[gi][0] + sx * bx + i
            m = tuple(int(v) for v in mv[gi][c])
            q, (jj, d, r), _ = PQ.refine_rect(ref, cur, x0 + qx, y0 + qy, qw, qh, m, lam, (0, 0), cost)
            ok = ok and (q, jj, d, r) == (tuple(int(v) for v in got.mv[gi][c]), int(got.cost[gi][c]),
                                          int(got.dist[gi][c]), int(got.bits[gi][c]))
            J[gi] += jj
        mode = min(range(4), key=lambda k: (J[k], k))
        ok = ok and (mode, J[mode]) == (int(got.mode[b]), int(got.mode_cost[b]))
    return bool(ok), len(pick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lam", type=int, default=16)
    ap.add_argument("--ramp-ms", type=float, default=300.0)
    ap.add_argument("--check-blocks", type=int, default=48)
    ap.add_argument("--content", default="pan", choices=("pan", "tiles"),
                    help="pan: bench.py's frames, one translation per frame (nearly every "
                         "macroblock holds one integer vector); tiles: "
                         "tests/partition_qpel_ref.content, every 8x8 tile at its own half-pel "
                         "offset (most macroblocks hold several)")
    ap.add_argument("--out", help="append the JSON line to this file as well "
                                  "(profiles/partition_qpel_time_1080p.jsonl)")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (the line quotes a median)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    cfg, blk, span = bench.CONFIGS[a.config]
    ref, cur = synth.named_pair(cfg)
    h, w = ref.shape
    F = a.frames
    if a.content == "tiles":
        import partition_qpel_ref as PQ
        pairs = [PQ.content(w, h, blk // 2, 7 + f, blk) for f in range(2)]
        ref, cur = pairs[0]
        frames = [pairs[f % 2] for f in range(F)]
    else:
        frames = bench.batch_frames(ref, cur, F)
    ref_t = torch.from_numpy(np.stack([r for r, _ in frames])).to(dev)
    cur_t = torch.from_numpy(np.stack([c for _, c in frames])).to(dev)
    cells = me.partition_counts(w, h, blk)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    searched = me.PartitionRdFields.device(w, h, blk, F, device=dev)   # integer grids
    chained = me.PartitionRdFields.device(w, h, blk, F, device=dev)    # search, refined in place
    refined = {c: me.PartitionRdFields.device(w, h, blk, F, device=dev) for c in COSTS}
    pred = z((F * cells[0], 2), torch.int16)
    # the block refinement's outputs: (q, J, dist) per grid
    blocks = {k: (z((F * cells[k], 2), torch.int16), z(F * cells[k], torch.int32),
                  z(F * cells[k], torch.int32)) for k in (0, 3)}
    pred8 = z((F * cells[3], 2), torch.int16)
    with me.Engine(devices=[0]) as eng:
        search = eng.prepared_partition_rd_search(ref_t, cur_t, blk, span, a.lam, searched, pred)
        search_c = eng.prepared_partition_rd_search(ref_t, cur_t, blk, span, a.lam, chained, pred)
        in_place = {c: eng.prepared_partition_refine_qpel(ref_t, cur_t, blk, c, a.lam, chained,
                                                          chained, pred) for c in COSTS}
        alone = {c: eng.prepared_partition_refine_qpel(ref_t, cur_t, blk, c, a.lam, searched,
                                                       refined[c], pred) for c in COSTS}

        def blocks_arm(c):
            def run():
                eng.refine_qpel_rd_device(ref_t, cur_t, blk, c, a.lam, searched.mv[0], *blocks[0], pred)
                eng.refine_qpel_rd_device(ref_t, cur_t, blk // 2, c, a.lam, searched.mv[3], *blocks[3],
                                          pred8)
            return run

        def chain(c):
            return lambda: (search_c(), in_place[c]())
        search()  # the integer grids the stand-alone arms read
        torch.cuda.synchronize()
        arms = {"search": search}
        for c in COSTS:
            arms["search_" + c] = chain(c)
            arms["refine_" + c] = alone[c]
            arms["blocks_" + c] = blocks_arm(c)
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
    ints = searched.numpy()
    mv0 = [ints.mv[k][:cells[k]] for k in range(4)]
    out = {
        "tool": "partition_qpel_time", "config": a.config, "content": a.content, "width": w, "height": h, "block": blk,
        "range": span, "lambda": a.lam, "frames_per_step": F, "steps": a.steps,
        "us_per_frame": {k: round(v, 2) for k, v in med.items()},
        "us_per_frame_p10_p90": {k: [round(sorted(v)[int(q * a.steps)] * 1e3 / F, 2) for q in (0.1, 0.9)]
                                 for k, v in ms.items()},
    }
    ok_all = True
    for c in COSTS:
        diff = med["search_" + c] - med["search"]
        out[c] = {
            "refinement_us_per_frame_by_difference": round(diff, 2),
            "refinement_us_per_frame_alone": round(med["refine_" + c], 2),
            "blocks_us_per_frame": round(med["blocks_" + c], 2),
            "refinement_over_blocks": round(diff / med["blocks_" + c], 3),
            "refinement_alone_over_blocks": round(med["refine_" + c] / med["blocks_" + c], 3),
            "goal_refinement_le_2x_blocks": bool(diff <= 2.0 * med["blocks_" + c]),
        }
        got = refined[c].numpy()
        if a.check_blocks > 0:
            ok, checked = check_frame0(ref, cur, blk, a.lam, mv0, got, c, a.check_blocks)
            out[c]["frame0_equals_partition_qpel_ref"] = ok
            out[c]["frame0_macroblocks_checked"] = checked
            ok_all = ok_all and ok
        out[c]["frame0_mode_histogram"] = np.bincount(got.mode[:cells[0]], minlength=4).tolist()
        out[c]["frame0_sum_mode_cost"] = int(got.mode_cost[:cells[0]].astype(np.int64).sum())
    out["frame0_integer_mode_histogram"] = np.bincount(ints.mode[:cells[0]], minlength=4).tolist()
    # how much the nine partitions of a macroblock share: distinct integer vectors
    import partition_rd_ref as PR
    nbx, nby = -(-w // blk), -(-h // blk)
    per = []
    for k in range(4):
        sx, sy = PR.REP[k]
        nx, ny = sx * nbx, sy * nby
        v = np.full((ny, nx), -1, np.int64)  # (a missing cell repeats none)
        gx, gy = -(-w // (blk // sx)), -(-h // (blk // sy))
        key = (mv0[k][:, 1].astype(np.int64) + 32768) * 65536 + mv0[k][:, 0].astype(np.int64) + 32768
        v[:gy, :gx] = key.reshape(gy, gx)
        per.append(v.reshape(nby, sy, nbx, sx).transpose(0, 2, 1, 3).reshape(nby * nbx, sx * sy))
    allv = np.concatenate(per, axis=1)
    distinct = np.array([len(set(r.tolist()) - {-1}) for r in allv])
    out["frame0_distinct_integer_vectors_per_macroblock_mean"] = round(float(distinct.mean()), 3)
    out["frame0_macroblocks_with_one_vector"] = int((distinct == 1).sum())
    out["frame0_macroblocks"] = int(nbx * nby)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
