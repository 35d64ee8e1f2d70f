#!/usr/bin/env python3
"""Per-wave timeline of the SAD flow kernel from the ME_STAMPS diagnostic build
(libme_hip_stamps.so): start-up delay to the first task, time spent waiting for
items, tasks per wave, and how the waves / CUs finish.  Diagnostic only (the
stamps cost cycles themselves); times in shader cycles unless marked.
The stamps library carries the tuning build's overrides (me_tuning.h), so e.g.
ME_PRUNE_SPLIT=0 gives the wave-task durations without the row split.
usage: python3 tools/flow_stamps.py [r0:r1 (one stripe's block rows: the split mode) | batchF]"""
import os, sys
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from motionestimation_amd import _lib, synth
# FLOW_STAMPS_LIB: another stamps build in motionestimation_amd/lib (e.g. one of
# the parent commit's kernels, for the "before" of a kernel change)
_lib.LIB_PATH = os.path.join(REPO, "motionestimation_amd", "lib",
                             os.path.basename(os.environ.get("FLOW_STAMPS_LIB", "libme_hip_stamps.so")))
import ctypes
import motionestimation_amd as me

ref, cur = synth.named_pair("1080p")
eng = me.Engine(devices=[0])
rt, ct = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
n = me.num_blocks(1920, 1080, 16)
mv = torch.empty((n, 2), dtype=torch.int16, device="cuda")
co = torch.empty(n, dtype=torch.int32, device="cuda")
rows = sys.argv[1] if len(sys.argv) > 1 else ""
if rows.startswith("batch"):  # batchF: F frames in one launch (me_full_search_batch_device)
    F = int(rows[5:])
    rows = ""
    rb = torch.from_numpy(np.stack([ref] * F)).cuda()
    cb = torch.from_numpy(np.stack([cur] * F)).cuda()
    mvb = torch.empty((F * n, 2), dtype=torch.int16, device="cuda")
    cob = torch.empty(F * n, dtype=torch.int32, device="cuda")
    for _ in range(40):  # past the clock ramp (tools/dbg/ramp_probe.py)
        eng.search_batch_device(rb, 0, cb, 0, 1920, 1080, 16, 32, "sad", 0, 68, mvb, cob)
else:
    for _ in range(400):  # past the clock ramp (tools/dbg/ramp_probe.py)
        eng.full_search_device(rt, ct, 16, 32, "sad", mv, co)
for _ in range(20):
    if "F" in dir() and not rows:
        eng.search_batch_device(rb, 0, cb, 0, 1920, 1080, 16, 32, "sad", 0, 68, mvb, cob)
    elif rows:
        a, b = (int(x) for x in rows.split(":"))
        eng.search_stripe_device(rt, 0, ct, 0, 1920, 1080, 16, 32, "sad", a, b, mv, co)
    else:
        eng.full_search_device(rt, ct, 16, 32, "sad", mv, co)
torch.cuda.synchronize()
L = _lib.lib()
L.me_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
buf = np.zeros(8 << 16, np.uint64)
L.me_debug_stamps(buf.ctypes.data, buf.size)
st = buf.reshape(-1, 8)[:4096].astype(np.int64)
if os.environ.get("FLOW_STAMPS_SAVE"):  # raw per-wave records for offline analysis
    np.save(os.environ["FLOW_STAMPS_SAVE"], st)
st = st[st[:, 0] > 0]
start, first, end, spin, ntask = st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4]
r0, r1 = st[:, 5], st[:, 6]
life = end - start
print(f"waves {len(st)}; tasks per wave: {np.bincount(ntask)}")
print(f"start -> first task (cycles): median {np.median(first - start):.0f} p90 {np.percentile(first - start, 90):.0f} max {(first - start).max():.0f}")
print(f"wave life: median {np.median(life):.0f}; spin share of life: median {np.median(spin / life):.3f} mean {np.mean(spin / life):.3f}")
base = r0.min()
print(f"realtime (us): starts {0:.2f}..{(r0.max() - base) / 100:.2f}; ends {(r1.min() - base) / 100:.2f}..{(r1.max() - base) / 100:.2f} median {(np.median(r1) - base) / 100:.2f}")
wg = np.arange(len(st)) // 16
cu_end = np.array([r1[wg == g].max() for g in np.unique(wg)]) - base
cu_first_end = np.array([r1[wg == g].min() for g in np.unique(wg)]) - base
print(f"per-CU (workgroup) end (us): min {cu_end.min()/100:.2f} median {np.median(cu_end)/100:.2f} max {cu_end.max()/100:.2f}; "
      f"spread inside a CU (last - first wave end): median {np.median(cu_end - cu_first_end)/100:.2f}")
clk = life / ((r1 - r0) / 100e6) / 1e9
print(f"clock (GHz): median {np.median(clk):.3f}")

# Where the SIMD-cycles go: hw_id (gfx9 HW_REG_HW_ID) bits 5:4 = SIMD; workgroup
# b runs on XCD b % 8 (round-robin dispatch).  Per SIMD: idle before its first
# task (from the kernel's first wave start) and after its last wave ends (to
# the kernel's last wave end), in us of realtime.
hw = st[:, 7] & 0xFFFFFFFF
if (st[:, 7] >> 32).any():  # (a stamps build from before the slot count was recorded leaves 0)
    print(f"ring slots of the launch: {int((st[:, 7] >> 32).max())}")
simd = (hw >> 4) & 3
kend = r1.max()
first_rt = r0 + (first - start) / np.maximum(clk, 1e-3) / 10.0  # cycles -> 10 ns ticks
lead, tail, cu_tail, simd_spread = [], [], [], []
for g in np.unique(wg):
    sel = wg == g
    cu_e = r1[sel].max()
    cu_tail.append((kend - cu_e) / 100)
    ends = []
    for s in range(4):
        ss = sel & (simd == s)
        if not ss.any():
            continue
        lead.append((first_rt[ss].min() - base) / 100)
        e = r1[ss].max()
        ends.append(e)
        tail.append((kend - e) / 100)
    simd_spread.append((max(ends) - min(ends)) / 100)
lead, tail = np.array(lead), np.array(tail)
span = (kend - base) / 100
print(f"span {span:.2f} us; per SIMD: lead-in (first task) mean {lead.mean():.2f} us, "
      f"tail (idle after its last wave) mean {tail.mean():.2f} us "
      f"= {100 * (lead.mean() + tail.mean()) / span:.1f} % of the span")
print(f"  CU tail (kernel end - CU end) mean {np.mean(cu_tail):.2f} us; SIMD end spread inside a CU "
      f"median {np.median(simd_spread):.2f} p90 {np.percentile(simd_spread, 90):.2f} us")
xcd = np.unique(wg) % 8
cu_e = np.array([r1[wg == g].max() for g in np.unique(wg)]) - base
for x in range(8):
    sx = np.isin(wg, np.unique(wg)[xcd == x])
    print(f"  XCD {x}: clock {np.median(clk[sx]):.3f} GHz, CU end median {np.median(cu_e[xcd == x]) / 100:.2f} "
          f"max {cu_e[xcd == x].max() / 100:.2f} us, tasks {ntask[sx].sum()}")

# Pruning launches: what a slot's refill costs the wave that does it (per
# refill, shader cycles): the wait for the item's DMA and the bound phase.
L.me_debug_wave_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
wbuf = np.zeros(8 << 14, np.uint64)
L.me_debug_wave_stamps(wbuf.ctypes.data, wbuf.size)
ws = wbuf.reshape(-1, 8)[:4096].astype(np.int64)
nref = ws[:, 2].sum()
if nref:
    print(f"refills {nref}: DMA wait mean {ws[:, 0].sum() / nref:.0f} cycles, stage-to-publish after it "
          f"(bound phase) mean {ws[:, 1].sum() / nref:.0f} cycles; spin per task mean {spin.sum() / max(ntask.sum(), 1):.0f}")
    # Executed wave-tasks (list read to key merge) by row-split class: run
    # whole, with 2 (7 rows a lane) and with 4 to 13 lanes per list entry (4 to 1
    # rows; ME_PRUNE_SPLIT=2: 4 lanes, 4 rows); word = count << 40 | cycles.
    for col, name in ((3, "whole"), (4, "2 lanes/entry"), (5, "4 or more lanes/entry")):
        cnt, cyc = (ws[:, col] >> 40).sum(), (ws[:, col] & ((1 << 40) - 1)).sum()
        print(f"executed wave-tasks {name}: {cnt}" + (f", mean {cyc / cnt:.0f} cycles" if cnt else ""))
    # The bound of a refill, split (g_bstamps, cycles per bounded item): cur q
    # and minlb init, step 2 per chunk, the fold column, step 3 with its wait
    # for the window DMA apart, step 4.
    if hasattr(L, "me_debug_bound_stamps"):
        L.me_debug_bound_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
        bbuf = np.zeros(16 << 14, np.uint64)
        L.me_debug_bound_stamps(bbuf.ctypes.data, bbuf.size)
        bsp = bbuf.reshape(-1, 16)[:4096].astype(np.int64).sum(axis=0)
        nbd, nch = max(bsp[6], 1), max(bsp[2], 1)
        print(f"bound split per bounded item ({bsp[6]} of {nref} refills): init {bsp[0] / nbd:.0f}, step 2 "
              f"{bsp[1] / nbd:.0f} ({bsp[1] / nch:.0f} per chunk, {bsp[2] / nbd:.2f} chunks), fold column {bsp[3] / nbd:.0f}, "
              f"window wait {bsp[7] / nbd:.0f}, step 3 {bsp[4] / nbd:.0f}, step 4 {bsp[5] / nbd:.0f}")
        # the head of the line: a slot's publish to the start of its item's first executed wave-task
        print(f"publish -> first executed task: mean {bsp[8] / max(bsp[9], 1):.0f} cycles ({bsp[9]} items)")
        # The chain kernel's pre-bound (words a build without it leaves 0): the
        # refills' last task done -> publish, the pre-bounds behind a publish,
        # and the post-bounds that found the slot's marker BUSY and waited.
        if bsp[14]:
            print(f"refill, last task done -> publish: mean {bsp[14] / nref:.0f} cycles ({nref} refills)")
            print(f"pre-bounds {bsp[13]}: mean {bsp[12] / max(bsp[13], 1):.0f} cycles; post-bounds that waited on BUSY "
                  f"{bsp[11]} of {nref} refills: mean {bsp[10] / max(bsp[11], 1):.0f} cycles a wait, "
                  f"{bsp[10] / nref:.0f} a refill")
        else:  # (the same interval from the timers every stamps build has)
            dr = ws[:, 7] & ((1 << 40) - 1)
            print(f"refill, decode + DMA wait + bound (last task done -> publish but for the records' write): "
                  f"mean {(dr.sum() + ws[:, 0].sum() + ws[:, 1].sum()) / nref:.0f} cycles ({nref} refills)")
    # Per XCD: the tile -> item decode (flow_item: the job lookup and the item's
    # geometry) where a wave advances to its next item and where the refill
    # names the item it stages, beside what a refill and a task wait for.
    # ws and the wave records are both indexed workgroup * 16 + wave.
    MASK = (1 << 40) - 1
    full = buf.reshape(-1, 8)[:4096].astype(np.int64)
    wxcd = (np.arange(4096) // 16) % 8
    print("  per XCD: decode cycles per item at the advance / at the refill; per refill DMA wait, bound; spin per task")
    for x in range(8):
        sx = (wxcd == x) & (full[:, 0] > 0)
        adv_n, adv_c = (ws[sx, 6] >> 40).sum(), (ws[sx, 6] & MASK).sum()
        ref_n, ref_c = (ws[sx, 7] >> 40).sum(), (ws[sx, 7] & MASK).sum()
        nr, nt = max(ws[sx, 2].sum(), 1), max(full[sx, 4].sum(), 1)
        print(f"  XCD {x}: advance {adv_c / max(adv_n, 1):.0f} ({adv_n} items), refill {ref_c / max(ref_n, 1):.0f} ({ref_n}); "
              f"DMA wait {ws[sx, 0].sum() / nr:.0f}, bound {ws[sx, 1].sum() / nr:.0f}; spin {full[sx, 3].sum() / nt:.0f}")
