"""A single search and a one-job list take one route (csrc/me_dispatch.cpp).

For thin cases of the dispatch table (tests/golden/plans/dispatch.json) whose
lists hold the leftover rules -- a partial right column, a bottom row that is
neither B nor B/2 high, a B/2 bottom row, for SAD and for SSD (where the 8x8
matrix-core kernel leaves the bottom row to the VALU route) -- the job runs
once through me_full_search_stripe_device and once as a one-job
me_search_stripes_device list: the records are bit-equal to each other and to
the oracle, and me_ctx_last_search_path reports the same family."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from motionestimation_amd import synth

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans", "dispatch.json")
# right column + odd bottom row; right column + B/2 bottom row; 8x8 odd and B/2 bottom rows
CASES = [f"{shape}_{cost}" for shape in ("87x53", "200x72", "64x43", "64x44") for cost in ("sad", "ssd")]


def _case(name):
    with open(FIXTURE) as f:
        return next(r for r in json.load(f)["records"] if r["name"] == name)


@pytest.mark.parametrize("name", CASES)
def test_stripe_call_equals_one_job_list(engine, name):
    import torch
    c = _case(name)
    w, h, pitch, blk, span = c["width"], c["height"], c["stride"], c["blk"], c["range"]
    cost = {0: "ssd", 1: "sad"}[c["cost"]]
    (r0, r1, ref_row0, cur_row0, _, _), = c["jobs"]
    nby, nbx = (h + blk - 1) // blk, (w + blk - 1) // blk
    assert (r0, r1, ref_row0, cur_row0) == (0, nby, 0, 0) and pitch >= w
    assert w % blk or h % blk  # a leftover rule applies
    ref, cur = synth.frame_pair(w, h, 5, 2, -3)
    omv, ocost, _ = O.full_search(ref, cur, blk, span, cost, threads=4)
    planes = []
    for a in (ref, cur):  # the table's pitch, any padding unlike the frame
        t = torch.full((h, pitch), 255, dtype=torch.uint8, device="cuda")
        t[:, :w] = torch.from_numpy(a).cuda()
        planes.append(t)
    rt, ct = planes
    got = []
    for how in ("stripe", "list"):
        mv = torch.full((nby * nbx, 2), -9, dtype=torch.int16, device="cuda")
        co = torch.full((nby * nbx,), -1, dtype=torch.int32, device="cuda")
        if how == "stripe":
            engine.search_stripe_device(rt, 0, ct, 0, w, h, blk, span, cost, 0, nby, mv, co, stride=pitch)
        else:
            engine.search_stripes_device(w, h, blk, span, cost, [(rt, 0, ct, 0, 0, nby, mv, co)],
                                         stride=pitch)
        torch.cuda.synchronize()
        engine.device_check()
        got.append((mv.cpu().numpy(), co.cpu().numpy().view(np.uint32), engine.last_search_path()))
    for mv, co, _ in got:
        np.testing.assert_array_equal(mv, omv)
        np.testing.assert_array_equal(co, ocost)
    assert got[0][2] == got[1][2] != "none"
