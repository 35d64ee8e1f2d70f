"""The lattice cases of tests/tie_cases.py are adversarial for the tie rule: on
the CPU, from the census alone, before a GPU sees them.

Per case: most full blocks have a tied minimum, for most of those a (dx, dy)
key order or a last-wins rule would pick another vector than the raster-first
one, the tied pairs of lat_320x136 and lat_1024x512 reach every seam of the
flow kernel's geometry, the oracle (tests/oracle_lib.py) returns the census's
raster-first minimiser and cost, and the oracle's work stays inside the budget
valu_envelope_cases.py documents.  The port of the row split's arithmetic is
pinned against bin/flow_split_dump as tests/test_flow_split_rule.py does.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rd_ref
import tie_cases as T

NT = min(16, os.cpu_count() or 1)
DUMP = os.path.join(O.REPO, "bin", "flow_split_dump")


def test_split_port_is_the_headers_rule():
    subprocess.run(["make", "-s", "-C", O.REPO, "-f", "tools.mk", "bin/flow_split_dump"], check=True, timeout=300)
    r = subprocess.run([DUMP], capture_output=True, text=True, timeout=60, check=True)
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    assert [d["n"] for d in rows] == list(range(1, 65))
    for d in rows:
        n, R = d["n"], T.split_rows(d["n"])
        assert (R, T.split_parts(R)) == (d["rows"], d["parts"]), n
        assert [T.split_lane(R, lane, n) for lane in range(64)] == d["lanes"], n
    assert {d["rows"] for d in rows} == set(T.SPLIT_ROWS) | {T.K}


def test_pair_labels_on_hand_made_pairs():
    L = T.pair_labels
    some = {"split_1", "split_2", "split_3", "split_4"}
    assert L((-32, -32), (-29, -32)) == {"same_row"}
    assert L((-31, -32), (-32, -27)) == some  # rows 0 and 5: both in part 0 of R = 7
    assert L((-31, -30), (-32, -25)) == some | {"split_7"}  # rows 2 and 7
    assert L((-31, -20), (-32, -19)) == {"chunks"}  # row 12 of chunk 0, row 0 of chunk 1
    assert L((5, -32), (-4, -27)) == {"groups"}
    assert L((-4, -32), (5, -27)) == set()  # another group, but dx_first < dx_other
    assert L((32, 0), (-32, 1)) == {"fold", "wrap", "groups"}
    assert L((-5, -3), (0, 0)) == {"seed_later"} and L((0, 0), (17, 29)) == {"chunks", "seed_earlier"}
    # the fold candidate of row j sits in the lane-task of group j, part 0 of a split
    assert T.lane_task((32, -32 + 6)) == (0, 6, 6, True) and T.lane_task((-32 + 4 * 6, -32 + 6)) == (0, 6, 6, False)
    assert L((-8, -26), (32, -26)) == some | {"same_row", "fold"}  # row 6 is in both parts of R = 7


def test_shapes_qualify_for_the_flow_plan():
    """S = 32, B = 16, width % 64 == 0 (4-block tiles, 16-byte aligned rows), 512 tiles or more."""
    for name in T.FLOW_CASES:
        c = T.CASES[name]
        assert c.width % 64 == 0 and len(c.frames) * (c.width // 64) * -(-c.height // T.B) >= 512, name
    assert len(T.CASES["lat_1024x512"].frames) == 1  # a single job: no box-sum planes
    assert len(T.CASES["lat_320x136"].frames) == 20 and 136 % 16 == 8  # the h = 8 bottom row
    # every dy window of lat_256x64 is clamped
    assert not T.case_census("lat_256x64").unclamped.any()
    c = T.CASES["lat_small"]
    assert c.width % 4 == 0 and c.width % 16 and c.height % 16  # fast partition / rate kernels with a generic rim


@pytest.mark.parametrize("name", list(T.CASES))
def test_blocks_tie_and_the_order_matters(name):
    n, tied, dxdy, last = T.tie_stats(T.case_census(name))
    print(f"{name}: {n} full blocks, tied {tied} ({100 * tied / n:.1f} %), first != (dx, dy)-first {dxdy} "
          f"({100 * dxdy / tied:.1f} % of tied), first != last {last} ({100 * last / tied:.1f} %)")
    assert tied >= 0.6 * n, (name, tied, n)
    assert 2 * dxdy >= tied, (name, dxdy, tied)
    assert 2 * last >= tied, (name, last, tied)


def test_pair_classes_reach_every_seam():
    total = {}
    for name in ("lat_320x136", "lat_1024x512"):
        pc = T.pair_classes(T.case_census(name))
        print(name, "unclamped blocks", int(T.case_census(name).unclamped.sum()), "per frame;",
              {k: pc.get(k, 0) for k in T.PAIR_CLASSES})
        for k, v in pc.items():
            total[k] = total.get(k, 0) + v
    for k in T.PAIR_CLASSES:  # six classes: 2 for every R, 5 with the wrap pair, 6 in both orders
        assert total.get(k, 0) > 0, (k, total)


@pytest.mark.parametrize("name", list(T.CASES))
def test_oracle_returns_the_raster_first_minimiser(name):
    ref, cur = T.frames(name)
    cen = T.case_census(name)
    F, h, w = ref.shape
    nby, nbx = h // T.B, w // T.B
    picks = {"lat_320x136": (13, 14), "lat_256x64": (5, 30)}.get(name, (0, F - 1))  # (the wrap and the defect frame)
    for f in sorted(set(picks)):
        mv, co, _ = O.full_search(ref[f], cur[f], T.B, T.S, "sad", threads=NT)
        nbx_all = -(-w // T.B)
        mv = mv.reshape(-1, nbx_all, 2)[:nby, :nbx]
        co = co.reshape(-1, nbx_all)[:nby, :nbx]
        np.testing.assert_array_equal(co, cen.cmin[f], err_msg=f"{name} frame {f}")
        np.testing.assert_array_equal(mv, cen.first[f], err_msg=f"{name} frame {f}")


@pytest.mark.parametrize("name", list(T.CASES))
def test_oracle_budget(name):
    cost = T.oracle_cost(T.CASES[name])
    print(f"{name}: {cost:.3g} 16x16 candidate equivalents")
    assert cost <= T.ORACLE_BUDGET


@pytest.mark.parametrize("blk,span,frames_", T.RD_SHAPES)
def test_midpoint_predictor_keeps_j_ties(blk, span, frames_):
    """With p = 2 (d1 + d2) the two tied minimisers of SAD have equal rates, and
    at least half of the blocks keep a tie of J = SAD + lambda R at its minimum."""
    ref, cur = T.frames("lat_small")
    h, w = ref.shape[1:]
    for lam in T.RD_LAMBDAS:
        tied = total = 0
        for f in frames_:
            cen = T.census(ref[f], cur[f], blk, span)
            pred = T.midpoint_pred(cen, 0, w, h, blk)
            t = T.j_ties(rd_ref.sad_table(ref[f], cur[f], blk, span), lam, pred)
            tied, total = tied + int(t.sum()), total + t.size
            p = pred.reshape(-(-h // blk), -(-w // blk), 2)[:h // blk, :w // blk].astype(np.int64)
            d1 = cen.first[0]
            for by, bx in zip(*np.nonzero(cen.nmin[0] > 1)):  # d2 = p / 2 - d1 is a minimiser, with d1's rate
                d2 = p[by, bx] // 2 - d1[by, bx]
                assert tuple(d2) in T.minimisers(cen, 0, by, bx)[1:]
                assert (rd_ref.bits(4 * d1[by, bx] - p[by, bx]) == rd_ref.bits(4 * d2 - p[by, bx])).all()
        print(f"B{blk} S{span} lambda {lam}: J tied in {tied} of {total} blocks")
        assert 2 * tied >= total, (blk, span, lam, tied, total)
