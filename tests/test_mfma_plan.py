"""The matrix-core SSD planners give the plans they gave before they moved.

tests/golden/plans/mfma_plans.json holds, for a table of shapes that reaches
every rule of the single-search planner, plan_bw and the batch planner
(csrc/me_mfma_plan.cpp), what the commit before the move planned inside
me_mfma.hip and me_band.hip (256 CUs, default tuning, every kernel path); each
record's note says which rule it is there for.  oracle/mfma_plan_dump.cc
links the planner file alone, reads the shapes back and prints today's plans;
every field of every record must be equal.  No GPU and no library load."""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle")
FIXTURE = os.path.join(REPO, "tests", "golden", "plans", "mfma_plans.json")


def _records():
    with open(FIXTURE) as f:
        return json.load(f)["records"]


def test_plans_equal_the_recorded_ones():
    subprocess.run(["make", "-s", "-C", ORACLE, "mfma_plan_dump"], check=True, timeout=300)
    r = subprocess.run([os.path.join(ORACLE, "mfma_plan_dump"), FIXTURE], capture_output=True,
                       text=True, timeout=60, check=True)
    got = [json.loads(line) for line in r.stdout.splitlines()]
    want = _records()
    assert len(got) == len(want) > 100
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, f"{len(bad)} plans differ, first: recorded {bad[0][0]} now {bad[0][1]}"


def _plan(recs, width, height, rng, path, blk=16):
    """The whole-frame record of this shape (SSD, everything 16-byte aligned, merge buffers present)."""
    hit = [r for r in recs if (r["width"], r["height"], r["stride"], r["blk"], r["range"], r["path"],
                               r["align"], r["cost"], r["r0"]) == (width, height, width, blk, rng, path, 7, 0, 0)
           and r["r1"] == (height + blk - 1) // blk and r["merge"] > 0]
    assert hit and all(h["g"] == hit[0]["g"] for h in hit), (width, height, rng, path)
    return hit[0]


def test_fixture_holds_the_plans_the_design_names():
    """DESIGN.md ties measured numbers to these plans; the table must keep their shapes."""
    recs = _records()
    # 1080p +-32, one frame per call: the band walk, 8 segments of 9 rows in one
    # round of workgroups, the partial bottom row inside the walk, no scratch
    for path in (0, 3):
        p = _plan(recs, 1920, 1080, 32, path)
        g = p["g"]
        assert p["ok"] and (g["bw"], g["bw_segs"], g["bw_seg_rows"], g["bw_cols"]) == (1, 8, 9, 4)
        assert g["bw_hb"] == 3 and p["scratch"] == 0 and p["plan_bw"][0]["one_round"]
    # 4K +-64, one frame per call (the band-walk row of DESIGN.md's SSD table):
    # 2 segments of 68 rows, 240 workgroups, still one round on 256 CUs
    for path in (0, 3):
        g = _plan(recs, 3840, 2160, 64, path)["g"]
        assert (g["bw"], g["bw_segs"], g["bw_seg_rows"], g["bw_strips"]) == (1, 2, 68, 120)
    # the automatic path declines a walk of several segments in several rounds
    # (the prepass + block-major pair runs); the lean path takes that walk
    p = _plan(recs, 5440, 2160, 64, 0)
    assert (p["g"]["bw"], p["g"]["bm"], p["g"]["bmv"]) == (0, 1, 0) and p["scratch"] > 0
    assert (p["plan_bw"][0]["bw_segs"], p["plan_bw"][0]["one_round"]) == (3, False)
    assert _plan(recs, 5440, 2160, 64, 3)["g"]["bw_segs"] == 3
    # ... whose batches take it whole (per-XCD tail split): the scratch of one search
    assert p["batch_scratch"] == [p["scratch"]] * 5
    # ME_PATH_MFMA_PREPASS: the pair, its batches sized by the 1 GiB cap (25 4K jobs)
    for w, h, s in ((1920, 1080, 32), (3840, 2160, 64)):
        p = _plan(recs, w, h, s, 4)
        assert (p["g"]["bw"], p["g"]["bm"], p["g"]["bmv"]) == (0, 1, 0) and p["scratch"] > 0
    stride = (p["scratch"] + 255) & ~255
    assert p["batch_scratch"] == [2 * stride, 8 * stride, 16 * stride, 25 * stride, 25 * stride]
    # the 8K 8x8 bench shape: the 8x8 tile kernel, S2 plane only
    p = _plan(recs, 7680, 4320, 128, 0, blk=8)
    assert p["ok"] and (p["g"]["km"], p["g"]["rp_bytes"], p["g"]["bm"]) == (3, 0, 0)
    # ME_PATH_VALU refuses everything
    assert not any(r["ok"] for r in recs if r["path"] == 1)


def test_fixture_reaches_every_kernel_instance_and_rule():
    recs = _records()
    ok = [r for r in recs if r["ok"]]
    assert {r["path"] for r in recs} == {0, 1, 2, 3, 4}
    assert {r["align"] & 1 for r in recs} == {0, 1} and {r["align"] for r in ok} >= {1, 3, 5, 7}
    # the six band-walk instances launch_bw dispatches, tail split on and off,
    # the partial row inside the walk and refused for LDS
    bw = [(r, b) for r in ok for b in r.get("plan_bw", []) if b["ok"]]
    assert {(b["bw_cols"], b["bw_lp"]) for _, b in bw} == {(6, 160), (4, 160), (3, 160), (3, 224),
                                                          (2, 160), (2, 224)}
    assert {b["bw_xt"] for _, b in bw} == {0, 1}
    assert {b["bw_hb"] > 0 for r, b in bw if r["g"]["hb_row"] >= 0} == {False, True}
    # the four tile-kernel instances' parameters, ngx up to 4, both window pitches, both bmv_r
    tiles = [r["g"] for r in ok if r["blk"] == 16 and not r["g"]["bm"]]
    assert {(g["ngxw"], g["km"]) for g in tiles} == {(1, 2), (1, 3), (2, 2), (2, 3)}
    assert {g["ngx"] for g in tiles} == {1, 2, 3, 4}
    assert {r["g"]["bm_lp"] for r in ok if r["g"]["bm"]} == {288, 544}
    assert {(r["g"]["bmv"], r["g"]["bmv_r"]) for r in ok} >= {(1, 1), (1, 2), (0, 1), (0, 2)}
    # stripes clamped on neither side, a partial bottom row with both block sizes
    assert any(r["g"]["ya0"] > 0 and r["g"]["ya0"] + r["g"]["rp_rows"] < r["height"] for r in ok)
    assert any(r["blk"] == 16 and r["g"]["hb_row"] >= 0 for r in ok)
    assert any(r["blk"] == 8 and r["g"]["nrows"] < r["r1"] - r["r0"] for r in ok)
