"""The VALU launch planners give the plans they gave before they moved.

tests/golden/plans/valu_plans.json holds, for a table of shapes that reaches
every rule of plan_fast and plan_flow (csrc/me_valu_plan.cpp), the plans the
commit before the move computed inside me_kernels.hip (256 CUs, default
tuning).  oracle/plan_dump.cc links the planner file alone, reads the shapes
back and prints today's plans; every field of every record must be equal.  No
GPU and no library load."""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle")
FIXTURE = os.path.join(REPO, "tests", "golden", "plans", "valu_plans.json")


def _plans():
    subprocess.run(["make", "-s", "-C", ORACLE, "plan_dump"], check=True, timeout=300)
    r = subprocess.run([os.path.join(ORACLE, "plan_dump"), FIXTURE], capture_output=True,
                       text=True, timeout=60, check=True)
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_plans_equal_the_recorded_ones():
    with open(FIXTURE) as f:
        want = json.load(f)["records"]
    got = _plans()
    assert len(got) == len(want) > 100
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, f"{len(bad)} plans differ, first: recorded {bad[0][0]} now {bad[0][1]}"


def test_fixture_holds_the_plans_the_design_names():
    """DESIGN.md ties measured numbers to these plans; the table must keep their shapes."""
    with open(FIXTURE) as f:
        recs = json.load(f)["records"]

    def plan(planner, width, blk, rng, cost, rows):
        hit = [r for r in recs if (r["planner"], r["width"], r["blk"], r["range"], r["cost"],
                                   r["rows"], r["align"]) == (planner, width, blk, rng, cost, rows, 7)]
        assert len(hit) == 1, (planner, width, blk, rng, cost, rows)
        return hit[0]

    SAD = 1
    p = plan("flow", 1920, 16, 32, SAD, 68)
    assert p["ok"] and (p["tb"], p["pitch"]) == (4, 144)
    p = plan("fast", 3840, 16, 64, SAD, 135)
    assert p["ok"] and (p["K"], p["tb"], p["pitch"]) == (13, 8, 272)
    p = plan("fast", 7680, 8, 128, SAD, 540)
    assert p["ok"] and (p["K"], p["tb"], p["pitch"]) == (26, 8, 336)
    p = plan("fast", 1920, 16, 32, SAD, 8)
    assert p["ok"] and (p["K"], p["tb"]) == (5, 1)
    # the B = 8 arm of the fold rule: S % 8 == 4 and the fold taken
    assert plan("fast", 1920, 8, 28, SAD, 135)["fold"] == 1
    assert plan("fast", 1920, 8, 36, SAD, 135)["fold"] == 1
    # refused shapes stay refused
    assert not plan("flow", 1920, 16, 48, SAD, 68)["ok"]
    assert not plan("fast", 1920, 16, 256, SAD, 68)["ok"]
    assert not plan("fast", 1920, 32, 16, SAD, 68)["ok"]
