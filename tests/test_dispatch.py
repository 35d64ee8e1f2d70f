"""The search dispatcher covers every block once and plans what it planned.

csrc/me_dispatch.cpp decides which kernel family searches which blocks of
which job; launch_jobs (me_kernels.hip) only walks its list.
oracle/dispatch_dump.cc links it with the two planner files alone and prints,
for the cases of tests/golden/plans/dispatch.json (256 CUs, default tuning),
each launch's kind, job range and per-job block rectangle.  No GPU and no
library load.

The recorded lists are the new code's: the commit before it had no list to
print.  They were recorded only after a kernel trace of the cases' searches
on an MI355X (through the device entry points, once on the parent build and
once on this one) gave the same sequence of kernel names, grids, workgroup
sizes and LDS sizes.  Traced: every case but the two with a "scratch" >= 0
(a context sizes its own scratch) and 87x53_sad_x3_empty_bottom, where the
parent launched the generic kernel for the bottom row of the empty job
[nby, nby) and wrote its records before the job's arrays; the dispatcher
drops that launch."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle")
FIXTURE = os.path.join(REPO, "tests", "golden", "plans", "dispatch.json")
MAX_JOBS = 32
SSD, SAD = 0, 1


@pytest.fixture(scope="module")
def lists():
    subprocess.run(["make", "-s", "-C", ORACLE, "dispatch_dump"], check=True, timeout=300)
    r = subprocess.run([os.path.join(ORACLE, "dispatch_dump"), FIXTURE], capture_output=True,
                       text=True, timeout=60, check=True)
    return {rec["name"]: rec for rec in map(json.loads, r.stdout.splitlines())}


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)["records"]


def _dims(case):
    b = case["blk"]
    return (case["height"] + b - 1) // b, (case["width"] + b - 1) // b


def test_every_block_is_searched_exactly_once(lists):
    """Paint each launch's rectangles into a grid per job: the rows [r0, r1) of the
    job, every column, must hold exactly 1 and nothing else may be painted."""
    assert len(lists) == len(_recorded()) > 100
    for name, case in lists.items():
        nby, nbx = _dims(case)
        grids = [[[0] * nbx for _ in range(nby)] for _ in case["jobs"]]
        for l in case["launches"]:
            assert len(l["rects"]) == l["njobs"] <= MAX_JOBS, name
            assert l["kind"] in ("ITEM", "FLOW", "MFMA") or l["njobs"] == 1, (name, l)
            for j, (r0, r1, bx0, bx1) in enumerate(l["rects"], start=l["job0"]):
                assert 0 <= bx0 <= bx1 <= nbx, (name, l)
                if l["kind"] == "MFMA":  # its kernels cover the plan's rows and columns
                    assert (l["row0"], l["row0"] + l["nrows"], 0, l["nbx"]) == (r0, r1, bx0, bx1), (name, l)
                assert r1 <= r0 or 0 <= r0 < r1 <= nby, (name, l)
                for r in range(r0, r1):
                    for bx in range(bx0, bx1):
                        grids[j][r][bx] += 1
        for j, (r0, r1, *_) in enumerate(case["jobs"]):
            want = [[1 if r0 <= r < r1 else 0] * nbx for r in range(nby)]
            assert grids[j] == want, f"{name}: job {j} rows [{r0}, {r1}) painted {grids[j]}"


def test_lists_equal_the_recorded_ones(lists):
    want = _recorded()
    bad = [(w, lists.get(w["name"])) for w in want if w != lists.get(w["name"])]
    assert not bad, f"{len(bad)} lists differ, first: recorded {bad[0][0]} now {bad[0][1]}"


def _kinds(case):
    return [l["kind"] for l in case["launches"]]


def _qsad(case):
    return [l for l in case["launches"] if l["kind"] in ("ITEM", "FLOW")]


def _generic(case, right):
    """Generic launches beside a qsad or MFMA launch: the partial right column
    (right) or rows below it from column 0."""
    if not set(_kinds(case)) & {"ITEM", "FLOW", "MFMA"}:
        return []
    return [l for l in case["launches"] if l["kind"] == "GENERIC" and (l["rects"][0][2] > 0) == right]


def _bottom_height(case):
    return case["height"] - (_dims(case)[0] - 1) * case["blk"]


def _takes_bottom(case, launches):
    nby = _dims(case)[0]
    return any(r0 < nby == r1 for l in launches for r0, r1, *_ in l["rects"])


def _mfma_rest(case):
    """The 8x8 MFMA kernel stops above the partial bottom row, which another launch takes."""
    nby = _dims(case)[0]
    mfma = [l for l in case["launches"] if l["kind"] == "MFMA"]
    rest = [l for l in case["launches"] if l["kind"] != "MFMA"]
    return (case["blk"] == 8 and len(mfma) == 1 and mfma[0]["rects"][0][1] == nby - 1 and
            _takes_bottom(case, rest))


def _batch_then_per_job(case):
    return len(case["jobs"]) > 1 and all(l["njobs"] == 1 for l in case["launches"]) and "ITEM" in _kinds(case)


def _empty_job_in_batch(case):
    return (any(r1 <= r0 for r0, r1, *_ in case["jobs"]) and
            any(l["njobs"] == len(case["jobs"]) > 1 for l in case["launches"]))


# What the table must reach: rule -> (a case that reaches it, the evidence in its list).
REACH = {
    "kind GENERIC": ("200x72_b32_sad", lambda c: "GENERIC" in _kinds(c)),
    "kind ITEM": ("4k_sad_x1", lambda c: _kinds(c) == ["ITEM"]),
    "kind FLOW": ("1080p_sad_x1", lambda c: _kinds(c) == ["FLOW"]),
    "kind MFMA": ("1080p_ssd_x1", lambda c: _kinds(c) == ["MFMA"]),
    "kind SSIM": ("352x288_ssim_x3", lambda c: _kinds(c) == ["SSIM", "SSIM"]),
    "generic right column after a qsad launch": ("87x53_sad", lambda c: _qsad(c) and _generic(c, True)),
    "generic right column after an MFMA launch": (
        "87x53_ssd", lambda c: _kinds(c) == ["MFMA", "GENERIC"] and _generic(c, True)),
    "generic bottom row": (
        "87x53_sad", lambda c: _bottom_height(c) not in (c["blk"], c["blk"] // 2) and
        not _takes_bottom(c, _qsad(c)) and _takes_bottom(c, _generic(c, False))),
    "B/2 bottom row kept by the flow kernel": (
        "1080p_sad_x1", lambda c: _bottom_height(c) == c["blk"] // 2 and _takes_bottom(c, _qsad(c))),
    "B/2 bottom row kept by the item kernel": (
        "200x72_sad", lambda c: _bottom_height(c) == c["blk"] // 2 and _kinds(c)[0] == "ITEM" and
        _takes_bottom(c, _qsad(c))),
    "MFMA rest row to the item kernel": ("64x44_ssd", lambda c: _mfma_rest(c) and "ITEM" in _kinds(c)),
    "MFMA rest row to the generic kernel": (
        "64x43_ssd", lambda c: _mfma_rest(c) and _takes_bottom(c, _generic(c, False))),
    "MFMA batch cut by the scratch given": (
        "1080p_ssd_x8_path4_scratch3",
        lambda c: c["scratch"] >= 0 and [l["njobs"] for l in c["launches"]] == [3, 3, 2] and
        set(_kinds(c)) == {"MFMA"}),
    "flow batch split into several launches": (
        "1080p_sad_x33", lambda c: [(l["kind"], l["njobs"]) for l in c["launches"]] == [("FLOW", 32), ("FLOW", 1)]),
    "item batch of more than MAX_JOBS jobs": (
        "4k_sad_x33", lambda c: [(l["kind"], l["njobs"]) for l in c["launches"]] == [("ITEM", 32), ("ITEM", 1)]),
    "batch refused for mixed alignment, then job by job": ("4k_sad_x2_mixed_align", _batch_then_per_job),
    "empty job inside a batch": ("1080p_sad_x3_empty", _empty_job_in_batch),
    "empty job at the frame's bottom inside a batch": ("87x53_sad_x3_empty_bottom", _empty_job_in_batch),
    "ME_PATH_VALU sends SSD to the item kernel": (
        "1080p_ssd_x1_path1", lambda c: c["path"] == 1 and c["cost"] == SSD and _kinds(c) == ["ITEM"]),
    "whole-job generic fallback": (
        "200x72_b32_sad", lambda c: _kinds(c) == ["GENERIC"] and
        c["launches"][0]["rects"] == [[0, _dims(c)[0], 0, _dims(c)[1]]]),
    "stripe with r0 > 0 and ref_row0 > 0": (
        "1080p_sad_stripe3", lambda c: c["jobs"][0][0] > 0 and c["jobs"][0][2] > 0 and c["launches"]),
}


@pytest.mark.parametrize("rule", sorted(REACH))
def test_table_reaches(lists, rule):
    name, evidence = REACH[rule]
    assert name in lists, f"no case {name} for: {rule}"
    assert evidence(lists[name]), f"{name} does not reach: {rule}: {lists[name]['launches']}"


def test_table_reaches_every_kind_path_and_bench_shape(lists):
    kinds = {k for c in lists.values() for k in _kinds(c)}
    assert kinds == {"GENERIC", "ITEM", "FLOW", "MFMA", "SSIM"}
    assert {c["path"] for c in lists.values()} == {0, 1, 2, 3, 4}
    for shape in ("1080p", "4k", "8k8"):
        for cost in ("sad", "ssd"):
            for n in (1, 2, 8, 33):
                assert len(lists[f"{shape}_{cost}_x{n}"]["jobs"]) == n
