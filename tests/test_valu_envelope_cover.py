"""The envelope table reaches every instance and plan feature it claims (CPU).

tests/valu_envelope_cases.py lists the shapes tests/test_gpu_valu_envelope.py
searches on the GPU.  plan_fast is pure host C++ (csrc/me_valu_plan.cpp), so
which me_fast_kernel instance and which plan features each shape reaches is
decided here, without a GPU: oracle/plan_dump plans the table's shapes (256
CUs, default tuning, as the library does on an MI355X), launch_fast's
ME_FAST_CASE lines give the compiled instances, and every instance and
feature must be reached by at least one case -- an instance added to
launch_fast without a case fails this test.  The content kinds are checked
with the oracle alone: the planted pairs of two_copies win at their first
copy with cost 0, antidiag separates raster-first from column-first tie
order, sat gives all-maximum costs.  No GPU and no library load."""
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import valu_envelope_cases as V
from valu_envelope_cases import CASES, SAD, SSD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle")
KERNELS = os.path.join(REPO, "motionestimation_amd", "csrc", "me_kernels.hip")
NT = min(16, os.cpu_count() or 1)
FAST = [(SAD, 16), (SAD, 8), (SSD, 16), (SSD, 8)]


def _planned(c):
    """Does the library ask plan_fast about this case (and run what it answers)?"""
    return c.expect_path == "valu"


@functools.lru_cache(maxsize=None)
def _plans(tmpdir):
    """{case name: plan_dump record} for the table, planned as the dispatcher
    plans a whole frame: rows = every block row, the class bits the item
    planner reads."""
    subprocess.run(["make", "-s", "-C", ORACLE, "plan_dump"], check=True, timeout=300)
    path = os.path.join(tmpdir, "envelope_shapes.json")
    with open(path, "w") as f:
        for c in CASES:
            f.write('{"planner":"fast","width":%d,"height":%d,"stride":%d,"blk":%d,"range":%d,'
                    '"cost":%d,"rows":%d,"align":%d}\n'
                    % (c.width, c.height, c.stride, c.blk, c.range, c.cost, c.nby,
                       c.align & (V.ALIGN_4 | V.ALIGN_REF16)))
    r = subprocess.run([os.path.join(ORACLE, "plan_dump"), path], capture_output=True, text=True,
                       timeout=120, check=True)
    recs = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(recs) == len(CASES)
    for c, p in zip(CASES, recs):
        assert (p["width"], p["height"], p["blk"], p["range"], p["cost"]) == (
            c.width, c.height, c.blk, c.range, c.cost)
    return {c.name: p for c, p in zip(CASES, recs)}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _plans(str(tmp_path_factory.mktemp("envelope")))


def _instances():
    """The (cost, B, K, compiled pitch) instances launch_fast dispatches to."""
    with open(KERNELS) as f:
        src = f.read()
    body = src[src.index("static hipError_t launch_fast("):]
    body = body[:body.index("#undef ME_FAST_CASE")]
    inst = set()
    for m in re.finditer(r"ME_FAST_CASE(_P)?\(\s*COST_(SAD|SSD)\s*,\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(\d+)\s*)?\)", body):
        assert (m.group(1) is None) == (m.group(5) is None), m.group(0)
        inst.add((SAD if m.group(2) == "SAD" else SSD, int(m.group(3)), int(m.group(4)),
                  int(m.group(5) or 0)))
    # every use of the macros parsed (the two #define lines are not uses)
    uses = len(re.findall(r"ME_FAST_CASE(?:_P)?\(\s*COST_", body))
    assert uses == len(inst) >= 17, (uses, sorted(inst))
    return inst


def _instance_of(c, p, compiled):
    """The instance launch_fast picks for plan p: the compiled-pitch one where the pitch matches."""
    pp = compiled.get((c.cost, c.blk, p["K"]), 0)
    return (c.cost, c.blk, p["K"], pp if pp == p["pitch"] else 0)


def _features(c, p):
    """The plan features of the issue's list that case c reaches with plan p."""
    fam = (c.cost, c.blk)
    if not p["ok"]:
        f = {("refused", fam)}
        if c.range == 0:
            f.add("refused S=0")
        if c.range == 256:
            f.add(("refused S=256", fam))
        if c.blk not in (8, 16):
            f.add(("refused B", c.cost))
        if fam == (SAD, 16) and 1 <= c.range <= 255:
            f.add("K=5 refused")  # a small search whose K = 5 tile leaves QSAD_LDS_BUDGET
        return f
    B = c.blk
    f = {(fam, "multi-pass" if p["cpp"] < p["chunks"] else "single-pass"),
         (fam, "aligned", p["aligned"]), (fam, "tile16", p["tile16"]),
         (fam, "tb=1" if p["tb"] == 1 else "tb>1")}
    if p["tb"] > 1 and p["nbx_full"] % p["tb"]:
        f.add((fam, "short last tile"))
    if c.height % B == B // 2:
        f.add((fam, "H%B=B/2"))
    elif c.height % B:
        f.add((fam, "H%B other"))
    if c.width % B:
        f.add((fam, "W%B!=0"))
    if c.cost == SAD:
        f.add((fam, "fold", p["fold"]))
        if not p["fold"]:
            f.add((fam, "unfolded S%4", c.range % 4))
        if p["K"] == 5:
            f.add("K=5")
    return f


def test_table_is_well_formed():
    for c in CASES:
        assert c.stride >= c.width and 1 <= c.blk <= 64 and 0 <= c.range <= 1024, c.name
        assert c.path in ("auto", "valu") and c.cost in (SAD, SSD), c.name
        assert c.kind in ("far_shift", "two_copies", "antidiag", "sat"), c.name
        assert c.align == V.align_class(c.stride, V.BASE_ALIGN + c.ref_off, V.BASE_ALIGN + c.cur_off)
        n = V.candidate_count(c.width, c.height, c.blk, c.range)
        assert n == O.candidate_count(c.width, c.height, c.blk, c.range), c.name
        assert V.oracle_cost(c) <= V.ORACLE_BUDGET, (c.name, V.oracle_cost(c))
        # thin frames: an unclipped window along one axis for at least one block
        if c.blk in (8, 16):
            assert max(c.width, c.height) >= 3 * c.blk + 2 * c.range, c.name
    # both orientations
    assert any(c.width > 2 * c.height for c in CASES) and any(c.height > 2 * c.width for c in CASES)


def test_recorded_plans_are_todays(plans):
    """K and cpp in the table (the two_copies content reads them) are the plan's."""
    for c in CASES:
        p = plans[c.name]
        if _planned(c):
            want = (p["K"], p["cpp"]) if p["ok"] else (None, None)
            assert (c.K, c.cpp) == want, (c.name, (c.K, c.cpp), want)
        else:
            assert (c.K, c.cpp) == (None, None), c.name


def test_every_instance_is_reached(plans):
    inst = _instances()
    compiled = {(co, b, k): pp for (co, b, k, pp) in inst if pp}
    hit = {}
    for c in CASES:
        p = plans[c.name]
        if _planned(c) and p["ok"]:
            i = _instance_of(c, p, compiled)
            assert i in inst, f"{c.name}: plan {i} has no compiled instance"
            hit.setdefault(i, []).append(c)
    missing = sorted(inst - set(hit))
    assert not missing, f"me_fast_kernel instances without an envelope case: {missing}"
    # ... each with a planted tie pair and with winners at the window's extremes
    for i, cs in sorted(hit.items()):
        kinds = {c.kind for c in cs}
        assert {"two_copies", "far_shift"} <= kinds, (i, sorted(kinds))


def test_every_plan_feature_is_reached(plans):
    got = set()
    for c in CASES:
        if _planned(c):
            got |= _features(c, plans[c.name])
    want = set()
    for fam in FAST:
        want |= {(fam, "single-pass"), (fam, "multi-pass"), (fam, "aligned", 0), (fam, "aligned", 1),
                 (fam, "tile16", 0), (fam, "tile16", 1), (fam, "tb=1"), (fam, "tb>1"),
                 (fam, "short last tile"), (fam, "H%B=B/2"), (fam, "H%B other"), (fam, "W%B!=0"),
                 ("refused S=256", fam)}
        if fam[0] == SAD:
            want |= {(fam, "fold", 0), (fam, "fold", 1)}
            want |= {(fam, "unfolded S%4", m) for m in range(4)}
    want |= {"K=5", "K=5 refused", "refused S=0", ("refused B", SAD), ("refused B", SSD)}
    assert not (want - got), f"plan features no case reaches: {sorted(map(str, want - got))}"


def test_ranges_and_block_sizes_of_the_issue():
    have = {(c.cost, c.blk, c.range, c.path) for c in CASES}
    for s in (193, 224, 255):
        assert (SSD, 16, s, "auto") in have
    for s in (129, 200, 256, 600, 1024):
        assert (SSD, 8, s, "auto") in have
    for s in (256, 257, 600, 1024):
        for b in (8, 16):
            assert (SAD, b, s, "auto") in have
    for b in (33, 48, 63, 64):
        for cost in (SAD, SSD):
            assert any(c.cost == cost and c.blk == b and c.width % b and c.height % b for c in CASES)
    for s in (87, 88):
        assert any(c.blk == 64 and c.range == s for c in CASES)
    for s in (115, 116):  # the generic kernel takes the partial right column and bottom row
        assert any(c.blk == 16 and c.range == s and c.cost == SAD and c.width % 16
                   and c.height % 16 not in (0, 8) for c in CASES)
    # |dx| = S is reachable for some block of the long-range cases
    for c in CASES:
        if c.range in (600, 1024):
            assert max(c.width, c.height) >= c.range + c.blk, c.name
    # the 8x8 matrix-core kernel merges 33 column groups per tile at S = 1024
    c = V.BY_NAME["ssd8_s1024_mfma"]
    assert (min(24 + 2 * c.range + 1, c.width - 7) + 63) // 64 == 33
    assert all(c.height % 8 == 0 for c in CASES if c.expect_path == "mfma_8x8")


# ------------------------------------------------------------ content, by the oracle
@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = V.BY_NAME[name]
    ref, cur, planted = V.frames(c)
    mv, cost, _ = O.full_search(ref, cur, c.blk, c.range, "sad" if c.cost == SAD else "mse", threads=NT)
    return ref, cur, planted, mv, cost


def _pass_of(c, dy):
    return ((dy + c.range) // c.K) // c.cpp


def test_two_copies_plant_first_winners(plans):
    kinds_of = {}
    for c in CASES:
        if c.kind != "two_copies":
            continue
        ref, cur, planted, mv, cost = _oracle(c.name)
        assert planted, f"{c.name}: nothing planted"
        for pl in planted:
            (x1, y1), (x2, y2) = pl.first, pl.second
            assert (y1, x1) < (y2, x2), (c.name, pl)  # raster order
            assert tuple(mv[pl.block]) == (x1, y1) and cost[pl.block] == 0, (c.name, pl, mv[pl.block])
            x, y, B = pl.bx * c.blk, pl.by * c.blk, c.blk
            blk = cur[y:y + B, x:x + B]
            assert np.array_equal(ref[y + y2:y + y2 + B, x + x2:x + x2 + B], blk), (c.name, pl)
            a = (x - c.range) % 4
            g1, g2 = (x1 + c.range + a) // 4, (x2 + c.range + a) // 4
            if pl.kind == "chunks":
                assert y1 < y2 and x1 > x2
            elif pl.kind == "groups":
                assert y1 == y2 and g1 != g2
            elif pl.kind == "ingroup":
                assert y1 == y2 and g1 == g2 and x2 == x1 + 1
            elif pl.kind == "fold_lo":
                assert (x1, x2) == (c.range - 1, c.range) and y1 == y2
            elif pl.kind == "fold_wrap":
                assert (x1, x2) == (c.range, -c.range) and y2 == y1 + 1
            elif pl.kind == "fold_lane":
                assert x2 == c.range and y1 == y2 and a == 0 and g1 == (y1 + c.range) % c.K < c.K
            tags = {pl.kind}
            p = plans[c.name]
            if _planned(c) and p["ok"]:
                if pl.kind == "chunks" and (y1 + c.range) // c.K != (y2 + c.range) // c.K:
                    tags.add("other chunk")
                    if _pass_of(c, y1) != _pass_of(c, y2):
                        tags.add("other pass")
                if p["fold"] and pl.kind in ("fold_lo", "fold_wrap", "fold_lane"):
                    tags.add(pl.kind + " on a fold plan")
                kinds_of.setdefault((c.cost, c.blk), set()).update(tags)
    for fam in FAST:
        want = set(V.PAIR_KINDS) - {"fold_lane"} | {"other chunk", "other pass"}
        if fam[0] == SAD:  # (the SSD lanes own one dx each: no fold)
            want |= {"fold_lo on a fold plan", "fold_wrap on a fold plan", "fold_lane on a fold plan"}
        assert want <= kinds_of.get(fam, set()), (fam, sorted(want - kinds_of.get(fam, set())))


def test_far_shift_wins_at_the_window_extremes(plans):
    """Every far_shift case with a range has winners at +-S; on fold plans one in
    the fold's dx = +S column."""
    for c in CASES:
        if c.kind != "far_shift" or c.range == 0:
            continue
        ref, cur, _ = V.frames(c)
        if V.oracle_cost(c) > 4e6:  # (the large cases are searched on the GPU machine only)
            continue
        mv, _, _ = O.full_search(ref, cur, c.blk, c.range, "sad" if c.cost == SAD else "mse", threads=NT)
        S = c.range
        if max(c.width, c.height) >= 3 * c.blk + 2 * S:
            assert (np.abs(mv) == S).any(), c.name
        p = plans[c.name]
        if _planned(c) and p["ok"] and c.cost == SAD and p["fold"]:
            assert (mv[:, 0] == S).any(), c.name


def test_antidiag_separates_raster_first_from_column_first():
    n = 0
    for c in CASES:
        if c.kind != "antidiag":
            continue
        ref, cur, _, mv, cost = _oracle(c.name)
        assert (cost == 0).all(), c.name
        assert ((mv[:, 0].astype(int) + mv[:, 1]) % 7 == 0).all(), c.name
        other = V.column_first_search(ref, cur, c.blk, c.range)
        assert (other != mv).any(), f"{c.name}: column-first order finds the raster-first winners"
        n += 1
    assert n >= 8


def test_sat_costs_are_all_maximum():
    seen = set()
    for c in CASES:
        if c.kind != "sat":
            continue
        seen.add((c.cost, c.content))
        if c.content == "sat:random":
            continue
        _, _, _, mv, cost = _oracle(c.name)
        xs, ws, _, _ = V._axis(c.width, c.blk, c.range)
        ys, hs, _, _ = V._axis(c.height, c.blk, c.range)
        area = (hs[:, None] * ws[None, :]).reshape(-1)
        np.testing.assert_array_equal(cost, area * (255 if c.cost == SAD else 255 * 255), err_msg=c.name)
    assert {(SAD, "sat:ref0"), (SAD, "sat:ref255"), (SAD, "sat:random")} <= seen
