"""The row split's rule (csrc/me_geom.h flow_split_*), on the CPU.

A wave-task of a pruned h = 16 item that holds n <= 32 list entries runs with
R rows of the chunk's 13 per lane and P = ceil(13 / R) lanes per entry:
R = ceil(13 / min(13, 64 // n)) rounded up to an instance the kernel has
(1, 2, 3, 4, 7; 13 = the task runs whole), part i from row min(i R, 13 - R).
bin/flow_split_dump (tools/flow_split_dump.cc) compiles the header alone and
prints, for n = 1 .. 64, what flow_split_lane (the function flow_split_task
places its lanes with) gives for the 64 lanes.  No GPU and no library load.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(REPO, "bin", "flow_split_dump")
K = 13
INSTANCES = (1, 2, 3, 4, 7, 13)


@pytest.fixture(scope="module")
def rule():
    subprocess.run(["make", "-s", "-C", REPO, "-f", "tools.mk", "bin/flow_split_dump"], check=True, timeout=300)
    r = subprocess.run([DUMP], capture_output=True, text=True, timeout=60, check=True)
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    assert [d["n"] for d in rows] == list(range(1, 65))
    return rows


def test_rows_and_parts_follow_the_stated_rule(rule):
    for d in rule:
        n = d["n"]
        want = -(-K // min(K, 64 // n))
        want = min(r for r in INSTANCES if r >= want)
        assert d["rows"] == want, d["n"]
        assert d["parts"] == -(-K // d["rows"])
    table = {d["n"]: (d["parts"], d["rows"]) for d in rule}
    assert all(table[n] == (13, 1) for n in range(1, 5))
    assert all(table[n][1] == 2 for n in range(5, 10))
    assert all(table[n][1] == 3 for n in range(10, 13))
    assert all(table[n][1] == 4 for n in range(13, 17))
    assert all(table[n] == (2, 7) for n in range(17, 33))
    assert all(table[n] == (1, 13) for n in range(33, 65))
    # the earlier rule, kept for the tuning build's A/B
    assert all((d["parts_124"], d["rows_124"]) == ((4, 4) if d["n"] <= 16 else (2, 7) if d["n"] <= 32 else (1, 13))
               for d in rule)


@pytest.mark.parametrize("which", ["", "_124"])
def test_lanes_cover_every_row_of_every_entry_once_folded(rule, which):
    for d in rule:
        n, R, P = d["n"], d["rows" + which], d["parts" + which]
        assert P * n <= 64, n
        lanes = d["lanes" + which]
        assert len(lanes) == 64
        covered = [set() for _ in range(n)]
        folds = [0] * n
        for lane, (e, row0, live, fold) in enumerate(lanes):
            assert 0 <= e < n, (n, lane)
            assert 0 <= row0 and row0 + R <= K, (n, lane)  # no row outside 0 .. 12
            assert live == (1 if lane < n * P else 0), (n, lane)
            if lane >= n * P:
                assert e == n - 1 and not fold, (n, lane)
            else:
                assert e == lane // P, (n, lane)
                covered[e].update(range(row0, row0 + R))
            assert fold == (1 if live and row0 == 0 else 0), (n, lane)  # the kernel's test of part 0 is row0 == 0
            folds[e] += fold
        assert all(c == set(range(K)) for c in covered), n
        assert folds == [1] * n, n
