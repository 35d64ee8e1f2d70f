"""The flow kernel's LDS item table (csrc/me_geom.h FlowEntry).

In a pruning launch with box-sum planes a workgroup decodes its items once, in
front of its start barrier: entry k holds the index of item k's first wave-task
(the prefix sum of the items' task counts; entry nitems the workgroup's total)
and job | tile column << 5 | block row << 16, from which the waves rebuild the
Item with no job-table load.  bin/flow_table_dump (tools/flow_table_dump.cc)
compiles the header alone and fills the table with the functions the kernel
compiles; here every workgroup's table is compared with the rule written out in
Python: the tile -> job scan of tests/test_flow_job_lookup.py, the row-major
tile -> (block row, first block) map, and the task count from the dy clamp.
No GPU and no library load.
"""
import json
import os
import subprocess

import pytest

from test_flow_job_lookup import TABLES, _progression, scan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(REPO, "bin", "flow_table_dump")
B, K, S, TB, G, CHUNKS = 16, 13, 32, 4, 16, 5
ROOM = 163840 - 149696  # the LDS a 10-slot slim ring leaves (tests/test_flow_slim_plan.py pins both)


@pytest.fixture(scope="module")
def dump():
    subprocess.run(["make", "-s", "-C", REPO, "-f", "tools.mk", "bin/flow_table_dump"], check=True, timeout=300)

    def run(w, h, nwg, bid, room, cap, jobs, strip=0):
        spec = ",".join(f"{r0}:{t}" for r0, t in jobs)
        r = subprocess.run([DUMP, *map(str, (w, h, nwg, bid, room, cap)), spec] + ([str(strip)] if strip else []),
                           capture_output=True, text=True,
                           timeout=120, check=True)
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


def rule(w, h, jobs, tile):
    """(Item fields in the tool's order, first valid chunk, wave-tasks) of a launch tile."""
    counts = [t for _, t in jobs]
    pre = [0]
    for c in counts:
        pre.append(pre[-1] + c)
    j = 0
    while j + 1 < len(counts) and pre[j + 1] <= tile:
        j += 1
    nbx = w // B
    wpr = (nbx + TB - 1) // TB
    t = tile - pre[j]
    by, bx0 = jobs[j][0] + t // wpr, (t % wpr) * TB
    nb = min(TB, nbx - bx0)
    tly = by * B
    hh = min(B, h - tly)
    a = (bx0 * B - S) % 4
    dymin, dymax = max(-S, -tly), min(S, h - hh - tly)
    lc0, lc1 = max(0, (dymin + S) // K), min(CHUNKS, (dymax + S) // K + 1)
    tasks = ((lc1 - lc0) * nb * G + 63) >> 6
    return [j, bx0, by, nb, tly, hh, a, bx0 * B - S - a, 0, CHUNKS, tly - S, CHUNKS * K + B - 1], lc0, tasks


def frames(w, h, n):
    """n whole frames, a job each."""
    rows = (h + B - 1) // B
    wpr = (w // B + TB - 1) // TB
    return [(0, rows * wpr)] * n


def stripes(w, cuts, n):
    wpr = (w // B + TB - 1) // TB
    return [(r0, (r1 - r0) * wpr) for _ in range(n) for r0, r1 in zip(cuts, cuts[1:])]


# name -> (width, height, workgroups, jobs as (first block row, launch tiles))
LAUNCHES = {
    "1080p_x16": (1920, 1080, 256, frames(1920, 1080, 16)),
    "1080p_x32": (1920, 1080, 256, frames(1920, 1080, 32)),
    "stripes_640x440": (640, 440, 256, stripes(640, [0, 7, 19, 28], 2)),
    "clamped_256x64": (256, 64, 256, frames(256, 64, 32)),  # every row clamped: items of fewer than 5 tasks
    "partial_336x136": (336, 136, 256, frames(336, 136, 20)),  # a one-block last tile, an h = 8 row
    "few_workgroups": (336, 136, 7, frames(336, 136, 3)),
}
# the job tables of the lookup test, the empty-job ones among them: one tile per
# block row (64 columns), so a table's counts are its jobs' rows
for _name, _counts in TABLES.items():
    LAUNCHES["lookup_" + _name] = (64, B * max(_counts), 256 if sum(_counts) > 300 else 7, [(0, c) for c in _counts])


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_every_workgroups_table_equals_the_scan(dump, name):
    w, h, nwg, jobs = LAUNCHES[name]
    ntiles = sum(t for _, t in jobs)
    recs = dump(w, h, nwg, -1, ROOM, 0, jobs)
    assert [r["bid"] for r in recs] == list(range(nwg))
    want_jobs = scan([t for _, t in jobs])
    seen, most = [], 0
    for r in recs:
        tiles = _progression(ntiles, nwg, r["bid"])
        assert r["tiles"] == tiles, r["bid"]
        pre = 0
        assert len(r["pre"]) == len(tiles) + 1
        for k, tile in enumerate(tiles):
            item, lc0, tasks = rule(w, h, jobs, tile)
            assert item[0] == want_jobs[tile]
            assert r["items"][k] == item, (r["bid"], k, tile)
            assert r["lc0"][k] == lc0, (r["bid"], k)
            assert r["pre"][k] == pre, (r["bid"], k)
            assert r["pack"][k] == item[0] | (item[1] // TB) << 5 | item[2] << 16
            assert tasks >= 1
            pre += tasks
        assert r["pre"][-1] == pre
        seen += tiles
        most = max(most, len(tiles))
    assert sorted(seen) == list(range(ntiles))
    # the launch's decision: the longest walk's items and the end entry, 8 bytes each
    assert 8 * (most + 1) <= ROOM
    assert all(r["entries"] == most + 1 for r in recs)


def test_short_items_and_bottom_row_are_among_the_cases(dump):
    w, h, nwg, jobs = LAUNCHES["clamped_256x64"]
    tasks = [rule(w, h, jobs, t)[2] for t in range(sum(t for _, t in jobs))]
    assert max(tasks) < 5
    w, h, nwg, jobs = LAUNCHES["partial_336x136"]
    items = [rule(w, h, jobs, t)[0] for t in range(sum(t for _, t in jobs))]
    assert any(it[5] == 8 for it in items) and any(it[3] == 1 for it in items)


@pytest.mark.parametrize("name", ["1080p_x16", "1080p_x32", "stripes_640x440", "few_workgroups"])
def test_fit_decision_matches_the_bytes(dump, name):
    w, h, nwg, jobs = LAUNCHES[name]
    ntiles = sum(t for _, t in jobs)
    most = max(len(_progression(ntiles, nwg, b)) for b in range(nwg))
    need = 8 * (most + 1)
    for room, cap, want in [(need, 0, most + 1), (need - 1, 0, 0), (0, 0, 0), (ROOM, most, most + 1),
                            (ROOM, most - 1 if most > 1 else 1, 0 if most > 1 else most + 1), (ROOM, 1, 0 if most > 1 else 2)]:
        (r,) = dump(w, h, nwg, 0, room, cap, jobs)
        assert r["entries"] == want, (room, cap, most)


def test_fields_past_their_bits_get_no_table(dump):
    """The packed word has 16 bits of block row and 11 of tile column."""
    (r,) = dump(64, B * 65536, 7, 0, ROOM, 0, [(65530, 20)])
    assert r["entries"] == 0
    (r,) = dump(64, B * 65536, 7, 0, ROOM, 0, [(65510, 20)])
    assert r["entries"] == 4  # 20 tiles over 7 workgroups: 3 items at most, and the end entry
    # 2,049 tile columns (131,136 / 64) do not fit 11 bits; 2,048 do
    (r,) = dump(64 * 2049, 64, 7, 0, ROOM, 0, [(0, 2049)])
    assert r["entries"] == 0
    (r,) = dump(64 * 2048, 64, 7, 0, ROOM, 0, [(0, 2048)])
    assert r["entries"] == 2048 // 7 + 1 + 1


def test_strip_walk_gets_no_table(dump):
    """flow_entry_of maps tiles row-major: a plan that walks them in strips keeps the old path."""
    w, h, nwg, jobs = LAUNCHES["few_workgroups"]
    (r,) = dump(w, h, nwg, 0, ROOM, 0, jobs)
    assert r["entries"] > 0
    (r,) = dump(w, h, nwg, 0, ROOM, 0, jobs, strip=2)
    assert r["entries"] == 0
