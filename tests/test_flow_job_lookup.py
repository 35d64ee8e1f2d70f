"""The launch tile -> job rule the flow kernel compiles (csrc/me_geom.h).

A launch's tiles are job-major: job j owns tiles [tile_pre[j], tile_pre[j + 1]).
The rule is the scan's: a tile's job is the smallest j with tile_pre[j + 1] >
tile, so a job without tiles owns none.  me_flow_kernel no longer scans from
job 0: a wave's first item bisects the table (flow_job_find) and every later
item, and every refill target, is found from the job of an earlier item of the
workgroup (flow_job_from), whose tiles only grow.  bin/flow_job_dump
(tools/flow_job_dump.cc) compiles the header alone and prints what the two
functions give; here every tile of every table is compared with the scan
written out in Python.  No GPU and no library load.

The rule has no uniform-count shortcut (no division by a per-job tile count):
uniform tables and tables one count away from uniform are ordinary tables.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(REPO, "bin", "flow_job_dump")


@pytest.fixture(scope="module")
def dump():
    subprocess.run(["make", "-s", "-C", REPO, "-f", "tools.mk", "bin/flow_job_dump"], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([DUMP, *map(str, args)], capture_output=True, text=True, timeout=60, check=True)
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


def scan(counts):
    """Per tile, the smallest j with tile_pre[j + 1] > tile."""
    pre = [0]
    for c in counts:
        pre.append(pre[-1] + c)
    jobs = []
    for t in range(pre[-1]):
        j = 0
        while j + 1 < len(counts) and pre[j + 1] <= t:
            j += 1
        jobs.append(j)
    return jobs


TABLES = {
    "uniform_1": [37],
    "uniform_2": [40, 40],
    "uniform_16": [20] * 16,
    "uniform_32": [17] * 32,
    "uniform_32_one_tile": [1] * 32,
    "1080p_batch16": [2040] * 16,
    "nonuniform_3": [5, 90, 17],
    "nonuniform_32": [5 * (1 + (7 * j) % 11) for j in range(32)],
    "one_count_off_first": [21] + [20] * 15,
    "one_count_off_middle": [20] * 7 + [19] + [20] * 8,
    "one_count_off_last": [20] * 31 + [25],
    "two_jobs_unequal": [40, 41],
    "empty_front": [0, 0, 12, 30, 7],
    "empty_middle": [12, 0, 30, 0, 0, 7, 9],
    "empty_end": [12, 30, 7, 0, 0],
    "empty_everywhere": [0, 5, 0, 0, 5, 5, 0, 1, 0],
    "empty_32": [0 if j % 3 == 1 else 4 + j for j in range(32)],
}


@pytest.mark.parametrize("name", list(TABLES))
def test_every_tile_gets_the_scans_job(dump, name):
    counts = TABLES[name]
    want = scan(counts)
    (got,) = dump("table", ",".join(map(str, counts)))
    assert got["find"] == want, name
    assert got["scan"] == want, name
    # a job without tiles owns no tile
    assert all(counts[j] > 0 for j in want)


def _progression(ntiles, nwg, bid):
    """me_flow_kernel's tiles of workgroup bid (csrc/me_kernels.hip: band bid % 8
    of the launch, member bid / 8 takes every n_x-th tile of it)."""
    ng = min(nwg, 8)
    x, m = bid % ng, bid // ng
    n_x = nwg // ng + (1 if x < nwg % ng else 0)
    band0, band1 = ntiles * x // ng, ntiles * (x + 1) // ng
    return list(range(band0 + m, band1, n_x))


# (table, workgroups, ring slots): the bench launch's shape scaled down, jobs a
# workgroup's step (32 tiles at 256 workgroups) skips whole, empty jobs, and
# the 6-slot and 4-slot rings.
WALKS = [("1080p_batch16", 256, 6), ("uniform_32", 256, 6), ("nonuniform_32", 256, 6),
         ("nonuniform_32", 256, 4), ("empty_32", 256, 6), ("empty_everywhere", 256, 4),
         ("one_count_off_middle", 256, 6), ("uniform_32_one_tile", 256, 6), ("nonuniform_3", 7, 2)]


@pytest.mark.parametrize("name,nwg,nb", WALKS)
def test_walk_from_the_previous_job(dump, name, nwg, nb):
    """Every workgroup's items in order, each looked up from the job of the item
    before it, and every + NB refill target looked up from the current item's
    job: the scan's job every time; together the workgroups take every tile once."""
    counts = TABLES[name]
    want = scan(counts)
    recs = dump("walk", nwg, nb, ",".join(map(str, counts)))
    assert [r["bid"] for r in recs] == list(range(nwg))
    seen = []
    for r in recs:
        tiles = _progression(len(want), nwg, r["bid"])
        assert r["tiles"] == tiles, r["bid"]
        assert r["adv"] == [want[t] for t in tiles], r["bid"]
        assert r["refill"] == [want[tiles[k + nb]] if k + nb < len(tiles) else -1
                               for k in range(len(tiles))], r["bid"]
        seen += tiles
    assert sorted(seen) == list(range(len(want)))
