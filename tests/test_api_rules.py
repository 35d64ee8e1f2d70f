"""The C ABI's argument rules and record layouts, without a GPU.

csrc/me_api_rules.cpp holds every argument rule of the entry points and the
layout of the record buffer of each host entry point; it is host-only C++.
oracle/api_rules_dump.cc links it alone (plus the host-only planner files its
rules call) and replays tests/golden/api_args.json: the calls the library
refused before the rules moved there, recorded on an MI355X
(tests/golden/make_api_args.py).  Same status for every case; same message
for every case but the frame-batch ones ("loose"), whose two wordings were
merged on purpose.  tests/test_gpu_api_rules.py holds the library's entry
points to the same table.

What the table cannot hold -- calls the library accepts would launch kernels
while recording -- is checked here against include/me.h: the accepted side of
every boundary, and the entry points that refuse a context of several devices.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle")
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_api_args as T  # noqa: E402

ME_OK, ME_EINVAL, ME_EUNSUPPORTED = 0, 1, 5
DUMP = os.path.join(ORACLE, "api_rules_dump")


@pytest.fixture(scope="module")
def dump():
    subprocess.run(["make", "-s", "-C", ORACLE, "api_rules_dump"], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([DUMP, *map(str, args)], capture_output=True, text=True, timeout=60, check=True)
        return [json.loads(l) for l in r.stdout.splitlines()]
    return run


def _replay(dump, tmp_path, cases, ndev=1):
    path = tmp_path / "cases.json"
    path.write_text("\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n")
    got = dump(path, ndev)
    assert [g["name"] for g in got] == [c["name"] for c in cases]
    return got


def test_table_statuses_and_messages(dump):
    want = T.load_table()
    got = {g["name"]: g for g in dump(T.TABLE)}
    assert len(got) == len(want) > 500
    for w in want:
        g = got[w["name"]]
        assert w["status"] != ME_OK
        assert g["status"] == w["status"], (w, g)
        if w["loose"]:
            assert g["message"], w
        else:
            assert g["message"] == w["message"], (w, g)


def test_table_is_the_case_list():
    """Every case of the list is in the table (none was accepted and dropped),
    with two rules broken at once in at least twenty of them."""
    want = {c["name"]: c for c in T.cases()}
    table = {r["name"]: r for r in T.load_table()}
    assert set(table) == set(want)
    for name, c in want.items():
        assert {k: table[name][k] for k in c} == c
    assert {r["fn"] for r in table.values()} == set(T.SPECS)
    singles = {n for fn in T.SPECS for n in T.violations(fn)}
    assert sum(r["name"].split(":", 1)[1] not in singles for r in table.values()) >= 20
    assert any(r["loose"] for r in table.values())


# The accepted side of each boundary (include/me.h), per entry point family.
def _accepted():
    out = []
    for fn, (names, _, costs, max_range, max_lambda) in T.SPECS.items():
        names = names.split()
        over = [{}]
        over += [{"blk": b} for b in ((8, 32) if "partition" in fn else (1, 64))]
        if max_range:
            over += [{"range": 0}, {"range": max_range}]
        if max_lambda:
            over += [{"lambda": 0}, {"lambda": max_lambda}]
        over += [{"cost": k} for k in costs or ()]
        if "stride" in names:
            over.append({"stride": 49})
        if "n_frames" in names:
            over.append({"n_frames": 4096})
        for fs in T.SIZES:
            if fs in names:
                over += [{"n_frames": 2, fs: T.FB}, {"n_frames": 2, fs: (1 << 31) - T.FB - 1},
                         {"n_frames": 1, fs: 0}]
        if fn in T.VECTORS:
            lim, arrays = T.VECTORS[fn]
            over += [{"elem": 3, "elem_val": v, "elem_arr": a} for v in (lim, -lim) for a in range(arrays)]
        if fn in T.MODES:
            over.append({"mode_idx": 5, "mode_val": 2})
        if "num_blks" in names:
            over += [{"pix_idx": 0, "pix_val": 255}, {"pix_idx": 1, "pix_val": 0}]
        if "r0" in names:
            over += [{"r0": 1, "r1": 2, "ref_row0": 12, "cur_row0": 16}, {"r0": 2, "r1": 2}]
        for o in over:
            case = dict(name=f"{fn}:{sorted(o.items())}", fn=fn, n_jobs=1, **o)  # (a list of the one job)
            if o.get("blk") == 1:
                case["num_blks"] = T.W * T.H
            elif o.get("blk") in (8, 32, 64):
                b = o["blk"]
                case["num_blks"] = -(-T.W // b) * -(-T.H // b)
                case["r1"] = -(-T.H // b) if "r1" not in o else o["r1"]
            out.append(case)
    return out


def test_accepted_side_of_every_boundary(dump, tmp_path):
    cases = _accepted()
    assert len(cases) > 200
    for c, g in zip(cases, _replay(dump, tmp_path, cases)):
        assert (g["status"], g["message"]) == (ME_OK, ""), (c, g)


# include/me.h documents ME_EUNSUPPORTED on a context of several devices for
# these; the others use the context's first device.
ONE_DEVICE_ONLY = {
    "me_full_search_qpel", "me_full_search_bipred", "me_partition_search_device", "me_partition_search",
    "me_partition_leaf_field_device", "me_rd_search_device", "me_rd_search", "me_refine_qpel_rd_device",
    "me_refine_qpel_rd", "me_full_search_rd_qpel", "me_partition_rd_search_device",
    "me_partition_rd_search"}


def test_device_count_rules(dump, tmp_path):
    cases = [dict(name=fn, fn=fn) for fn in T.SPECS]
    for c, g in zip(cases, _replay(dump, tmp_path, cases, ndev=2)):
        if c["fn"] in ONE_DEVICE_ONLY:
            assert g["status"] == ME_EUNSUPPORTED and "on 2 devices (one device only)" in g["message"], g
        else:
            assert (g["status"], g["message"]) == (ME_OK, ""), g
    # a broken argument is reported before the device count, as on one device
    broken = [dict(name=fn, fn=fn, width=0) for fn in sorted(ONE_DEVICE_ONLY)]
    for g in _replay(dump, tmp_path, broken, ndev=2):
        assert g["status"] == ME_EINVAL and "devices" not in g["message"], g


@pytest.mark.parametrize("shape", [(48, 32, 16), (50, 34, 8)])
def test_record_layouts(dump, shape):
    """Disjoint regions in the order and at the sizes the entry points used
    before the layouts were functions, each aligned to its element, and the
    byte count they asked grow() for: 8 nb; 28 nb; 17 nb rounded up to 8; the
    partition grids' bytes rounded up to 8 (upload_pair took a count of 8-byte
    records)."""
    (got,) = dump("--layouts", *shape)
    w, h, b = shape
    nb = -(-w // b) * -(-h // b)
    nhx, nhy = -(-w // (b // 2)), -(-h // (b // 2))
    n = [nb, -(-w // b) * nhy, nhx * -(-h // b), nhx * nhy]
    assert got["n_blocks"] == nb and got["counts"] == n
    assert nb % 2 == (shape != (48, 32, 16))  # the second shape's counts are odd
    cells = sum(n)
    g4 = [(4 * k, 4) for k in n]
    want = {
        "mv_cost": ([(4 * nb, 2), (4 * nb, 4)], 8 * nb),
        "bipred": ([(4 * nb, 2), (4 * nb, 2), (4 * nb, 4), (12 * nb, 4), (nb, 1)], 28 * nb),
        "rd": ([(4 * nb, 2), (4 * nb, 2), (4 * nb, 4), (4 * nb, 4), (nb, 1)], (17 * nb + 7) // 8 * 8),
        "partition": ([(4 * k, 2) for k in n] + g4 + [(4 * n[0], 4), (n[0], 1)],
                      (8 * cells + 4 * n[0] + n[0] + 7) // 8 * 8),
        "partition_rd": ([(4 * n[0], 2)] + [(4 * k, 2) for k in n] + g4 + g4 + [(4 * n[0], 4)] +
                         [(k, 1) for k in n] + [(n[0], 1)],
                         (4 * n[0] + 12 * cells + 4 * n[0] + cells + n[0] + 7) // 8 * 8),
    }
    assert set(got) == set(want) | {"n_blocks", "counts"}
    for name, (regions, total) in want.items():
        L = got[name]
        assert L["total"] == total, name
        end = 0
        for (off, size, elem), (want_size, want_elem) in zip(L["regions"], regions, strict=True):
            assert (size, elem) == (want_size, want_elem), name
            assert off == end and off % elem == 0, (name, off)  # back to back: disjoint, in order
            end = off + size
        assert end <= total
