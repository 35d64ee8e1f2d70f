"""The pruning flow kernel's item chain: the LDS item table, the bound started
under the window DMA, and the fold column fetched under the last chunk.

In a launch with box-sum planes a workgroup decodes its items once into a table
behind its control block (csrc/me_geom.h FlowEntry, tests/test_flow_item_table.py);
a slot's fill issues the cur blocks and the first plane rows in front of the
window's DMA and waits for those alone, so paths of the bound that never read
the window (the h = 8 row, the bypass state) must still wait for it before the
slot is published; and the bound's last chunk runs apart from the loop, with
the fold column's loads in flight.  Nothing of this may change a field or a
live list: every case is compared record for record with the oracle's full
search, each batch run twice into the same buffers, and the tuning build's
live / total lane-task counts must be the same with the table on, off and
overflowed, on short rings, in verify mode and with the planes in LDS (whose
step 2 is untouched code).
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_flow_job_lookup import _progression
from test_gpu_flow_slim import _CHILD, _frames, _oracle, _search, _stripe_jobs, B, CUTS
from test_gpu_flow_slim import test_batch_fields_equal_oracle as _slim_batch_test



def _cases_of(test, argname):
    """The values a test's parametrize mark gives `argname` (positional or by keyword, any number of marks)."""
    for m in getattr(test, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = m.args[0] if m.args else m.kwargs.get("argnames")
        values = m.args[1] if len(m.args) > 1 else m.kwargs.get("argvalues")
        if names == argname or names == [argname] or names == (argname,):
            return list(values)
    return []


# The cases this issue names; with them whatever else the slim-scratch test of
# the same name runs (read from its mark, so the two lists cannot drift apart
# unnoticed; the named ones stand here in any case).
CHAIN_CASES = ["clamped_256x64", "shifts", "partial_336x136", "noise", "flat", "refill_1080p"]
BATCH_CASES = CHAIN_CASES + [c for c in _cases_of(_slim_batch_test, "name") if c not in CHAIN_CASES]


@functools.lru_cache(maxsize=None)
def _fields(name):
    """(ref, cur, oracle mv, oracle cost) of a named case, computed once."""
    ref, cur = _frames(name)
    return (ref, cur) + _oracle(ref, cur)


# ------------------------------------------------------- product build: fields
@pytest.mark.gpu
@pytest.mark.parametrize("name", BATCH_CASES)
def test_batch_fields_equal_oracle(engine, name):
    """clamped_256x64: 32 jobs, every window clamped, items of fewer than five
    tasks in the table's prefixes.  shifts (320x136 x 20): the h = 8 row returns
    from the bound before its step 3 and must still wait for the window.
    partial_336x136: a one-block last tile.  noise: the bypass engages, and a
    prober leaves it.  flat: every bound ties.  refill_1080p: two frames, the
    smallest product launch that refills a 10-slot ring through the table."""
    ref, cur, omv, oco = _fields(name)
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


@pytest.mark.gpu
def test_unequal_stripes_with_halos(engine):
    import torch
    ref, cur, omv, oco = _fields("stripes_640x440")
    nbx = ref.shape[2] // B
    jobs = _stripe_jobs(ref, cur)
    run = engine.prepared_stripes_search(ref.shape[2], ref.shape[1], B, 32, "sad", jobs)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    engine.device_check()
    for i, j in enumerate(jobs):
        f, (r0, r1) = i // 3, (j[4], j[5])
        np.testing.assert_array_equal(j[7].cpu().numpy().view(np.uint32), oco[f][r0 * nbx:r1 * nbx],
                                      err_msg=f"job {i} sad")
        np.testing.assert_array_equal(j[6].cpu().numpy(), omv[f][r0 * nbx:r1 * nbx], err_msg=f"job {i} mv")


# ------------------------------------------------------------ the tuning build
MODES = {
    "table_auto": {"ME_PRUNE_PLANES": "1"},
    "table_off": {"ME_FLOW_TABLE": "0", "ME_PRUNE_PLANES": "1"},
    "table_cap1": {"ME_FLOW_TABLE_CAP": "1", "ME_PRUNE_PLANES": "1"},  # more than one item a workgroup: no table
    "slots2": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1"},
    "slots3": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1"},
    "verify": {"ME_PRUNE": "2", "ME_PRUNE_PLANES": "1"},
    "planes_off": {"ME_PRUNE_PLANES": "0"},
}
_stats = {}
_table = {}
# the child also reports the item table of its last launch with planes (me_debug_flow_table)
_CHILD_TABLE = _CHILD + r"""
L.me_debug_flow_table.argtypes = []
L.me_debug_flow_table.restype = ctypes.c_int
print("TABLE %d %d" % (L.me_debug_flow_table(), torch.cuda.get_device_properties(0).multi_processor_count))
"""


def _child(mode, tmp_path_factory):
    """The three-stripe case in a child on the tuning build, once per mode:
    equal to the oracle there, me_device_check clean; returns [live, total,
    bypassed, items]."""
    if mode not in _stats:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        d = tmp_path_factory.mktemp("chain_" + mode)
        ref, cur, omv, oco = _fields("stripes_640x440")
        np.savez(d / "case.npz", ref=ref, cur=cur, mv=omv, co=oco)
        script = d / "child.py"
        script.write_text(_CHILD_TABLE.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cuts=CUTS,
                                        data=str(d / "case.npz")))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        for k in ("ME_PRUNE", "ME_PRUNE_PLANES", "ME_FLOW_SLOTS", "ME_FLOW_TABLE", "ME_FLOW_TABLE_CAP"):
            env.pop(k, None)
        env.update(MODES[mode])
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "slim ok" in r.stdout
        _stats[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
        _table[mode] = tuple(int(x) for x in [ln for ln in r.stdout.splitlines() if ln.startswith("TABLE ")][0].split()[1:])
    return _stats[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_tuning_build_modes_equal_oracle(tmp_path_factory, mode):
    """No table, a table that does not fit (the fallback path), rings of 2 and
    3 slots (refills through the table on a small launch), verify mode (a
    wrongly dead lane-task fails me_device_check) and the planes in LDS: equal
    to the oracle, every full-height and h = 8 item counted."""
    live, total, bypassed, items = _child(mode, tmp_path_factory)
    assert items == 2 * 28 * 10, (mode, live, total, bypassed, items)  # 640 / 64 tile columns x 28 block rows x 2
    assert 0 < live <= total
    # The path the mode names is the path the launch took: the table's entries
    # (the longest walk's items and the end entry) where it is on, none where
    # the switch turns it off or the cap overflows it, no launch with planes at all.
    entries, cus = _table[mode]
    most = max(len(_progression(items, min(cus, items), b)) for b in range(min(cus, items)))
    assert most > 1  # (so that a cap of one item overflows)
    want = {"table_off": 0, "table_cap1": 0, "planes_off": -1}.get(mode, most + 1)
    assert entries == want, (mode, entries, want)


@pytest.mark.gpu
def test_live_lists_equal_across_modes(tmp_path_factory):
    """The same live and total lane-task counts in every mode with planes as
    with the planes in LDS, whose step 2 is the independent check of the bound
    that reads them from global memory."""
    off = _child("planes_off", tmp_path_factory)
    for mode in MODES:
        on = _child(mode, tmp_path_factory)
        print(mode, on, "planes_off", off)
        assert on[:2] == off[:2], (mode, on, off)
