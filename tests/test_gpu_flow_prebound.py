"""The chain kernel's pre-bound: a slot's next item bounded one ring turn ahead.

The wave that publishes item k of a slot forms the bound's minlb and the cur
blocks' box sums of item k + ring slots behind the publish, while k's tasks
run; the wave that later fills the slot finds the slot's marker DONE (or waits
for it) and runs only the seeds and the live list (csrc/me_kernels.hip,
flow_fill).  minlb depends on the cur bytes, the plane bytes and the geometry
alone, so nothing may change: every case is compared record for record with the
oracle's full search, each batch run twice into the same buffers, with
me_device_check clean.  On the tuning build (child processes, one per mode, all
cases in each) the live / total lane-task counts must be the same with the
pre-bound on and off and with the planes in LDS, and the count of pre-bound
items says that the path was taken: it is compared with the number the
workgroups' walks give (items k + slots of h = 16 behind an item k), which is
exact where the bypass never engages, and there no item may fall back to the
whole bound.  clamped_256x64 has 512 tiles: on a device of 256 or more CUs a
workgroup has two items and no slot gets a second one, so the modes with
ME_FLOW_WGS=8 (8 workgroups, one per band of the launch's tiles, 64 to 180
items each) are where its clamped windows are pre-bound; they also run the
pre-bound at issue priorities 0 and 3.  bypass_bands is shaped for those modes:
every band is two noise frames and then two shifted ones, so each workgroup
bypasses about 96 items, probes in the shifted frames, leaves the bypass state
and bounds the rest: items whose pre-bound ran are bypassed, and items
published in the bypass state (marker NONE) fall back to the whole bound.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from motionestimation_amd import synth
from test_flow_job_lookup import _progression
from test_gpu_flow_chain import _fields
from test_gpu_flow_slim import _CHILD, _frames, _oracle, _search, _stripe_jobs, B, CUTS  # noqa: F401

S, TB = 32, 4


# ------------------------------------------------------- product build: fields
@functools.lru_cache(maxsize=None)
def _batch32_640x136():
    """32 jobs of 640x136: 90 tiles a frame, about 11 items per workgroup on 256
    CUs; the h = 8 row is not pre-bound, and some items follow one that was not."""
    pairs = [synth.frame_pair(640, 136, 900 + f, *((5, -2) if f % 2 == 0 else (-9, 7))) for f in range(32)]
    ref, cur = np.stack([r for r, _ in pairs]), np.stack([c for _, c in pairs])
    return (ref, cur) + _oracle(ref, cur)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refill_1080p", "batch32_640x136"])
def test_batch_fields_equal_oracle(engine, name):
    """refill_1080p: two frames, the smallest product launch whose 10-slot ring
    refills, so the smallest with a pre-bound."""
    ref, cur, omv, oco = _batch32_640x136() if name == "batch32_640x136" else _fields(name)
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


# ------------------------------------------------------------ the tuning build
@functools.lru_cache(maxsize=None)
def _alternating(group):
    """32 jobs of 320x136 that alternate noise pairs and shifted pairs in groups
    of `group` jobs, the oracle's fields assembled from the two cases' own.
    Job by job (group 1) items k and k + slots of a workgroup lie in different
    jobs.  In groups of 2 a band of 180 tiles (an eighth of the launch: what one
    of 8 workgroups walks) is 90 noise items and then 90 shifted ones."""
    n, s = _fields("noise"), _fields("shifts")
    pick = [(n, f) if (f // group) % 2 == 0 else (s, f % s[0].shape[0]) for f in range(32)]
    return tuple(np.stack([src[i][f] for src, f in pick]) for i in range(4))


def _case(name):
    if name == "alternating":
        return _alternating(1)
    if name == "bypass_bands":
        return _alternating(2)
    return _fields(name)


CASES = ["stripes_640x440", "partial_336x136", "clamped_256x64", "flat", "alternating", "bypass_bands"]
NOISY = ("alternating", "bypass_bands")
MODES = {
    "slots2_pre1": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1"},
    "slots2_pre0": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "0"},
    "slots3_pre1": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1"},
    "slots3_pre0": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "0"},
    "verify": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1", "ME_PRUNE": "2"},
    "table_off": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1", "ME_FLOW_TABLE": "0"},
    "planes_off": {"ME_PRUNE_PLANES": "0"},
    # 8 workgroups: long walks on these small launches; the pre-bound at the other two issue priorities
    "wgs8_slots3_prio0": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1", "ME_FLOW_PRE_PRIO": "0",
                          "ME_FLOW_WGS": "8"},
    "wgs8_slots2_prio3": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1", "ME_FLOW_PRE": "1", "ME_FLOW_PRE_PRIO": "3",
                          "ME_FLOW_WGS": "8"},
}
_ENV = ("ME_PRUNE", "ME_PRUNE_PLANES", "ME_FLOW_SLOTS", "ME_FLOW_TABLE", "ME_FLOW_TABLE_CAP", "ME_FLOW_PRE",
        "ME_FLOW_PRE_PRIO", "ME_FLOW_WGS")

_CHILD_PRE = r"""
import ctypes, json, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import motionestimation_amd as me
assert me._lib.LIB_PATH.endswith("libme_hip_tune.so"), me._lib.LIB_PATH
L = me._lib.lib()
for fn in (L.me_debug_prune_stats, L.me_debug_flow_pre_stats):
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
B, S, CUTS = 16, 32, {cuts!r}
z = np.load({data!r})
out = {{"cus": torch.cuda.get_device_properties(0).multi_processor_count}}
with me.Engine() as eng:
    for name in {cases!r}:
        ref, cur, omv, oco = (z[name + "_" + k] for k in ("ref", "cur", "mv", "co"))
        F, h, w = ref.shape
        nbx = w // B
        if name.startswith("stripes"):
            jobs = []
            for f in range(F):
                for r0, r1 in zip(CUTS, CUTS[1:]):
                    ry0, ry1 = max(0, r0 * B - S), min(h, r1 * B + S)
                    rt = torch.from_numpy(ref[f, ry0:ry1].copy()).cuda()
                    ct = torch.from_numpy(cur[f, r0 * B:min(h, r1 * B)].copy()).cuda()
                    n = (r1 - r0) * nbx
                    jobs.append((rt, ry0, ct, r0 * B, r0, r1, torch.full((n, 2), -7, dtype=torch.int16, device="cuda"),
                                 torch.zeros(n, dtype=torch.int32, device="cuda")))
            run = eng.prepared_stripes_search(w, h, B, S, "sad", jobs)
        else:
            nb = me.num_blocks(w, h, B)
            ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
            mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
            co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
            run = eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        eng.device_check()
        st, pre = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 3)()
        assert L.me_debug_prune_stats(eng._h, st) == 0 and L.me_debug_flow_pre_stats(eng._h, pre) == 0
        if name.startswith("stripes"):
            for i, j in enumerate(jobs):
                f, r0, r1 = i // 3, j[4], j[5]
                assert np.array_equal(j[7].cpu().numpy().view(np.uint32), oco[f][r0 * nbx:r1 * nbx]), (name, "sad", i)
                assert np.array_equal(j[6].cpu().numpy(), omv[f][r0 * nbx:r1 * nbx]), (name, "mv", i)
        else:
            assert np.array_equal(co.cpu().numpy().view(np.uint32).reshape(F, nb), oco), (name, "sad")
            assert np.array_equal(mv.cpu().numpy().reshape(F, nb, 2), omv), (name, "mv")
        out[name] = {{"stats": list(st), "pre": list(pre)}}
print("RESULT " + json.dumps(out))
print("prebound ok")
"""
_results = {}


def _child(mode, tmp_path_factory):
    """Every case in one child on the tuning build, once per mode: equal to the
    oracle there, me_device_check clean; returns {case: {stats: [live, total,
    bypassed, items], pre: [pre-bound, waited, fell back]}, cus: n}."""
    if mode not in _results:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        d = tmp_path_factory.mktemp("prebound")
        data = d / "cases.npz"
        arrays = {}
        for name in CASES:
            for k, a in zip(("ref", "cur", "mv", "co"), _case(name)):
                arrays[name + "_" + k] = a
        np.savez(data, **arrays)
        script = d / "child.py"
        script.write_text(_CHILD_PRE.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cuts=CUTS, data=str(data),
                                            cases=CASES))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        for k in _ENV:
            env.pop(k, None)
        env.update(MODES[mode])
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "prebound ok" in r.stdout
        _results[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    return _results[mode]


def _tile_rows(name):
    """(tile columns, [block rows of every job], frame height) of a case's launch: its tiles run job-major."""
    ref = _case(name)[0]
    F, h, w = ref.shape
    cols = (w // B + TB - 1) // TB
    if name.startswith("stripes"):
        return cols, [list(range(r0, r1)) for _ in range(F) for r0, r1 in zip(CUTS, CUTS[1:])], h
    return cols, [list(range((h + B - 1) // B)) for _ in range(F)], h


def _walk_counts(name, cus, slots):
    """(items, items k + slots of h = 16 behind an item k of the same workgroup) of one launch."""
    cols, jobs, h = _tile_rows(name)
    full = [h - by * B >= B for rows in jobs for by in rows for _ in range(cols)]  # per launch tile
    nwg = min(cus, len(full))
    ahead = 0
    for b in range(nwg):
        tiles = _progression(len(full), nwg, b)
        ahead += sum(1 for t in tiles[slots:] if full[t])
    return len(full), ahead


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_tuning_build_modes_equal_oracle(tmp_path_factory, mode):
    """Rings of 2 and 3 slots pre-bound many turns deep on small launches; with
    the pre-bound on and off, in verify mode (a wrongly dead lane-task fails
    me_device_check), without the item table and with the planes in LDS the
    child compares every case with the oracle; here: every item counted, and
    the pre-bound taken exactly where the mode and the walk say."""
    res = _child(mode, tmp_path_factory)
    slots = int(MODES[mode].get("ME_FLOW_SLOTS", 0))
    for name in CASES:
        live, total, bypassed, items = res[name]["stats"]
        pre, waited, whole = res[name]["pre"]
        print(mode, name, res[name])
        if mode == "planes_off":
            n_items, _ = _walk_counts(name, res["cus"], 1)
            assert items == 2 * n_items and (pre, waited, whole) == (0, 0, 0), (mode, name, res[name])
            continue
        n_items, ahead = _walk_counts(name, min(res["cus"], int(MODES[mode].get("ME_FLOW_WGS", 1 << 20))), slots)
        assert items == 2 * n_items, (mode, name, res[name])  # (each batch runs twice)
        assert 0 < live <= total
        if MODES[mode]["ME_FLOW_PRE"] == "0":
            assert pre == 0 and waited == 0, (mode, name, res[name])
            continue
        assert waited <= pre <= 2 * ahead, (mode, name, res[name])
        # A later turn of a slot with an h = 16 item was pre-bound, or it fell back to the whole bound, or it
        # was bypassed unbound; a pre-bound item may be bypassed as well.
        assert pre + whole <= 2 * ahead <= pre + whole + bypassed, (mode, name, res[name], ahead)
        if name not in NOISY and bypassed == 0:
            # (noise items can raise the bypass state for a publish without one item being bypassed)
            assert pre == 2 * ahead and whole == 0, (mode, name, res[name], ahead)
        elif ahead:
            assert pre > 0, (mode, name, res[name], ahead)
        if name == "bypass_bands" and mode.startswith("wgs8"):
            # The bypass engaged behind pre-bounds (their results ignored) and ended: items published in the
            # bypass state found the marker NONE and ran the whole bound, the rest of the band was pre-bound.
            assert bypassed >= 2 * 8 * 90 // 2 and whole > 0 and 0 < pre < 2 * ahead, (mode, res[name], ahead)
    # the path was taken: small rings pre-bound on every case whose workgroups have more items than slots
    if MODES[mode].get("ME_FLOW_PRE") == "1":
        assert sum(res[name]["pre"][0] for name in CASES) > 0


@pytest.mark.gpu
def test_live_lists_equal_with_the_prebound_on_and_off(tmp_path_factory):
    """The same live and total lane-task counts with the pre-bound on and off,
    in every ring, without the table and with the planes in LDS (whose bound is
    the independent code), on the inputs where the bypass does not engage."""
    off = _child("planes_off", tmp_path_factory)
    for mode in MODES:
        if mode in ("planes_off", "verify"):  # (verify: every lane-task is live)
            continue
        on = _child(mode, tmp_path_factory)
        for name in CASES:
            if name in NOISY:
                continue
            # (a long walk of 8 workgroups meets runs of items the bound cannot thin on these inputs too: the
            # bypass's own doing, on or off the pre-bound; one workgroup per CU never does)
            if on[name]["stats"][2] and mode.startswith("wgs8"):
                continue
            assert on[name]["stats"][2] == 0 or name == "flat", (mode, name, on[name])
            print(mode, name, on[name]["stats"], "planes_off", off[name]["stats"])
            assert on[name]["stats"][:2] == off[name]["stats"][:2], (mode, name, on[name], off[name])
