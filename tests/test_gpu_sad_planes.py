"""The pruning flow kernel's box sums from the per-frame prepass planes.

me_box_planes_kernel writes q = (4x4 box sum) >> 4 (`box_q` of
tests/test_gpu_sad_prune.py) of every job's resident reference rows once per
launch, as four x-phase byte planes in the context scratch; the wave that stages
an item of me_flow_kernel<16, 13, 144> DMAs the item's 4 x 77 x 32 bytes into
the slot's bound scratch instead of forming them from the window (step 1 of
flow_bound, which stays as the fallback).  Same q, so the same live lists and
the same fields: every test compares record for record with the oracle's full
search (src/cpu/main.c:39-82 restated), and the tuning build's live / total
lane-task counts must be equal with the planes on and off.

CPU: the scratch sizing (flow_planes_scratch, me_valu_plan.cpp, through
bin/flow_planes_dump).  GPU: the product build on the pruning cases, a width
whose plane row pitch needs padding, a batch of unequal stripes with halos,
capture without a warm-up run, and the tuning build's modes in child processes.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_sad_prune import B, NT, S, _case, _search

DUMP = os.path.join(O.REPO, "bin", "flow_planes_dump")
CASES = ["shifts", "fold_corners", "flat", "clamped_256x64"]
PADDED = "padded_pitch"  # + the width of _padded_width()


def _dump(w, h, cost, planes, jobs, blk=B, span=S):
    subprocess.run(["make", "-s", "-C", O.REPO, "-f", "tools.mk", "bin/flow_planes_dump"], check=True, timeout=300)
    r = subprocess.run([DUMP, str(w), str(h), str(blk), str(span), str(cost), str(planes)] +
                       [f"{a}:{b}:{c}" for a, b, c in jobs], capture_output=True, text=True, timeout=60, check=True)
    return json.loads(r.stdout)


@functools.lru_cache(maxsize=None)
def _padded_width():
    """The first width around 336 whose 20 x 136-row batch gets the pruning flow
    plan (the planner's own answer) and whose (W + 64) / 4 is no multiple of 16."""
    for w in (336, 304, 352, 368, 288):
        d = _dump(w, 136, 1, -1, [(0, 9, 0)] * 20)
        if d["flow"] and d["prune"] and d["tb"] == 4 and ((w + 64) // 4) % 16:
            assert d["pitch"] % 16 == 0 and d["pitch"] >= (w + 64) // 4
            return w
    raise AssertionError("no width with a padded plane pitch takes the flow plan")


# ------------------------------------------------------------------ CPU: sizing
def test_scratch_size_zero_without_the_pruning_flow_plan():
    assert _dump(1920, 1080, 0, -1, [(0, 68, 0)])["need"] == 0          # SSD
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)], span=16)["need"] == 0  # +-16: no flow plan
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)], blk=8)["need"] == 0    # 8x8: the item kernel
    assert _dump(1920, 1080, 1, -1, [(0, 4, 0)])["need"] == 0            # a small stripe: too few tiles
    assert _dump(1920, 1080, 1, 0, [(0, 68, 0)])["need"] == 0            # planes off
    d = _dump(1920, 1080, 1, 0, [(0, 68, 0)])
    assert d["flow"] and d["prune"]  # (the plan itself does not change with the planes)


def test_scratch_size_is_the_documented_bytes():
    # one 1080p frame: 1080 rows x 4 phases x 496 bytes ((1920 + 64) / 4)
    d = _dump(1920, 1080, 1, 1, [(0, 68, 0)])
    assert d["pitch"] == 496 and d["jobs"] == [{"rows": 1080, "bytes": 1080 * 4 * 496}]
    assert d["need"] == 1080 * 4 * 496
    # the automatic rule: launches of two or more jobs
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)])["need"] == 0
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)] * 2)["need"] == 2 * 1080 * 4 * 496
    # a batch counts every job of a launch, MAX_JOBS = 32 at most
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)] * 16)["need"] == 16 * 1080 * 4 * 496
    assert _dump(1920, 1080, 1, -1, [(0, 68, 0)] * 40)["need"] == 32 * 1080 * 4 * 496
    # unequal stripes with halos: a job's rows are its resident ref rows
    jobs = [(0, 20, 0), (20, 45, 288), (45, 68, 688)]
    d = _dump(1920, 1080, 1, -1, jobs * 4)
    rows = [20 * 16 + 32, 45 * 16 + 32 - 288, 1080 - 688]
    assert [j["rows"] for j in d["jobs"]] == rows * 4
    assert d["need"] == 4 * sum(r * 4 * 496 for r in rows)
    for w in (320, 256, _padded_width(), 1920, 4096):
        d = _dump(w, 1088, 1, 1, [(0, 68, 0)] * 8)
        assert d["pitch"] % 16 == 0 and d["pitch"] >= (w + 64) // 4 and d["pitch"] < (w + 64) // 4 + 16
        assert all(j["bytes"] % 64 == 0 and j["bytes"] == j["rows"] * 4 * d["pitch"] for j in d["jobs"])


# ------------------------------------------------------------------ GPU: fields
def _padded_case():
    from motionestimation_amd import synth
    w = _padded_width()
    pairs = [synth.frame_pair(w, 136, 300 + f, *((5, -2) if f % 2 == 0 else (-9, 7))) for f in range(20)]
    return np.stack([r for r, _ in pairs]), np.stack([c for _, c in pairs])


@pytest.fixture(scope="module")
def oracle_fields(tmp_path_factory):
    """The oracle's fields of every case, computed once; saved for the children."""
    d = tmp_path_factory.mktemp("planes")
    out = {}
    for name in CASES + [PADDED]:
        ref, cur = _padded_case() if name == PADDED else _case(name)
        mv, co = [], []
        for r, c in zip(ref, cur):
            m, k, _ = O.full_search(r, c, B, S, "sad", threads=NT)
            mv.append(m)
            co.append(k)
        out[name] = (ref, cur, np.stack(mv), np.stack(co))
        np.savez(d / f"{name}.npz", ref=ref, cur=cur, mv=out[name][2], co=out[name][3])
    return d, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + [PADDED])
def test_product_fields_equal_oracle(engine, oracle_fields, name):
    ref, cur, omv, oco = oracle_fields[1][name]
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


@pytest.mark.gpu
def test_unequal_stripes_with_halos(engine):
    """One launch of 24 stripe jobs (6 frames of 320x400, block rows [0, 4),
    [4, 11), [11, 19), [19, 25): 750 tiles): plane rows count from each job's
    ref_row0 > 0, and the scratch holds jobs of unequal size."""
    import torch
    from motionestimation_amd import synth
    w, h, F = 320, 400, 6
    nbx, cuts = w // B, [0, 4, 11, 19, 25]
    jobs, want = [], []
    for f in range(F):
        ref, cur = synth.frame_pair(w, h, 500 + f, *((4, -5) if f % 2 else (-7, 3)))
        omv, oco, _ = O.full_search(ref, cur, B, S, "sad", threads=NT)
        for r0, r1 in zip(cuts, cuts[1:]):
            ry0, ry1 = max(0, r0 * B - S), min(h, r1 * B + S)
            rt = torch.from_numpy(ref[ry0:ry1].copy()).cuda()
            ct = torch.from_numpy(cur[r0 * B:min(h, r1 * B)].copy()).cuda()
            n = (r1 - r0) * nbx
            mv = torch.full((n, 2), -7, dtype=torch.int16, device="cuda")
            co = torch.zeros(n, dtype=torch.int32, device="cuda")
            jobs.append((rt, ry0, ct, r0 * B, r0, r1, mv, co))
            want.append((omv[r0 * nbx:r1 * nbx], oco[r0 * nbx:r1 * nbx]))
    assert any(j[1] > 0 for j in jobs) and len({j[0].shape[0] for j in jobs}) > 2
    run = engine.prepared_stripes_search(w, h, B, S, "sad", jobs)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    engine.device_check()
    for i, (j, (omv, oco)) in enumerate(zip(jobs, want)):
        np.testing.assert_array_equal(j[7].cpu().numpy().view(np.uint32), oco, err_msg=f"job {i} sad")
        np.testing.assert_array_equal(j[6].cpu().numpy(), omv, err_msg=f"job {i} mv")


@pytest.mark.gpu
def test_capture_without_warm_up_and_stale_graph(oracle_fields):
    """A SAD batch is captured on a fresh context (no scratch yet: it runs
    without planes, not ME_EINVAL) and replays to the oracle's fields; the run
    outside capture then grows the scratch for the planes, so the old graph is
    refused; a graph captured now points into the scratch and is refused once a
    larger batch regrows it."""
    import ctypes
    import torch
    import motionestimation_amd as me
    ref, cur, omv, oco = oracle_fields[1]["shifts"]
    F, h, w = ref.shape
    nb = (w // B) * ((h + B - 1) // B)
    s = torch.cuda.Stream()
    sh = ctypes.c_void_p(s.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(s):
        ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
        co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
        run = eng.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co,
                                        stream=sh)

        def check_fields(what):
            torch.cuda.synchronize()
            eng.device_check()
            np.testing.assert_array_equal(co.cpu().numpy().view(np.uint32).reshape(F, nb), oco, err_msg=what)
            np.testing.assert_array_equal(mv.cpu().numpy().reshape(F, nb, 2), omv, err_msg=what)
            mv.fill_(-7)
            co.zero_()

        g0 = eng.capture(sh, run)  # nothing has run on this context
        for _ in range(2):
            g0.launch(sh)
        check_fields("graph captured without scratch")
        run()  # sizes the scratch for the planes
        check_fields("direct")
        with pytest.raises(me.MEError) as ei:
            g0.launch(sh)
        assert ei.value.status == me._lib.ME_EINVAL
        g1 = eng.capture(sh, run)  # with planes
        for _ in range(2):
            g1.launch(sh)
        check_fields("graph captured with planes")
        # a larger batch (twice the frames) regrows the scratch g1 points into
        ref2, cur2 = torch.cat([ref_t, ref_t]), torch.cat([cur_t, cur_t])
        mv2 = torch.empty((2 * F * nb, 2), dtype=torch.int16, device="cuda")
        co2 = torch.empty(2 * F * nb, dtype=torch.int32, device="cuda")
        eng.search_batch_device(ref2, 0, cur2, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv2, co2, stream=sh)
        torch.cuda.synchronize()
        eng.device_check()
        np.testing.assert_array_equal(mv2.cpu().numpy().reshape(2 * F, nb, 2), np.concatenate([omv, omv]))
        with pytest.raises(me.MEError) as ei:
            g1.launch(sh)
        assert ei.value.status == me._lib.ME_EINVAL


# ------------------------------------------------------------ GPU: tuning build
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import motionestimation_amd as me
assert me._lib.LIB_PATH.endswith("libme_hip_tune.so"), me._lib.LIB_PATH
L = me._lib.lib()
L.me_debug_prune_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
L.me_debug_prune_stats.restype = ctypes.c_int
B, S = 16, 32
stats = {{}}
with me.Engine() as eng:
    for name in {cases!r}:
        z = np.load({data!r} + "/" + name + ".npz")
        ref, cur = z["ref"], z["cur"]
        F, h, w = ref.shape
        nb = (w // B) * ((h + B - 1) // B)
        ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
        co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
        eng.search_batch_device(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
        torch.cuda.synchronize()
        eng.device_check()
        out = (ctypes.c_uint32 * 4)()
        assert L.me_debug_prune_stats(eng._h, out) == 0
        stats[name] = list(out)
        assert np.array_equal(co.cpu().numpy().view(np.uint32).reshape(F, nb), z["co"]), name + " sad"
        assert np.array_equal(mv.cpu().numpy().reshape(F, nb, 2), z["mv"]), name + " mv"
print("STATS " + json.dumps(stats))
print("planes ok")
"""

MODES = {
    "verify_planes": {"ME_PRUNE": "2", "ME_PRUNE_PLANES": "1"},
    "slots4_planes": {"ME_PRUNE": "1", "ME_FLOW_SLOTS": "4", "ME_PRUNE_PLANES": "1"},
    "planes_off": {"ME_PRUNE_PLANES": "0"},
    "planes_on": {"ME_PRUNE_PLANES": "1"},
}
_child_stats = {}


def _run_child(mode, data_dir, tmp_path):
    """The child of `mode`, run once per session: every case equals the oracle
    there (asserted in the child); returns its counts per case."""
    if mode not in _child_stats:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        script = tmp_path / f"planes_child_{mode}.py"
        script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cases=CASES + [PADDED],
                                        data=str(data_dir)))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        env.update(MODES[mode])
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "planes ok" in r.stdout
        _child_stats[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
    return _child_stats[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["verify_planes", "slots4_planes", "planes_off"])
def test_tuning_build_modes_equal_oracle(oracle_fields, tmp_path, mode):
    """ME_PRUNE=2 with planes (a wrongly dead lane-task fails me_device_check),
    ME_PRUNE=1 ME_FLOW_SLOTS=4 with planes (refills and ring reuse) and
    ME_PRUNE_PLANES=0: every case equals the oracle, every item was bounded."""
    stats = _run_child(mode, oracle_fields[0], tmp_path)
    for name in CASES + [PADDED]:
        live, total, bypassed, items = stats[name]
        F, h, w = oracle_fields[1][name][0].shape
        assert items == F * ((h + B - 1) // B) * ((w // B + 3) // 4), (name, stats[name])  # 4-block tiles
        assert 0 < live <= total, (name, stats[name])
    assert stats["shifts"][0] < stats["shifts"][1] // 2, stats["shifts"]  # heavy pruning


@pytest.mark.gpu
def test_counts_equal_with_planes_on_and_off(oracle_fields, tmp_path):
    """Same q, same lists: live and total lane-tasks are equal between the
    planes and the in-kernel box sums, in every mode, for every case."""
    off = _run_child("planes_off", oracle_fields[0], tmp_path)
    for mode in ("planes_on", "verify_planes", "slots4_planes"):
        on = _run_child(mode, oracle_fields[0], tmp_path)
        for name in CASES + [PADDED]:
            print(mode, name, "on", on[name], "off", off[name])
            assert on[name][:2] == off[name][:2], (mode, name, on[name], off[name])
