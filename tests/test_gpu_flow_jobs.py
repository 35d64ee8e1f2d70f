"""The flow kernel finds an item's job without scanning the job table from job 0.

me_flow_kernel's launch holds every job's tiles, job-major; a wave finds its
first item's job by bisection and every later item's, and every refill
target's, from the job of the item before (csrc/me_geom.h flow_job_find /
flow_job_from; tests/test_flow_job_lookup.py checks the rule itself on the
CPU).  An item given the wrong job reads another job's planes and writes
another job's records, so here every job's fields are compared bit for bit
with oracle_lib.full_search of the same rows (src/cpu/main.c:39-82 restated),
on records pre-filled with -7.  Every frame has a displacement of its own.

The flow plan needs >= 512 tiles at +-32, B = 16 (tests/test_gpu_flow_split.py);
a workgroup's items are 32 tiles apart inside its band (256 workgroups, 8 bands).

  uniform32      32 frames of 256x64 (test_gpu_sad_prune's refs), 16 tiles each,
                 one search_batch_device call; frame f searched alone must
                 equal slice f of the batch.
  nonuniform32   32 stripes of four 320x440 frames in one
                 prepared_stripes_search call, 5 tiles per block row, block-row
                 counts ROWS32 (1-row jobs in runs of one to six, jobs of up to
                 28 rows, some on the h = 8 bottom row): 2,275 tiles, 8 to 9
                 items per workgroup, so the product's 6-slot ring refills.
                 Between one item and the next (+32 tiles) a workgroup crosses
                 0 (inside the 20- to 28-row jobs), 1 and up to 6 job
                 boundaries (the runs of 1-row jobs, 5 tiles each); between an
                 item and its refill target (+192 tiles) 1 to 7
                 (test_nonuniform_walk_crosses_zero_one_and_several computes
                 both on the CPU from the progression rule).
  two_jobs, three_jobs   28 + 27 and 19 + 19 + 18 block rows of 640x440 frames
                 (10 tiles per row): one count away from equal counts.
  bottom_rows20  test_gpu_sad_prune's 20 frames of 320x136: the h = 8 bottom
                 row's items are unpruned and their lists full.

Child processes on libme_hip_tune.so run every case with ME_PRUNE=2 (verify:
me_device_check stays clean), ME_FLOW_SLOTS=4 (ring reuse with refills) and
ME_PRUNE=0 (the unpruned instance shares the lookup); the pruning counts show
the flow kernel took every tile.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from motionestimation_amd import synth

NT = min(16, os.cpu_count() or 1)
S, B = 32, 16

# nonuniform32: block rows of job j (of a 28-row frame; frame j % 4)
ROWS32 = [1, 1, 1, 1, 1, 1, 28, 20, 1, 27, 2, 24, 26, 1, 1, 1, 28, 3, 22, 28, 28, 1, 1, 26, 5, 25, 21, 28, 23, 27, 28, 24]
assert len(ROWS32) == 32 and sum(ROWS32) == 455 and max(ROWS32) == 28


def _nonuniform_jobs():
    """(frame, r0, r1) of job j: rows anywhere in the frame, every third 1-row
    job on the h = 8 bottom row (row 27), the others spread from row 0 on."""
    jobs = []
    for j, n in enumerate(ROWS32):
        r0 = 27 if n == 1 and j % 3 == 0 else (5 * j) % (28 - n + 1)
        jobs.append((j % 4, r0, r0 + n))
    return jobs


def _frames(w, h, seed0, n):
    """n (ref, cur) pairs, frame f displaced by its own (dx, dy)."""
    pairs = [synth.frame_pair(w, h, seed0 + f, ((7 * f + 3) % 33) - 16, ((5 * f) % 15) - 7) for f in range(n)]
    assert len({(((7 * f + 3) % 33) - 16, ((5 * f) % 15) - 7) for f in range(n)}) == n
    return np.stack([r for r, _ in pairs]), np.stack([c for _, c in pairs])


def _whole(F, nby):
    return [(f, 0, nby) for f in range(F)]


# name -> (frame set, api, jobs [(frame, r0, r1)])
CASES = {
    "uniform32": ("f256x64", "batch", _whole(32, 4)),
    "nonuniform32": ("f320x440", "stripes", _nonuniform_jobs()),
    "two_jobs": ("f640x440", "stripes", [(0, 0, 28), (1, 0, 27)]),
    "three_jobs": ("f640x440", "stripes", [(0, 0, 19), (1, 4, 23), (2, 10, 28)]),
    "bottom_rows20": ("f320x136", "batch", _whole(20, 9)),
}


def frame_set(name):
    if name == "f256x64":
        return _frames(256, 64, 100, 32)  # (the refs of test_gpu_sad_prune._case("clamped_256x64"))
    if name == "f320x440":
        return _frames(320, 440, 300, 4)
    if name == "f640x440":
        return _frames(640, 440, 400, 3)
    if name == "f320x136":
        from test_gpu_sad_prune import _case
        return _case("shifts")
    raise KeyError(name)


def case_tiles(name):
    fs, _, jobs = CASES[name]
    w = int(fs[1:].split("x")[0])
    return [(w // B + 3) // 4 * (r1 - r0) for _, r0, r1 in jobs]


def run_case(eng, name, ref, cur):
    """Per job (mv [rows * nbx, 2], cost [rows * nbx]) of one call of the case's entry point."""
    import torch
    _, api, jobs = CASES[name]
    F, h, w = ref.shape
    nbx, nby = w // B, (h + B - 1) // B
    ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
    if api == "batch":
        assert jobs == _whole(F, nby)
        mv = torch.full((F * nbx * nby, 2), -7, dtype=torch.int16, device="cuda")
        co = torch.zeros(F * nbx * nby, dtype=torch.int32, device="cuda")
        eng.search_batch_device(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, nby, mv, co)
        torch.cuda.synchronize()
        eng.device_check()
        mv, co = mv.cpu().numpy().reshape(F, -1, 2), co.cpu().numpy().view(np.uint32).reshape(F, -1)
        return [(mv[f], co[f]) for f in range(F)]
    outs = [(torch.full(((r1 - r0) * nbx, 2), -7, dtype=torch.int16, device="cuda"),
             torch.zeros((r1 - r0) * nbx, dtype=torch.int32, device="cuda")) for _, r0, r1 in jobs]
    run = eng.prepared_stripes_search(w, h, B, S, "sad", [(ref_t[f], 0, cur_t[f], 0, r0, r1, m, c)
                                                           for (f, r0, r1), (m, c) in zip(jobs, outs)])
    run()
    torch.cuda.synchronize()
    eng.device_check()
    return [(m.cpu().numpy(), c.cpu().numpy().view(np.uint32)) for m, c in outs]


def check_case(name, got, ref, omv, oco):
    """Every job's records against the oracle's rows of its frame."""
    _, _, jobs = CASES[name]
    nbx = ref.shape[2] // B
    assert len(got) == len(jobs)
    for j, ((f, r0, r1), (mv, co)) in enumerate(zip(jobs, got)):
        np.testing.assert_array_equal(co, oco[f][r0 * nbx:r1 * nbx], err_msg=f"{name} job {j} sad")
        np.testing.assert_array_equal(mv, omv[f][r0 * nbx:r1 * nbx], err_msg=f"{name} job {j} mv")


@pytest.fixture(scope="module")
def oracle_fields(tmp_path_factory):
    """The oracle's fields of every frame set, computed once; also saved for
    the child processes (one .npz per set)."""
    d = tmp_path_factory.mktemp("flow_jobs")
    out = {}
    for fs in sorted({c[0] for c in CASES.values()}):
        ref, cur = frame_set(fs)
        fields = [O.full_search(r, c, B, S, "sad", threads=NT)[:2] for r, c in zip(ref, cur)]
        out[fs] = (ref, cur, np.stack([m for m, _ in fields]), np.stack([k for _, k in fields]))
        np.savez(d / f"{fs}.npz", ref=ref, cur=cur, mv=out[fs][2], co=out[fs][3])
    return d, out


def test_cases_take_the_flow_plan():
    """>= 512 tiles each (2 per CU of 256: plan_flow's floor), at most 32 jobs."""
    for name in CASES:
        t = case_tiles(name)
        assert sum(t) >= 512 and len(t) <= 32, (name, sum(t))
    assert len(set(case_tiles("uniform32"))) == 1 and len(case_tiles("uniform32")) == 32
    assert case_tiles("two_jobs") == [280, 270] and case_tiles("three_jobs") == [190, 190, 180]
    assert sorted(set(case_tiles("nonuniform32")))[0] == 5 and sum(case_tiles("nonuniform32")) == 2275


def test_nonuniform_walk_crosses_zero_one_and_several():
    """What the docstring says of nonuniform32, from the kernel's progression
    rule at 256 workgroups: job boundaries crossed from item to item and from
    an item to its refill target (6 slots ahead)."""
    tiles = case_tiles("nonuniform32")
    job = np.repeat(np.arange(32), tiles)
    nwg, nb, ntiles = 256, 6, len(job)
    step, refill, items = set(), set(), []
    for bid in range(nwg):
        x, m = bid % 8, bid // 8
        t = np.arange(ntiles * x // 8 + m, ntiles * (x + 1) // 8, nwg // 8)
        items.append(len(t))
        step |= set((job[t[1:]] - job[t[:-1]]).tolist())
        refill |= set((job[t[nb:]] - job[t[:-nb]]).tolist())
    assert (min(items), max(items)) == (8, 9)
    assert {0, 1, 2} <= step and max(step) == 6
    assert (min(refill), max(refill)) == (1, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_job_fields_equal_oracle(engine, oracle_fields, name):
    ref, cur, omv, oco = oracle_fields[1][CASES[name][0]]
    check_case(name, run_case(engine, name, ref, cur), ref, omv, oco)


@pytest.mark.gpu
def test_frame_alone_equals_its_slice_of_the_batch(engine, oracle_fields):
    import torch
    ref, cur, _, _ = oracle_fields[1]["f256x64"]
    batch = run_case(engine, "uniform32", ref, cur)
    n = (256 // B) * (64 // B)
    for f in range(32):
        mv = torch.full((n, 2), -7, dtype=torch.int16, device="cuda")
        co = torch.zeros(n, dtype=torch.int32, device="cuda")
        engine.full_search_device(torch.from_numpy(ref[f]).cuda(), torch.from_numpy(cur[f]).cuda(), B, S, "sad", mv, co)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mv.cpu().numpy(), batch[f][0], err_msg=f"frame {f} mv")
        np.testing.assert_array_equal(co.cpu().numpy().view(np.uint32), batch[f][1], err_msg=f"frame {f} sad")


_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch  # (before the library, as in the parent process: both bring a HIP runtime)
import motionestimation_amd as me
import test_gpu_flow_jobs as T
assert me._lib.LIB_PATH.endswith("libme_hip_tune.so"), me._lib.LIB_PATH
L = me._lib.lib()
L.me_debug_prune_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
L.me_debug_prune_stats.restype = ctypes.c_int
stats = {{}}
with me.Engine() as eng:
    for name in T.CASES:
        z = np.load({data!r} + "/" + T.CASES[name][0] + ".npz")
        got = T.run_case(eng, name, z["ref"], z["cur"])
        out = (ctypes.c_uint32 * 4)()
        assert L.me_debug_prune_stats(eng._h, out) == 0
        stats[name] = list(out)
        T.check_case(name, got, z["ref"], z["mv"], z["co"])
print("STATS " + json.dumps(stats))
print("jobs ok")
"""

_MODES = {"verify": {"ME_PRUNE": "2"}, "slots4": {"ME_PRUNE": "1", "ME_FLOW_SLOTS": "4"}, "off": {"ME_PRUNE": "0"}}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(_MODES))
def test_tuning_build_modes(oracle_fields, tmp_path, mode):
    """Every case in a child on the tuning build: the oracle's fields, a clean
    me_device_check, and the pruning kernel's item count = the case's tiles
    (none with ME_PRUNE=0: the unpruned instance ran them)."""
    lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
    assert os.path.exists(lib), "build with __graft_entry__.build()"
    script = tmp_path / "jobs_child.py"
    script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), data=str(oracle_fields[0])))
    env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
    for k in ("ME_PRUNE", "ME_PRUNE_SPLIT", "ME_FLOW_SLOTS"):
        env.pop(k, None)
    env.update(_MODES[mode])
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "jobs ok" in r.stdout
    stats = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
    print(mode, stats)
    for name in CASES:
        live, total, bypassed, items = stats[name]
        assert items == (0 if mode == "off" else sum(case_tiles(name))), (name, stats[name])
        if mode != "off":
            assert 0 < live <= total, (name, stats[name])
