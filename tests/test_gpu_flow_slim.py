"""The pruning flow kernel's bound with plane loads from global memory.

In a launch with box-sum planes (two or more jobs) step 2 of flow_bound loads
its plane rows from the job's planes into registers (csrc/me_geom.h,
flow_plane_byte) and the slot carries the slim bound scratch: 10 ring slots at
the 144-byte pitch where the layout with the planes in LDS has 6.  Same box
sums, so the same live lists and the same fields: every test compares record
for record with the oracle's full search (tests/oracle_lib.py), and the tuning
build's live / total lane-task counts must be equal with the planes on and off.

Shapes: every window clamped in y (256x64), the h = 8 bottom row (320x136), a
width the flow plan does not take (200x96: no partial tile without W % 16 == 0)
next to one whose last tile has a single block (336x136), three unequal stripes
with halos (ref_row0 > 0; rows above and below the resident ones), a padded
stride, and two 1080p frames: 16 tiles per CU, the smallest product-build
launch that refills a 10-slot ring.
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
from test_gpu_sad_prune import B, NT, S, _case

CUTS = [0, 7, 19, 28]  # block rows of the three stripes of a 640x440 frame (28 rows, the last h = 8)


def _oracle(ref, cur):
    f = [O.full_search(r, c, B, S, "sad", threads=NT)[:2] for r, c in zip(ref, cur)]
    return np.stack([m for m, _ in f]), np.stack([k for _, k in f])


@functools.lru_cache(maxsize=None)
def _frames(name):
    """(ref [F, h, w], cur [F, h, w]) of a named case; content as in the
    pruning tests (displaced synthetic pairs) unless the name says otherwise."""
    if name in ("clamped_256x64", "shifts", "flat", "noise"):
        return _case(name)
    w, h, F = {"partial_336x136": (336, 136, 20), "small_200x96": (200, 96, 4), "stripes_640x440": (640, 440, 2),
               "stride_320x136": (320, 136, 20), "refill_1080p": (1920, 1080, 2)}[name]
    pairs = [synth.frame_pair(w, h, 700 + f, *((6, -4) if f % 2 == 0 else (-11, 9))) for f in range(F)]
    return np.stack([r for r, _ in pairs]), np.stack([c for _, c in pairs])


@pytest.fixture(scope="module")
def fields():
    """name -> (ref, cur, oracle mv, oracle cost), each computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            ref, cur = _frames(name)
            cache[name] = (ref, cur) + _oracle(ref, cur)
        return cache[name]
    return get


def _search(engine, ref, cur):
    """One batch launch over the frames, run twice into the same buffers."""
    import torch
    import motionestimation_amd as me
    F, h, w = ref.shape
    nb = me.num_blocks(w, h, B)  # (a partial last block column and row count)
    ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
    mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
    co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
    run = engine.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    engine.device_check()
    return mv.cpu().numpy().reshape(F, nb, 2), co.cpu().numpy().view(np.uint32).reshape(F, nb)


# ------------------------------------------------------- product build: fields
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["clamped_256x64", "shifts", "small_200x96", "partial_336x136", "refill_1080p",
                                  "flat", "noise"])
def test_batch_fields_equal_oracle(engine, fields, name):
    """clamped_256x64: 32 frames, every window clamped in y, all four corners.
    shifts: 320x136 x 20, the h = 8 row is not bounded and loads no planes.
    flat: every bound ties (equality is never pruned).  noise: the bypass
    engages and no planes are loaded in that state."""
    ref, cur, omv, oco = fields(name)
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


def _stripe_jobs(ref, cur):
    """Per frame three stripe jobs whose ref planes hold only the rows the
    stripe contract asks for (S rows of halo, cut at the frame)."""
    import torch
    F, h, w = ref.shape
    nbx = w // B
    jobs = []
    for f in range(F):
        for r0, r1 in zip(CUTS, CUTS[1:]):
            ry0, ry1 = max(0, r0 * B - S), min(h, r1 * B + S)
            rt = torch.from_numpy(ref[f, ry0:ry1].copy()).cuda()
            ct = torch.from_numpy(cur[f, r0 * B:min(h, r1 * B)].copy()).cuda()
            n = (r1 - r0) * nbx
            jobs.append((rt, ry0, ct, r0 * B, r0, r1, torch.full((n, 2), -7, dtype=torch.int16, device="cuda"),
                         torch.zeros(n, dtype=torch.int32, device="cuda")))
    return jobs


@pytest.mark.gpu
def test_unequal_stripes_with_halos(engine, fields):
    import torch
    ref, cur, omv, oco = fields("stripes_640x440")
    nbx = ref.shape[2] // B
    jobs = _stripe_jobs(ref, cur)
    assert any(j[1] > 0 for j in jobs) and len({j[0].shape[0] for j in jobs}) == 3
    assert sum((j[5] - j[4]) * ((nbx + 3) // 4) for j in jobs) >= 512  # the flow plan's floor
    run = engine.prepared_stripes_search(ref.shape[2], ref.shape[1], B, S, "sad", jobs)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    engine.device_check()
    for i, j in enumerate(jobs):
        f, (r0, r1) = i // 3, (j[4], j[5])
        np.testing.assert_array_equal(j[7].cpu().numpy().view(np.uint32), oco[f][r0 * nbx:r1 * nbx],
                                      err_msg=f"job {i} sad")
        np.testing.assert_array_equal(j[6].cpu().numpy(), omv[f][r0 * nbx:r1 * nbx], err_msg=f"job {i} mv")


@pytest.mark.gpu
def test_padded_stride(engine, fields):
    """Planes of 320 columns in rows of 384 bytes: the plane pitch follows the
    width, the window DMA the stride."""
    import torch
    ref, cur, omv, oco = fields("stride_320x136")
    F, h, w = ref.shape
    nb = (w // B) * ((h + B - 1) // B)
    rbuf = torch.full((F, h, 384), 255, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((F, h, 384), 255, dtype=torch.uint8, device="cuda")
    rbuf[:, :, :w] = torch.from_numpy(ref).cuda()
    cbuf[:, :, :w] = torch.from_numpy(cur).cuda()
    mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
    co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
    engine.search_batch_device(rbuf[:, :, :w], 0, cbuf[:, :, :w], 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
    torch.cuda.synchronize()
    engine.device_check()
    np.testing.assert_array_equal(co.cpu().numpy().view(np.uint32).reshape(F, nb), oco)
    np.testing.assert_array_equal(mv.cpu().numpy().reshape(F, nb, 2), omv)


# ------------------------------------------------------------ the tuning build
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
B, S, CUTS = 16, 32, {cuts!r}
z = np.load({data!r})
ref, cur, omv, oco = z["ref"], z["cur"], z["mv"], z["co"]
F, h, w = ref.shape
nbx = w // B
with me.Engine() as eng:
    jobs = []
    for f in range(F):
        for r0, r1 in zip(CUTS, CUTS[1:]):
            ry0, ry1 = max(0, r0 * B - S), min(h, r1 * B + S)
            rt = torch.from_numpy(ref[f, ry0:ry1].copy()).cuda()
            ct = torch.from_numpy(cur[f, r0 * B:min(h, r1 * B)].copy()).cuda()
            n = (r1 - r0) * nbx
            jobs.append((rt, ry0, ct, r0 * B, r0, r1, torch.full((n, 2), -7, dtype=torch.int16, device="cuda"),
                         torch.zeros(n, dtype=torch.int32, device="cuda")))
    eng.prepared_stripes_search(w, h, B, S, "sad", jobs)()
    torch.cuda.synchronize()
    eng.device_check()
    out = (ctypes.c_uint32 * 4)()
    assert L.me_debug_prune_stats(eng._h, out) == 0
    for i, j in enumerate(jobs):
        f, r0, r1 = i // 3, j[4], j[5]
        assert np.array_equal(j[7].cpu().numpy().view(np.uint32), oco[f][r0 * nbx:r1 * nbx]), "job %d sad" % i
        assert np.array_equal(j[6].cpu().numpy(), omv[f][r0 * nbx:r1 * nbx]), "job %d mv" % i
print("STATS " + json.dumps(list(out)))
print("slim ok")
"""

MODES = {
    "planes_on": {"ME_PRUNE_PLANES": "1"},
    "verify": {"ME_PRUNE": "2", "ME_PRUNE_PLANES": "1"},
    "slots2": {"ME_FLOW_SLOTS": "2", "ME_PRUNE_PLANES": "1"},
    "slots3": {"ME_FLOW_SLOTS": "3", "ME_PRUNE_PLANES": "1"},
    "planes_off": {"ME_PRUNE_PLANES": "0"},
    "split_off": {"ME_PRUNE_SPLIT": "0", "ME_PRUNE_PLANES": "1"},
}
_stats = {}


def _child(mode, fields, tmp_path_factory):
    """The three-stripe case in a child on the tuning build, once per mode:
    equal to the oracle there, me_device_check clean; returns [live, total,
    bypassed, items]."""
    if mode not in _stats:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        d = tmp_path_factory.mktemp("slim_" + mode)
        ref, cur, omv, oco = fields("stripes_640x440")
        np.savez(d / "case.npz", ref=ref, cur=cur, mv=omv, co=oco)
        script = d / "child.py"
        script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cuts=CUTS,
                                        data=str(d / "case.npz")))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        env.update(MODES[mode])
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "slim ok" in r.stdout
        _stats[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
    return _stats[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["verify", "slots2", "slots3", "planes_off", "split_off"])
def test_tuning_build_modes_equal_oracle(fields, tmp_path_factory, mode):
    """ME_PRUNE=2 (a wrongly dead lane-task fails me_device_check), rings of 2
    and 3 slots (reuse on a small launch), the layout without planes, and no
    row split: equal to the oracle, every full-height and h = 8 item counted."""
    live, total, bypassed, items = _child(mode, fields, tmp_path_factory)
    assert items == 2 * 28 * 10, (mode, live, total, bypassed, items)  # 640 / 64 tile columns x 28 block rows x 2
    assert 0 < live <= total
    if mode != "verify":
        assert live < total // 2, (mode, live, total)  # displaced synthetic content prunes heavily


@pytest.mark.gpu
def test_counts_equal_with_planes_on_and_off(fields, tmp_path_factory):
    off = _child("planes_off", fields, tmp_path_factory)
    for mode in ("planes_on", "slots2", "slots3", "split_off"):
        on = _child(mode, fields, tmp_path_factory)
        print(mode, "on", on, "off", off)
        assert on[:2] == off[:2], (mode, on, off)
