"""The flow kernel's row split of a pruned item's partial wave-task.

A wave-task of me_flow_kernel<16, 13, 144> that holds n <= 32 entries of a
pruned item's live list runs with P = 4 (n <= 16) or P = 2 lanes per entry, each
lane taking a run of the entry's 13 dy rows (csrc/me_geom.h flow_split_*,
csrc/me_kernels.hip flow_split_task): rows [0,4) [3,7) [6,10) [9,13) for P = 4,
[0,7) [6,13) for P = 2, the fold column (dx = +32) in part 0.  The fields must
stay the exhaustive search's, bit for bit: every case is compared with
oracle_lib.full_search per frame (src/cpu/main.c:39-82 restated).

Shapes as in test_gpu_sad_prune.py (the flow plan needs >= 512 tiles): 20 frames
of 320x136 at +-32 (900 tiles with the h = 8 bottom row, whose items are never
split), 32 frames of 256x64 (every dy range clipped).

  dy_sweep  smooth content (nearly every task has n <= 16); the halves of every
            frame are displaced by their own (dx, dy): the 40 dy + 32 values put
            a winner on every row 0..12 of a chunk in three different chunks
            (so on every part seam: rows 3, 6, 9, 12 of P = 4, row 6 of P = 2)
            and on dy = +-32; per row one half has dx = +32 (the fold column),
            one dx = -32.
  mixed     the smooth plane blended with uniform noise of growing amplitude:
            list lengths from a few entries to full, so tasks of all three
            classes run (counted in the tuning build's child).  The amplitudes
            were chosen on the CPU with the numpy bound of test_gpu_sad_prune.py
            (box_q): per item the lane-tasks with 16 * minlb - 240 <= U_b.
  clamped_256x64, flat   test_gpu_sad_prune's: jlo / jhi cut into the parts; every
            tie goes to the first candidate in raster order.
The 320x136 cases' top and bottom block rows have lc0 > 0 and partial chunks.

Child processes on libme_hip_tune.so: ME_PRUNE_SPLIT=0 (no task split, same
fields), =1 (tasks split four ways on dy_sweep, all three classes on mixed),
ME_PRUNE=2 (verify: me_device_check stays clean) and ME_FLOW_SLOTS=4 (ring reuse).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from motionestimation_amd import synth
from test_gpu_sad_prune import _case, _search

NT = min(16, os.cpu_count() or 1)
S, B = 32, 16
F, H, W = 20, 136, 320

# mixed: noise weight (of 256) of frame f
# mixed: noise weight (of 256) of frame f.  CPU estimate of the full-height items'
# median list length (of 320): 4 up to weight 12, 9..15 at 16..19, 22..54 at
# 20..24, 76 at 26, 129 at 28, 162 at 32, 252 at 40, 292 from 64; over the case
# about 1,000 tasks with n > 32, 140 with 16 < n <= 32 (most at weights 17..24),
# 350 with n <= 16.
MIXED_AMPL = [0, 4, 8, 12, 14, 16, 17, 18, 19, 20, 21, 22, 23, 24, 26, 28, 32, 40, 64, 256]


def _sweep_shifts():
    """40 (dx, dy): dy + 32 = r + 13 c for every row r in three chunks c (39
    values, 0 and 64 among them) and dy = 0; dx = +32 / -32 / other per row."""
    other = [0, 5, -7, 17, -20, 31, -31, 1, -1, 12, -13, 3, -9]
    out = []
    for r in range(13):
        for k, c in enumerate(sorted({r % 5, (r + 2) % 5, (r + 4) % 5})):
            out.append(((32, -32, other[r])[(k + r) % 3], r + 13 * c - 32))
    out.append((0, 0))
    assert len(out) == 40 and {dy for _, dy in out} >= {-32, 32}
    return out


def split_case(name):
    """(ref [F, h, w], cur [F, h, w]) of a named case."""
    if name in ("clamped_256x64", "flat"):
        return _case(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    refs, curs = [], []
    if name == "dy_sweep":
        sh = _sweep_shifts()
        for f in range(F):
            ref = synth._box5(rng.integers(0, 256, (H, W), dtype=np.uint8))
            cur = np.empty_like(ref)
            for half, (sx, sy) in enumerate(sh[2 * f:2 * f + 2]):  # cur[y, x] = ref[y + sy, x + sx]
                cols = slice(half * W // 2, (half + 1) * W // 2)
                cur[:, cols] = synth.shift_plane(ref, -sx, -sy)[:, cols]
            refs.append(ref)
            curs.append(cur)
        return np.stack(refs), np.stack(curs)
    if name == "mixed":
        for f in range(F):
            ref = synth._box5(rng.integers(0, 256, (H, W), dtype=np.uint8))
            a = MIXED_AMPL[f]  # cur = the displaced smooth plane with a / 256 of noise of its own
            cur = synth.shift_plane(ref, *((3, -3) if f % 2 == 0 else (-6, 4))).astype(np.int32)
            cur = ((256 - a) * cur + a * rng.integers(0, 256, (H, W))) >> 8
            refs.append(ref)
            curs.append(np.ascontiguousarray(cur.astype(np.uint8)))
        return np.stack(refs), np.stack(curs)
    raise KeyError(name)


CASES = ["dy_sweep", "mixed", "clamped_256x64", "flat"]


@pytest.fixture(scope="module")
def oracle_fields(tmp_path_factory):
    """The oracle's fields of every case, computed once; also saved for the
    child processes (one .npz per case)."""
    d = tmp_path_factory.mktemp("split")
    out = {}
    for name in CASES:
        ref, cur = split_case(name)
        mv, co = [], []
        for r, c in zip(ref, cur):
            m, k, _ = O.full_search(r, c, B, S, "sad", threads=NT)
            mv.append(m)
            co.append(k)
        out[name] = (ref, cur, np.stack(mv), np.stack(co))
        np.savez(d / f"{name}.npz", ref=ref, cur=cur, mv=out[name][2], co=out[name][3])
    return d, out


def test_sweep_reaches_every_row_and_seam(oracle_fields):
    """The dy sweep's winners (the oracle's) sit on every row of a chunk in at
    least two chunks, with dx = +32 on every P = 4 seam row and dx = -32 present."""
    _, _, omv, _ = oracle_fields[1]["dy_sweep"]
    dx, y = omv[..., 0].ravel().astype(int), omv[..., 1].ravel().astype(int) + S
    for r in range(13):
        assert len({int(v) // 13 for v in y[y % 13 == r]}) >= 2, r
    assert {0, 2 * S} <= set(y.tolist())
    for r in (3, 5, 6, 7, 9, 12):
        assert ((dx == S) & (y % 13 == r)).any(), r
    assert (dx == -S).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_split_fields_equal_oracle(engine, oracle_fields, name):
    ref, cur, omv, oco = oracle_fields[1][name]
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import motionestimation_amd as me
assert me._lib.LIB_PATH.endswith("libme_hip_tune.so"), me._lib.LIB_PATH
L = me._lib.lib()
L.me_debug_prune_split_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
L.me_debug_prune_split_stats.restype = ctypes.c_int
B, S = 16, 32
stats = {{}}
with me.Engine() as eng:
    out = (ctypes.c_uint32 * 3)()
    assert L.me_debug_prune_split_stats(eng._h, out) == 0
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
        assert L.me_debug_prune_split_stats(eng._h, out) == 0
        stats[name] = list(out)
        assert np.array_equal(co.cpu().numpy().view(np.uint32).reshape(F, nb), z["co"]), name + " sad"
        assert np.array_equal(mv.cpu().numpy().reshape(F, nb, 2), z["mv"]), name + " mv"
print("STATS " + json.dumps(stats))
print("split ok")
"""

_MODES = {"off": {"ME_PRUNE_SPLIT": "0"}, "on": {"ME_PRUNE_SPLIT": "1"}, "verify": {"ME_PRUNE": "2"},
          "slots4": {"ME_PRUNE_SPLIT": "1", "ME_FLOW_SLOTS": "4"}}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(_MODES))
def test_tuning_build_split_modes(oracle_fields, tmp_path, mode):
    """Every mode: the oracle's fields and a clean me_device_check on every
    case.  The executed wave-tasks by class [P = 1, P = 2, P = 4] show the
    switch is obeyed and that the cases run what they are meant to."""
    lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
    assert os.path.exists(lib), "build with __graft_entry__.build()"
    script = tmp_path / "split_child.py"
    script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cases=CASES,
                                    data=str(oracle_fields[0])))
    env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
    for k in ("ME_PRUNE", "ME_PRUNE_SPLIT", "ME_FLOW_SLOTS"):
        env.pop(k, None)
    env.update(_MODES[mode])
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "split ok" in r.stdout
    stats = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
    print(mode, stats)
    for name in CASES:
        p1, p2, p4 = stats[name]
        assert p1 + p2 + p4 > 0, (name, stats[name])
        if name in ("dy_sweep", "mixed"):
            assert p1 > 0, (name, stats[name])  # the h = 8 bottom row's items are never split
        if mode == "off":
            assert p2 == 0 and p4 == 0, (name, stats[name])
    if mode in ("on", "slots4"):
        assert stats["dy_sweep"][2] > 0, stats["dy_sweep"]
        assert all(v > 0 for v in stats["mixed"]), stats["mixed"]
