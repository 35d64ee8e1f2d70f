"""The flow kernel's candidate pruning: SAD fields stay the exhaustive search's.

me_flow_kernel<16, 13, 144> skips a lane-task (52 candidates of one block) only
when the sub-block bound proves every valid candidate in it strictly worse than
a seed candidate of the block (csrc/me_kernels.hip, flow_bound):

    q(.)  = 4x4 box sum >> 4                      (16 sub-blocks per 16x16 block)
    LB    = 16 * sum_sb |q(cur_sb) - q(ref_sb)| - 240   <=   SAD

`lower_bound()` below is the numpy statement of that bound; the CPU test checks
LB <= SAD for every valid candidate of the small synthetic fixtures.  The GPU
cases are batches of small frames that get the flow plan (+-32, width % 16 == 0,
>= 512 tiles: 20 frames of 320x136 -> 900 tiles with the h = 8 bottom row, 32
frames of 256x64 -> 512 tiles, every window clamped), compared field for field
with the oracle's full search per frame (src/cpu/main.c:39-82 restated), in the
product build and, in child processes, on the tuning build with ME_PRUNE=2
(verify), ME_PRUNE=1 ME_FLOW_SLOTS=4 (refills and ring reuse) and ME_PRUNE=0.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from motionestimation_amd import synth

NT = min(16, os.cpu_count() or 1)
S, B = 32, 16


# ------------------------------------------------------------------ the bound
def box_q(a):
    """q at every position: (sum of the 4x4 box whose top-left is (y, x)) >> 4."""
    a = a.astype(np.int32)
    c = np.pad(a, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
    return (c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4]) >> 4


def lower_bound(qref, qcur, x, y, bx, by):
    """LB of candidate top-left (x, y) of ref for the block at (bx, by) of cur."""
    r = qref[y:y + 16:4, x:x + 16:4]
    c = qcur[by:by + 16:4, bx:bx + 16:4]
    return 16 * int(np.abs(r - c).sum()) - 240


def _fixture_pairs():
    out = []
    for name, (w, h) in [("syn_contrast_96x96", (96, 96)), ("syn_noise_100x75", (100, 75)),
                         ("syn_stripes_80x60", (80, 60)), ("syn_translate_128x96", (128, 96))]:
        d = os.path.join(O.REPO, "tests", "golden", "frames")
        ref = np.fromfile(os.path.join(d, name + "_ref.yuv"), np.uint8)[:w * h].reshape(h, w)
        cur = np.fromfile(os.path.join(d, name + "_cur.yuv"), np.uint8)[:w * h].reshape(h, w)
        out.append((name, ref, cur))
    return out


@pytest.mark.parametrize("name,ref,cur", _fixture_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_bound_never_exceeds_sad(name, ref, cur):
    """LB <= SAD for every valid +-32 candidate of every full 16x16 block."""
    h, w = ref.shape
    qref, qcur = box_q(ref), box_q(cur)
    win = np.lib.stride_tricks.sliding_window_view(ref.astype(np.int16), (B, B))
    checked = 0
    for by in range(0, h - B + 1, B):
        for bx in range(0, w - B + 1, B):
            y0, y1 = max(by - S, 0), min(by + S, h - B)
            x0, x1 = max(bx - S, 0), min(bx + S, w - B)
            blk = cur[by:by + B, bx:bx + B].astype(np.int16)
            sad = np.abs(win[y0:y1 + 1, x0:x1 + 1] - blk).sum((2, 3))
            qc = qcur[by:by + B:4, bx:bx + B:4]
            lb = np.zeros_like(sad)
            for sy in range(4):
                for sx in range(4):
                    lb += np.abs(qref[y0 + 4 * sy:y1 + 4 * sy + 1, x0 + 4 * sx:x1 + 4 * sx + 1] - qc[sy, sx])
            lb = 16 * lb - 240
            assert (lb <= sad).all(), (name, bx, by)
            # the scalar statement agrees with the vectorised one
            assert lower_bound(qref, qcur, x0, y0, bx, by) == lb[0, 0]
            checked += sad.size
    assert checked > 0


# ------------------------------------------------------------------ the cases
def _stack(pairs):
    return np.stack([r for r, _ in pairs]), np.stack([c for _, c in pairs])


def _case(name):
    """(ref [F, h, w], cur [F, h, w]) of a named case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "clamped_256x64":
        F, h, w = 32, 64, 256
    elif name == "noise":  # 1,440 tiles: 5 to 6 items per workgroup, so the bypass gets its run of 4
        F, h, w = 32, 136, 320
    else:
        F, h, w = 20, 136, 320
    if name in ("shifts", "clamped_256x64"):
        return _stack([synth.frame_pair(w, h, 100 + f, *((3, -3) if f % 2 == 0 else (-6, 4))) for f in range(F)])
    if name == "flat":
        a = np.full((F, h, w), 128, np.uint8)
        a[1::2] = np.arange(1, F, 2, dtype=np.uint8)[:, None, None]  # other levels, 0 included
        return a, a.copy()
    if name == "noise":
        return (rng.integers(0, 256, (F, h, w), dtype=np.uint8), rng.integers(0, 256, (F, h, w), dtype=np.uint8))
    if name == "fold_corners":
        # winners at dx = +32 (the fold column), dx = -32 and the four window corners
        sh = [(32, 0), (-32, 0), (32, 32), (-32, -32), (32, -32), (-32, 32), (0, 32), (0, -32), (32, 5), (32, -7)]
        pairs = []
        for f in range(F):
            ref = synth._box5(rng.integers(0, 256, (h, w), dtype=np.uint8))
            sx, sy = sh[f % len(sh)]
            pairs.append((ref, np.ascontiguousarray(synth.shift_plane(ref, -sx, -sy))))
        return _stack(pairs)
    if name == "stripes_checker":
        yy, xx = np.mgrid[0:h, 0:w]
        stripes = np.where((xx % 8) < 4, 40, 210).astype(np.uint8)
        chk8 = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0, 255).astype(np.uint8)
        chk1 = np.where((xx + yy) % 2 == 0, 0, 255).astype(np.uint8)
        chk4 = np.where(((xx // 4) + (yy // 4)) % 2 == 0, 0, 255).astype(np.uint8)
        pats = [stripes, chk8, chk1, chk4]
        ref = np.stack([pats[f % 4] for f in range(F)])
        cur = np.stack([np.ascontiguousarray(synth.shift_plane(pats[f % 4], f % 3, (f // 4) % 3)) for f in range(F)])
        return ref, cur
    raise KeyError(name)


CASES = ["shifts", "flat", "noise", "fold_corners", "stripes_checker", "clamped_256x64"]
TILES = {"clamped_256x64": 512, "noise": 1440}  # every other case: 900 (5 tiles x 9 block rows x 20 frames)


@pytest.fixture(scope="module")
def oracle_fields(tmp_path_factory):
    """The oracle's fields of every case, computed once; also saved for the
    child processes (one .npz per case)."""
    d = tmp_path_factory.mktemp("prune")
    out = {}
    for name in CASES:
        ref, cur = _case(name)
        mv, co = [], []
        for r, c in zip(ref, cur):
            m, k, _ = O.full_search(r, c, B, S, "sad", threads=NT)
            mv.append(m)
            co.append(k)
        out[name] = (ref, cur, np.stack(mv), np.stack(co))
        np.savez(d / f"{name}.npz", ref=ref, cur=cur, mv=out[name][2], co=out[name][3])
    return d, out


def _search(engine, ref, cur):
    import torch
    F, h, w = ref.shape
    nb = (w // B) * ((h + B - 1) // B)
    ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
    mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
    co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
    run = engine.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
    for _ in range(2):  # the same buffers rewritten
        run()
    torch.cuda.synchronize()
    engine.device_check()
    return mv.cpu().numpy().reshape(F, nb, 2), co.cpu().numpy().view(np.uint32).reshape(F, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_pruned_fields_equal_oracle(engine, oracle_fields, name):
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
print("prune ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["verify", "slots4", "off"])
def test_tuning_build_modes(oracle_fields, tmp_path, mode):
    """ME_PRUNE=2 (every lane-task runs; a wrongly dead one fails
    me_device_check), ME_PRUNE=1 with a ring of 4 slots, and ME_PRUNE=0; the
    counts show the pruning kernel took every item (or none with ME_PRUNE=0),
    thinned the correlated content and bypassed the bound on noise."""
    import json
    lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
    assert os.path.exists(lib), "build with __graft_entry__.build()"
    script = tmp_path / "prune_child.py"
    script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), cases=CASES,
                                    data=str(oracle_fields[0])))
    env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
    env.update({"verify": {"ME_PRUNE": "2"}, "slots4": {"ME_PRUNE": "1", "ME_FLOW_SLOTS": "4"},
                "off": {"ME_PRUNE": "0"}}[mode])
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prune ok" in r.stdout
    stats = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][0][6:])
    for name in CASES:
        live, total, bypassed, items = stats[name]
        if mode == "off":
            assert items == 0, (name, stats[name])
            continue
        assert items == TILES.get(name, 900), (name, stats[name])
        assert 0 < live <= total
        if name == "shifts":
            assert live < total // 2, (name, stats[name])  # heavy pruning
        if name == "noise" and mode == "slots4":
            assert bypassed > 0, (name, stats[name])
