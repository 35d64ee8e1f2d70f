"""The row split over the whole wave: R = 1, 2, 3, 4 or 7 rows per lane.

A wave-task of a pruned h = 16 item with n <= 32 list entries left runs with
P = ceil(13 / R) lanes per entry, R chosen by n (csrc/me_geom.h flow_split_rows:
n <= 4 -> 1, <= 9 -> 2, <= 12 -> 3, <= 16 -> 4, <= 32 -> 7; more: the task runs
whole), instead of the earlier 4 lanes (n <= 16) or 2.  Nothing but the lanes'
share of an entry's 13 dy rows changes, so the fields must stay the oracle's
full search (tests/oracle_lib.py, src/cpu/main.c:39-82 restated) bit for bit,
under the rule and under the earlier one (the tuning build's ME_PRUNE_SPLIT=2),
and the live lane-task counts must be equal between the two.

Shapes: the smallest batches the flow plan takes with pruning and box-sum planes
(two or more jobs, width % 64 == 0 so every tile has 4 blocks at the 144-byte
pitch, +-32, B = 16, 512 tiles or more: two per CU of 256):
  graded_256x64   32 jobs, 512 full-height tiles, every dy range clamped at the
                  top and at the bottom (lc0 > 0, partial chunks: jlo / jhi cut
                  into the parts).
  mixed           test_gpu_flow_split's: 20 jobs of 320x136, 900 tiles with the
                  h = 8 bottom row (never split) and dy clamped in the top and
                  bottom block rows.
  bypass_bands    test_gpu_flow_prebound's: 32 jobs of 320x136, noise and
                  shifted pairs in groups of two, for the 8-workgroup mode.
Content of the first two: a displaced smooth plane blended with uniform noise
whose weight grows from frame to frame, the weights of test_gpu_flow_split's
mixed case (chosen there on the CPU with the numpy bound of
test_gpu_sad_prune.py: box_q, per item the lane-tasks with 16 minlb - 240 <=
U_b): no noise leaves an item a handful of entries (n <= 4), weights 12 .. 19
five to sixteen, 20 .. 24 up to about fifty, the heaviest a full list; a flat
frame ties every bound.  That every class of R ran is asserted from the tuning
build's histogram of executed wave-tasks by n (me_debug_prune_split_hist).

Child processes on libme_hip_tune.so, every case in each: the rule, the earlier
rule, 8 workgroups with a ring of 3 slots (long walks, ring reuse), ME_PRUNE=2
(verify: every lane-task runs and a wrongly dead one sets the error word, which
me_device_check reads: it must stay 0).
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
from test_gpu_flow_prebound import _alternating
from test_gpu_flow_slim import _oracle, _search
from test_gpu_flow_split import MIXED_AMPL, split_case

S, B = 32, 16
ROWS = (1, 2, 3, 4, 7, 13)
# noise weight (of 256) of frame f of graded_256x64: the middle weights of the mixed case twice (a frame has 16
# items where the mixed case's has 40); the last frame is flat
GRADED_AMPL = [0, 4, 8] + [a for a in MIXED_AMPL[3:16] for _ in (0, 1)] + [40, 256, 0]
assert len(GRADED_AMPL) == 32


def rows_of(n, rule="1"):
    """csrc/me_geom.h flow_split_rows / flow_split_rows_124."""
    if n > 32:
        return 13
    if rule == "2":
        return 4 if n <= 16 else 7
    return 1 if n <= 4 else 2 if n <= 9 else 3 if n <= 12 else 4 if n <= 16 else 7


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ref, cur, oracle mv, oracle cost) of a named case, computed once."""
    if name == "bypass_bands":
        return _alternating(2)
    if name == "mixed":
        ref, cur = split_case("mixed")
    else:
        rng = np.random.default_rng(2024)
        refs, curs = [], []
        for f, a in enumerate(GRADED_AMPL):
            ref = synth._box5(rng.integers(0, 256, (64, 256), dtype=np.uint8))
            cur = synth.shift_plane(ref, *((3, -3) if f % 2 == 0 else (-6, 4))).astype(np.int32)
            cur = ((256 - a) * cur + a * rng.integers(0, 256, (64, 256))) >> 8
            refs.append(ref)
            curs.append(np.ascontiguousarray(cur.astype(np.uint8)))
        refs[-1] = np.full((64, 256), 77, np.uint8)
        curs[-1] = refs[-1].copy()
        ref, cur = np.stack(refs), np.stack(curs)
    return (ref, cur) + _oracle(ref, cur)


CASES = ["graded_256x64", "mixed", "bypass_bands"]


def test_shapes_qualify():
    """Two or more jobs, 4-block tiles, two tiles or more per CU of 256."""
    for name in CASES:
        F, h, w = (32, 64, 256) if name == "graded_256x64" else (20, 136, 320) if name == "mixed" else (32, 136, 320)
        assert F >= 2 and w % 64 == 0 and F * (w // 64) * ((h + B - 1) // B) >= 512, name
    assert 64 % B == 0 and 136 % B == 8  # full tiles only; an h = 8 bottom row


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_product_fields_equal_oracle(engine, name):
    ref, cur, omv, oco = _case(name)
    mv, co = _search(engine, ref, cur)
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


_CHILD = r"""
import ctypes, hashlib, json, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import motionestimation_amd as me
assert me._lib.LIB_PATH.endswith("libme_hip_tune.so"), me._lib.LIB_PATH
L = me._lib.lib()
for fn in (L.me_debug_prune_stats, L.me_debug_prune_split_stats, L.me_debug_prune_split_hist):
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
B, S = 16, 32
z = np.load({data!r})
out = {{}}
with me.Engine() as eng:
    for name in {cases!r}:
        ref, cur, omv, oco = (z[name + "_" + k] for k in ("ref", "cur", "mv", "co"))
        F, h, w = ref.shape
        nb = me.num_blocks(w, h, B)
        ref_t, cur_t = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
        co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
        st, sp, hist = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 3)(), (ctypes.c_uint32 * 64)()
        assert L.me_debug_prune_stats(eng._h, st) == 0 and L.me_debug_prune_split_stats(eng._h, sp) == 0
        assert L.me_debug_prune_split_hist(eng._h, hist) == 0  # (the counts start at 0)
        eng.search_batch_device(ref_t, 0, cur_t, 0, w, h, B, S, "sad", 0, (h + B - 1) // B, mv, co)
        torch.cuda.synchronize()
        eng.device_check()
        assert L.me_debug_prune_stats(eng._h, st) == 0 and L.me_debug_prune_split_stats(eng._h, sp) == 0
        assert L.me_debug_prune_split_hist(eng._h, hist) == 0
        mvh, coh = mv.cpu().numpy().reshape(F, nb, 2), co.cpu().numpy().view(np.uint32).reshape(F, nb)
        assert np.array_equal(coh, oco), (name, "sad")
        assert np.array_equal(mvh, omv), (name, "mv")
        out[name] = {{"stats": list(st), "split": list(sp), "hist": list(hist),
                      "sha": hashlib.sha256(mvh.tobytes() + coh.tobytes()).hexdigest()}}
print("RESULT " + json.dumps(out))
print("split2 ok")
"""

MODES = {
    "rule": {},
    "rule_124": {"ME_PRUNE_SPLIT": "2"},
    "wgs8_slots3": {"ME_FLOW_WGS": "8", "ME_FLOW_SLOTS": "3"},
    "verify": {"ME_PRUNE": "2"},
}
_ENV = ("ME_PRUNE", "ME_PRUNE_SPLIT", "ME_PRUNE_PLANES", "ME_PRUNE_BYPASS", "ME_FLOW_SLOTS", "ME_FLOW_TABLE",
        "ME_FLOW_TABLE_CAP", "ME_FLOW_PRE", "ME_FLOW_PRE_PRIO", "ME_FLOW_WGS")
_results = {}


def _child(mode, tmp_path_factory):
    """Every case in one child on the tuning build, once per mode: equal to the
    oracle there and me_device_check clean (asserted in the child); returns
    {case: {stats: [live, total, bypassed, items], split: [whole, 2, 4 or more
    lanes per entry], hist: tasks by n, sha: of the fields}}."""
    if mode not in _results:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        d = tmp_path_factory.mktemp("split2")
        data = d / "cases.npz"
        arrays = {}
        for name in CASES:
            for k, a in zip(("ref", "cur", "mv", "co"), _case(name)):
                arrays[name + "_" + k] = a
        np.savez(data, **arrays)
        script = d / "child.py"
        script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), data=str(data), cases=CASES))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        for k in _ENV:
            env.pop(k, None)
        env.update(MODES[mode])
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "split2 ok" in r.stdout
        _results[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    return _results[mode]


def _by_rows(hist, rule):
    out = dict.fromkeys(ROWS, 0)
    for i, c in enumerate(hist):
        out[rows_of(i + 1, rule)] += c
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_tuning_build_modes(tmp_path_factory, mode):
    """The child holds every case against the oracle; here: the planes' launch
    took every item, the histogram agrees with the class counters under the
    mode's rule, and every class of R ran on the graded inputs."""
    res = _child(mode, tmp_path_factory)
    rule = MODES[mode].get("ME_PRUNE_SPLIT", "1")
    for name in CASES:
        live, total, bypassed, items = res[name]["stats"]
        whole, two, more = res[name]["split"]
        by = _by_rows(res[name]["hist"], rule)
        print(mode, name, res[name]["stats"], res[name]["split"], by)
        ref = _case(name)[0]
        F, h, w = ref.shape
        assert items == F * (w // 64) * ((h + B - 1) // B), (mode, name)
        assert 0 < live <= total
        # h = 16 items: the histogram's classes are the counters' (an h = 8 item's tasks run whole, uncounted by n)
        assert by[7] == two and sum(by[r] for r in (1, 2, 3, 4)) == more and by[13] <= whole, (mode, name, by)
        if h % B == 0:
            assert by[13] == whole, (mode, name, by)
        if mode == "verify":  # every lane-task runs: full lists, nothing to split
            assert two + more == 0, (mode, name)
        elif name != "bypass_bands":
            want = (4, 7, 13) if rule == "2" else ROWS
            assert all(by[r] > 0 for r in want), (mode, name, by)
            assert all(by[r] == 0 for r in ROWS if r not in want), (mode, name, by)
    if mode.startswith("wgs8"):
        assert res["bypass_bands"]["stats"][2] > 0  # the bypass engaged on the long walks


@pytest.mark.gpu
def test_rules_agree(tmp_path_factory):
    """The rule and the earlier one from the same build: the same fields, the
    same live lists and the same tasks by n; 8 workgroups: the same fields."""
    new, old, wgs = (_child(m, tmp_path_factory) for m in ("rule", "rule_124", "wgs8_slots3"))
    for name in CASES:
        assert new[name]["sha"] == old[name]["sha"] == wgs[name]["sha"], name
        if new[name]["stats"][2] == 0 and old[name]["stats"][2] == 0:  # (the bypass depends on timing)
            assert new[name]["stats"] == old[name]["stats"], name
            assert new[name]["hist"] == old[name]["hist"], name
