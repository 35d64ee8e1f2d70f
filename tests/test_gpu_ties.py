"""The tie rule (first minimum in raster order: dy outer, dx inner, strict <)
on every search kernel, with the sheared-periodic frames of tests/tie_cases.py.

Candidates d and d + v read identical reference patches for every lattice
vector v, so they tie bit for bit in SAD, SSD, SSIM score and box-sum bound at
any cost level; tests/test_tie_cases.py proves on the CPU that most blocks tie,
that a (dx, dy) key order or a last-wins rule would pick other vectors, and
that the tied pairs sit on every seam of the flow kernel's geometry (lane-task,
row part of every split, dx group, dy chunk, fold column and its wrap, the
(0, 0) seed in both orders).  Every comparison here is array_equal on vectors
and costs, against the oracle's full search (tests/oracle_lib.py) or the numpy
restatements (partition_ref, rd_ref, partition_rd_ref).

a. The flow kernels (SAD, 16x16, +-32): the product build, and child processes
   on the tuning build in every mode that changes how a pruned item's
   surviving candidates are reduced (the pattern of test_gpu_flow_split2.py,
   whose child script this module runs on its own cases).
b. The matrix-core SSD kernels on every me_set_kernel_path value, the 8x8
   kernel, the block-major kernel's segmented keys at +-128, and 16x16 SSIM on
   the matrix cores and on the float-chain kernels.  The path each search must
   report is the planner's (csrc/me_mfma_plan.cpp, oracle/mfma_plan_dump for
   256 CUs): rows of 200 bytes are not 16-byte aligned, so every matrix-core
   path plans the 4x4-block-tile kernel for lat_small; 656 x 368 gets the band
   walk on 'auto' and 'lean'; at +-128 the band walk (S <= 64) and the tile
   kernel (S <= 103) are out: the prepass pair, or the VALU kernels on 'tiles'.
c. The partition, rate-constrained and rate-constrained partition searches on
   their fast kernels (16x16, +-16 and +-32) and generic ones (8x8), at lambda
   0 and, with the predictor half way between two tied minimisers, at lambda 5
   and 1000: J ties exactly at a non-zero rate.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_rd_ref as Q
import partition_ref as P
import rd_ref as R
import test_gpu_partition as GP
import test_gpu_partition_rd as GQ
import test_gpu_rd as GR
import tie_cases as T
from test_gpu_flow_slim import _oracle, _search
from test_gpu_flow_split2 import _CHILD, _ENV, rows_of

NT = min(16, os.cpu_count() or 1)
ROWS = (1, 2, 3, 4, 7, 13)


# --------------------------------------------------------------- a. flow kernels
@functools.lru_cache(maxsize=None)
def _flow_case(name):
    """(ref, cur, oracle mv, oracle cost) of a case of the table, computed once."""
    ref, cur = (np.array(a) for a in T.frames(name))  # (writable copies: they become torch tensors)
    return (ref, cur) + _oracle(ref, cur)


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.FLOW_CASES)
def test_flow_product_build(engine, name):
    """prepared_batch_search, twice into the same buffers, me_device_check (in
    _search); lat_1024x512 is a single job: me_flow_kernel without planes."""
    ref, cur, omv, oco = _flow_case(name)
    mv, co = _search(engine, ref, cur)
    assert me.last_search_path() == "valu", me.last_search_path()
    np.testing.assert_array_equal(co, oco, err_msg=f"{name} sad")
    np.testing.assert_array_equal(mv, omv, err_msg=f"{name} mv")


MODES = {
    "rule": {},
    "rule_124": {"ME_PRUNE_SPLIT": "2"},
    "split_off": {"ME_PRUNE_SPLIT": "0"},
    "verify": {"ME_PRUNE": "2"},
    "prune_off": {"ME_PRUNE": "0"},
    "planes_off": {"ME_PRUNE_PLANES": "0"},
    "table_off": {"ME_FLOW_TABLE": "0"},
    "pre_off": {"ME_FLOW_PRE": "0"},
    "wgs8_slots3": {"ME_FLOW_WGS": "8", "ME_FLOW_SLOTS": "3"},
}
_results = {}


def _child(mode, tmp_path_factory):
    """Every flow case in one fresh child on the tuning build, once per mode:
    equal to the oracle there and me_device_check clean (asserted in the
    child); {case: {stats: [live, total, bypassed, items], split, hist: tasks
    by n, sha}}.  A child that fails fails its test once: nothing is retried."""
    if mode not in _results:
        lib = os.path.join(O.REPO, "motionestimation_amd", "lib", "libme_hip_tune.so")
        assert os.path.exists(lib), "build with __graft_entry__.build()"
        d = tmp_path_factory.mktemp("ties_" + mode)
        arrays = {}
        for name in T.FLOW_CASES:
            for k, a in zip(("ref", "cur", "mv", "co"), _flow_case(name)):
                arrays[name + "_" + k] = a
        np.savez(d / "cases.npz", **arrays)
        script = d / "child.py"
        script.write_text(_CHILD.format(repo=O.REPO, tests=os.path.join(O.REPO, "tests"), data=str(d / "cases.npz"),
                                        cases=list(T.FLOW_CASES)))
        env = dict(os.environ, ME_HIP_LIB="libme_hip_tune.so")
        for k in _ENV:
            env.pop(k, None)
        env.update(MODES[mode])
        _results[mode] = None
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "split2 ok" in r.stdout
        _results[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert _results[mode] is not None, f"the child of mode {mode} failed in an earlier test"
    return _results[mode]


def _by_rows(hist, rule):
    out = dict.fromkeys(ROWS, 0)
    for i, c in enumerate(hist):
        out[rows_of(i + 1, rule)] += c
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_flow_tuning_build_modes(tmp_path_factory, mode):
    """The child holds every case against the oracle.  Here: the pruning launch
    took every item (none with ME_PRUNE=0), and under the current rule every
    class of wave-task ran on lat_320x136: R = 1, 2, 3, 4, 7 rows per lane and
    whole (13)."""
    res = _child(mode, tmp_path_factory)
    rule = MODES[mode].get("ME_PRUNE_SPLIT", "1")
    for name in T.FLOW_CASES:
        c = T.CASES[name]
        live, total, bypassed, items = res[name]["stats"]
        by = _by_rows(res[name]["hist"], "2" if rule == "2" else "1")
        print(mode, name, "stats", res[name]["stats"], "split", res[name]["split"], "tasks by R", by)
        if mode == "prune_off":
            assert items == 0, (mode, name, res[name]["stats"])
            continue
        assert items == len(c.frames) * (c.width // 64) * -(-c.height // T.B), (mode, name, res[name]["stats"])
        assert 0 < live <= total
    if mode == "rule":
        by = _by_rows(res["lat_320x136"]["hist"], "1")
        assert all(by[r] > 0 for r in ROWS), by


@pytest.mark.gpu
def test_flow_modes_agree(tmp_path_factory):
    """The same fields in every mode; the same live and total lane-task counts
    under the rule and the earlier one, and with the planes on and off, where no
    item was bypassed (the bypass depends on timing)."""
    res = {m: _child(m, tmp_path_factory) for m in MODES}
    for name in T.FLOW_CASES:
        assert len({res[m][name]["sha"] for m in MODES}) == 1, name
        base = res["rule"][name]["stats"]
        for m in ("rule_124", "planes_off"):
            other = res[m][name]["stats"]
            print(name, "rule", base, m, other)
            if base[2] == 0 and other[2] == 0:
                assert base[:2] == other[:2], (name, m, base, other)


# ------------------------------------------------- b. matrix-core SSD, and SSIM
@functools.lru_cache(maxsize=None)
def _frame(name):
    """(ref, cur) of one lattice frame."""
    if name.startswith("small"):
        ref, cur = T.frames("lat_small")
        return ref[int(name[5:])], cur[int(name[5:])]
    sw = T.sweep_shifts()
    if name == "lat_656x368":  # whole blocks, 16-byte aligned rows
        return T.build_frame(656, 368, T.Fr((37, 17, 20), (sw[3], sw[10], sw[20], sw[31]), (0, 8, 16, 24)), 656)
    if name == "dense_656x368":  # a period that ties inside a +-7 window
        return T.build_frame(656, 368, T.Fr((5, 3, 2), ((2, -1), (-3, 1)), (6, 12)), 657)
    if name == "lat_384x320":  # 16 * 8 + 2 * 128 wide, 16 * 4 + 2 * 128 tall: 8 x 4 blocks with the whole +-128 window
        return T.build_frame(384, 320, T.Fr((97, 61, 40), ((5, -3), (-70, 90)), (8, 0)), 384)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_one(name, blk, span, cost):
    ref, cur = _frame(name)
    return O.full_search(ref, cur, blk, span, cost, threads=NT)[:2]


def _ssd_path(name, blk, span, path):
    """The kernel family the planner gives the search (see the module docstring)."""
    if path == "valu":
        return "valu"
    if blk == 8:
        return "mfma_8x8"
    if name.startswith("small"):
        return "mfma_tiles"
    if span > 64:
        return "valu" if path == "tiles" else "mfma_prepass"
    return {"auto": "mfma_bandwalk", "lean": "mfma_bandwalk", "prepass": "mfma_prepass", "tiles": "mfma_tiles"}[path]


def _run_ssd(engine, name, blk, span, paths):
    ref, cur = _frame(name)
    omv, oco = _oracle_one(name, blk, span, "ssd")
    try:
        for path in paths:
            me.set_kernel_path(path)
            mv, co = engine.full_search(ref, cur, blk, span, "ssd")
            tag = f"{name} B{blk} S{span} {path}"
            assert me.last_search_path() == _ssd_path(name, blk, span, path), (tag, me.last_search_path())
            np.testing.assert_array_equal(co, oco, err_msg=tag)
            np.testing.assert_array_equal(mv, omv, err_msg=tag)
        engine.device_check()
    finally:
        me.set_kernel_path("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("name,span", [("small0", 7), ("small0", 32), ("small0", 64), ("small1", 7), ("small1", 32),
                                       ("small1", 64), ("dense_656x368", 7), ("lat_656x368", 32), ("lat_656x368", 64)])
def test_ssd_every_kernel_path(engine, name, span):
    _run_ssd(engine, name, 16, span, ("auto", "lean", "prepass", "tiles", "valu"))
    _run_ssd(engine, name, 8, span, ("auto", "valu"))


@pytest.mark.gpu
def test_ssd_segmented_keys(engine):
    """+-128: 16 + 2 S >= 256 positions, so the block-major kernel keeps its
    keys in segments; tied candidates lie 97 columns and 61 rows apart."""
    _run_ssd(engine, "lat_384x320", 16, 128, ("auto", "lean", "prepass", "tiles", "valu"))


@pytest.mark.gpu
@pytest.mark.parametrize("span", [7, 24])
@pytest.mark.parametrize("name", ["small0", "small1"])
def test_ssim_ties(engine, name, span):
    """Identical patches give identical float chains: exact ties for the
    first-strict-maximum rule; score bits and vectors against the oracle."""
    ref, cur = _frame(name)
    omv, obits = _oracle_one(name, 16, span, "ssim")
    try:
        for path, want in (("auto", "ssim_mfma"), ("valu", "ssim")):
            me.set_kernel_path(path)
            mv, bits = engine.full_search(ref, cur, 16, span, "ssim")
            assert me.last_search_path() == want, (path, me.last_search_path())
            np.testing.assert_array_equal(bits, obits, err_msg=f"{name} S{span} {path}")
            np.testing.assert_array_equal(mv, omv, err_msg=f"{name} S{span} {path}")
        engine.device_check()
    finally:
        me.set_kernel_path("auto")


# ------------------------- c. partition, rate-constrained and both at once
LAMBDAS = T.RD_LAMBDAS


@functools.lru_cache(maxsize=None)
def _rd_inputs(blk, span, f):
    """(ref, cur, mid-point predictor, rd_ref.sad_table) of frame f of lat_small."""
    ref, cur = _frame(f"small{f}")
    cen = T.census(ref, cur, blk, span)
    h, w = ref.shape
    return ref, cur, T.midpoint_pred(cen, 0, w, h, blk), R.sad_table(ref, cur, blk, span)


def _j_ties_hold(blk, span, frames_):
    """On the CPU, before the GPU run: at least half of the blocks keep a tie
    of J under the mid-point predictor, at every lambda."""
    for lam in LAMBDAS:
        t = np.concatenate([T.j_ties(_rd_inputs(blk, span, f)[3], lam, _rd_inputs(blk, span, f)[2]) for f in frames_])
        print(f"B{blk} S{span} lambda {lam}: J tied in {int(t.sum())} of {t.size} blocks")
        assert 2 * int(t.sum()) >= t.size, (blk, span, lam)


@pytest.mark.gpu
@pytest.mark.parametrize("blk,span,frames_", T.RD_SHAPES)
def test_partition_search_ties(engine, blk, span, frames_):
    """lambda = 0: SAD ties decide all nine minima."""
    h, w = _frame("small0")[0].shape
    want_variant = GP.FAST if blk == 16 else GP.GENERIC
    assert me.partition_kernel_variant(w, h, w, blk, span) == want_variant
    for f in frames_:
        ref, cur = _frame(f"small{f}")
        GP._check(GP._device(engine, ref, cur, blk, span, 0), P.search_frame(ref, cur, blk, span, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("blk,span,frames_", T.RD_SHAPES)
def test_rd_search_ties(engine, blk, span, frames_):
    h, w = _frame("small0")[0].shape
    _j_ties_hold(blk, span, frames_)
    for lam in LAMBDAS:
        assert me.rd_kernel_variant(w, h, w, blk, span, lam) == (GR.FAST if blk == 16 else GR.GENERIC)
        for f in frames_:
            ref, cur, pred, table = _rd_inputs(blk, span, f)
            want = R.search_frame(ref, cur, blk, span, lam, pred, table=table)
            GR._check(GR._device(engine, ref, cur, blk, span, lam, pred), want)


@pytest.mark.gpu
@pytest.mark.parametrize("blk,span,frames_", T.RD_SHAPES)
def test_partition_rd_search_ties(engine, blk, span, frames_):
    h, w = _frame("small0")[0].shape
    _j_ties_hold(blk, span, frames_)
    for f in frames_:
        ref, cur, pred, _ = _rd_inputs(blk, span, f)
        table = Q.quad_table(ref, cur, blk, span)
        for lam in LAMBDAS:
            assert me.partition_rd_kernel_variant(w, h, w, blk, span, lam) == (GQ.FAST if blk == 16 else GQ.GENERIC)
            want = Q.search_frame(ref, cur, blk, span, lam, pred, table)
            GQ._check(GQ._device(engine, ref, cur, blk, span, lam, pred), want)
