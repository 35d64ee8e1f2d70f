"""The partition-wise quarter-pel restatement (tests/partition_qpel_ref.py)
checked against itself and the restatements it stands on (CPU suite): its two
forms agree, the identities Q1-Q6 of include/me.h hold against rd_ref, qpel_ref,
satd_ref and qpel_ref.compensate, the host-only pieces of the C ABI behave as
specified, and on Foreman 1 -> 2 (16x16, +-7, lambda 16, zero predictor) the
sums are the ones DESIGN.md "Partition-wise quarter-pel refinement" quotes."""
import ctypes

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_qpel_ref as PQ
import partition_rd_ref as PR
import partition_ref as P
import qpel_ref as Q
import rd_ref as RD
import satd_ref as SR
from motionestimation_amd import _lib
from rd_ref import bits

# (w, h, B, tile, S, lambda): clipped right and bottom, empty lower halves
SHAPES = [(56, 40, 16, 8, 4, 4), (29, 21, 8, 4, 3, 2), (50, 38, 16, 8, 3, 0), (40, 40, 32, 8, 3, 8)]


def _random_fields(w, h, B, lim, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-lim, lim + 1, (n, 2)).astype(np.int16) for n in P.counts(w, h, B)]


def _pred(w, h, B, seed):
    n = P.counts(w, h, B)[0]
    return np.random.default_rng(seed).integers(-40, 41, (n, 2)).astype(np.int16)


_cache = {}


def _case(w, h, B, tile, S, lam, cost, with_pred):
    """(ref, cur, integer fields, pred, refine_frame's result), computed once."""
    key = (w, h, B, tile, S, lam, cost, with_pred)
    if key not in _cache:
        ref, cur = PQ.content(w, h, tile, 7, B)
        F = PR.search_frame(ref, cur, B, S, lam)
        pred = _pred(w, h, B, 5) if with_pred else None
        _cache[key] = (ref, cur, F.mv, pred, PQ.refine_frame(ref, cur, B, F.mv, lam, pred, cost))
    return _cache[key]


def _same(a, b):
    for k in range(4):
        np.testing.assert_array_equal(a.mv[k], b.mv[k])
        np.testing.assert_array_equal(a.cost[k], b.cost[k])
        np.testing.assert_array_equal(a.dist[k], b.dist[k])
        np.testing.assert_array_equal(a.bits[k], b.bits[k])
    np.testing.assert_array_equal(a.mode, b.mode)
    np.testing.assert_array_equal(a.mode_cost, b.mode_cost)


@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,tile,S,lam", SHAPES)
def test_the_two_forms_agree(w, h, B, tile, S, lam, cost):
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, lam, cost, True)
    _same(A, PQ.refine_cells(ref, cur, B, mv, lam, pred, cost))


def test_the_two_forms_agree_on_hand_made_fields():
    # independent vectors per cell, far enough out that whole windows are edge replication
    w, h, B = 56, 40, 16
    ref, cur = PQ.content(w, h, 8, 3, B)
    for lim, cost in ((6, "sad"), (40, "satd"), (_lib.ME_QPEL_MAX_MV, "ssd")):
        mv = _random_fields(w, h, B, lim, lim)
        pred = np.random.default_rng(1).integers(-32767, 32768, (P.counts(w, h, B)[0], 2)).astype(np.int16)
        _same(PQ.refine_frame(ref, cur, B, mv, 4, pred, cost),
              PQ.refine_cells(ref, cur, B, mv, 4, pred, cost))


def _refine_rd(ref, cur, blk, mv, lam, pred, cost):
    if cost == "satd":
        return SR.refine_rd(ref, cur, blk, mv, lam, pred)
    return RD.refine(ref, cur, blk, mv, lam, pred, cost)


@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,tile,S,lam", SHAPES)
def test_q1_q2_square_grids_are_the_block_refinement(w, h, B, tile, S, lam, cost):
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, lam, cost, True)
    for k, blk in ((0, B), (3, B // 2)):
        p = PQ.cell_pred(pred, w, h, B, k)
        q, J, D = _refine_rd(ref, cur, blk, mv[k], lam, p, cost)
        np.testing.assert_array_equal(A.mv[k], q)
        np.testing.assert_array_equal(A.cost[k], J)
        np.testing.assert_array_equal(A.dist[k], D)


@pytest.mark.parametrize("cost", PQ.COSTS)
def test_q3_without_a_rate_it_is_the_plain_refinement(cost):
    w, h, B, tile, S, _ = SHAPES[0]
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, 0, cost, True)
    for k in range(4):
        np.testing.assert_array_equal(A.cost[k], A.dist[k])
    for k, blk in ((0, B), (3, B // 2)):
        q, c = SR.refine(ref, cur, blk, mv[k]) if cost == "satd" else Q.refine(ref, cur, blk, mv[k], cost)
        np.testing.assert_array_equal(A.mv[k], q)
        np.testing.assert_array_equal(A.dist[k], c)


@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,tile,S,lam", SHAPES)
def test_q4_mode_follows_from_the_costs(w, h, B, tile, S, lam, cost):
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, lam, cost, True)
    nbx, nby = P.grids(w, h, B)[0]
    for by in range(nby):
        for bx in range(nbx):
            J = [lam * m for m in PR.MBITS]
            for gi, i, j, *_ in P._partitions(B, min(B, w - bx * B), min(B, h - by * B)):
                sx, sy = PR.REP[gi]
                J[gi] += int(A.cost[gi][(sy * by + j) * P.grids(w, h, B)[gi][0] + sx * bx + i])
            mode = min(range(4), key=lambda m: (J[m], m))
            assert (A.mode[by * nbx + bx], A.mode_cost[by * nbx + bx]) == (mode, J[mode])


@pytest.mark.parametrize("w,h,B,tile,S,lam", SHAPES)
def test_q5_leaf_compensation_reproduces_the_chosen_distortion(w, h, B, tile, S, lam):
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, lam, "sad", True)
    leaf = P.leaf_field(A)
    # the C function copies int16 vectors whatever their unit
    np.testing.assert_array_equal(
        leaf, me.partition_leaf_field(w, h, B, me.PartitionFields(A.mv, None, A.mode, None)))
    mc = Q.compensate(ref, B // 2, leaf)
    assert int(np.abs(mc.astype(np.int64) - cur.astype(np.int64)).sum()) == PQ.summary(A)[2]


@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,tile,S,lam", SHAPES)
def test_q6_no_cell_is_worse_than_its_centre(w, h, B, tile, S, lam, cost):
    ref, cur, mv, pred, A = _case(w, h, B, tile, S, lam, cost, True)
    for k, (bw, bh) in enumerate(PQ.dims(B)):
        F = PQ._RectFrame(ref, bw, bh)
        q = 4 * mv[k].astype(np.int64)
        p = PQ.cell_pred(pred, w, h, B, k)
        centre = F.costs(cur.astype(np.int64) - F.predict(q), cost) + \
            lam * (bits(q[:, 0] - p[:, 0]) + bits(q[:, 1] - p[:, 1]))
        assert (A.cost[k] <= centre).all()
        # bits is the result's rate and J = dist + lam * bits
        r = bits(A.mv[k][:, 0].astype(np.int64) - p[:, 0]) + bits(A.mv[k][:, 1].astype(np.int64) - p[:, 1])
        np.testing.assert_array_equal(A.bits[k], r)
        np.testing.assert_array_equal(A.cost[k], A.dist[k].astype(np.int64) + lam * r)


def test_constant_planes_keep_every_centre_and_mode_zero():
    w, h, B = 50, 38, 16
    ref = np.full((h, w), 90, np.uint8)
    cur = np.full((h, w), 97, np.uint8)
    mv = _random_fields(w, h, B, 6, 2)
    for cost in PQ.COSTS:
        A = PQ.refine_frame(ref, cur, B, mv, 0, None, cost)
        for k in range(4):
            np.testing.assert_array_equal(A.mv[k], 4 * mv[k])
        assert not A.mode.any()


def test_the_content_exercises_the_partitions():
    """The counts the GPU tests rely on (tests/test_gpu_partition_qpel.py)."""
    moved = lambda A, mv: (sum(int((A.q1[k] != 4 * mv[k]).any(1).sum()) for k in range(4)),
                           sum(int((A.q1[k] != A.mv[k]).any(1).sum()) for k in range(4)))
    for cost, hist in (("sad", [5, 1, 2, 4]), ("satd", [5, 1, 2, 4]), ("ssd", [6, 1, 1, 4])):
        ref, cur, mv, _, A = _case(56, 40, 16, 8, 4, 4, cost, False)
        assert np.bincount(A.mode, minlength=4).tolist() == hist
        s1, s2 = moved(A, mv)
        cells = sum(len(m) for m in mv)
        assert cells == 88 and 2 * s1 >= cells and 10 * s2 >= cells, (s1, s2)
    differ = 0
    nbx, nby = P.grids(56, 40, 16)[0]
    for by in range(nby):
        for bx in range(nbx):
            vs = set()
            for gi, i, j, *_ in P._partitions(16, min(16, 56 - 16 * bx), min(16, 40 - 16 * by)):
                sx, sy = PR.REP[gi]
                vs.add(tuple(mv[gi][(sy * by + j) * P.grids(56, 40, 16)[gi][0] + sx * bx + i]))
            differ += len(vs) > 1
    assert 2 * differ >= nbx * nby, differ


# ---- host-only pieces of the C ABI

def test_entry_points_refuse_a_null_context():
    """The refusal that needs no context (the rules that need one:
    tests/test_gpu_partition_qpel.py)."""
    L = _lib.lib()
    a = np.zeros(64, np.uint8)
    fin, fout = me.PartitionFields.host(16, 16, 16), me.PartitionRdFields.host(16, 16, 16)
    sin, sout = fin.struct(), fout.rd_struct()
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.me_partition_refine_qpel(None, p, p, 16, 16, 16, 16, _lib.ME_COST_SAD, 0, None,
                                      ctypes.byref(sin), ctypes.byref(sout)) == _lib.ME_EINVAL
    assert L.me_partition_refine_qpel_device(None, p, 0, p, 0, 16, 16, 16, 16, _lib.ME_COST_SAD, 0, 1,
                                             None, ctypes.byref(sin), ctypes.byref(sout),
                                             None) == _lib.ME_EINVAL
    assert L.me_partition_search_qpel(None, p, p, 16, 16, 16, 16, 4, _lib.ME_COST_SAD, 0, None,
                                      ctypes.byref(sout), None) == _lib.ME_EINVAL


def test_header_states_the_limits():
    src = open(O.REPO + "/include/me.h").read()
    for name in ("me_partition_refine_qpel_device", "me_partition_refine_qpel", "me_partition_search_qpel"):
        assert f"me_status {name}(" in src
    # Jq of the largest macroblock at SSD and the largest lambda fits u32
    assert 32 * 32 * 255 * 255 == 66585600
    assert 66585600 + (4 * 66 + 5) * me.ME_PART_RD_MAX_LAMBDA == 2323121152 < 1 << 32
    # |q - p| <= 4 * ME_QPEL_MAX_MV + 3 + 32768 codes in 33 bits
    assert int(bits(4 * _lib.ME_QPEL_MAX_MV + 3 + 32768)) == 33


# ---- Foreman 1 -> 2, 16x16, +-7, lambda 16, zero predictor: DESIGN.md
# "Partition-wise quarter-pel refinement".  Integer: (mode histogram, sum J,
# sum dist); per cost: today's recipe (sum J at its true rate, sum dist, vectors
# coded), the partition-wise refinement (histogram, sum J, sum dist).
FOREMAN_INT = ([356, 13, 24, 3], 340705, 280801)
FOREMAN = {"sad": ((348402, 220338, 917), ([357, 14, 22, 3], 282403, 217955)),
           "satd": ((553133, 399725, 1075), ([327, 30, 35, 4], 471103, 396991))}


def _recipe(ref, cur, F, lam, cost):
    """INTEGRATION.md's plain-field recipe: the integer leaf field refined at
    B / 2, priced at its true rate: per macroblock mbits(mode) and one
    bits(qx) + bits(qy) per distinct leaf vector it actually produces."""
    w, h, B = F.w, F.h, F.B
    q, _, D = _refine_rd(ref, cur, B // 2, P.leaf_field(F), lam, None, cost)
    g = P.grids(w, h, B)
    (nbx, nby), (nhx, nhy) = g[0], g[3]
    rate = vectors = 0
    for by in range(nby):
        for bx in range(nbx):
            vs = {tuple(int(v) for v in q[hy * nhx + hx])
                  for hy in (2 * by, 2 * by + 1) for hx in (2 * bx, 2 * bx + 1) if hx < nhx and hy < nhy}
            rate += sum(int(bits(v[0])) + int(bits(v[1])) for v in vs) + PR.MBITS[F.mode[by * nbx + bx]]
            vectors += len(vs)
    sd = int(D.astype(np.int64).sum())
    return sd + lam * rate, sd, vectors


def test_foreman_table():
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    lam = 16
    F = PR.search_frame(ref, cur, 16, 7, lam)
    got = PR.summary(F, lam)[:3]
    print("integer partition-RD:", got)
    assert got == FOREMAN_INT
    for cost, (recipe, ours) in FOREMAN.items():
        r = _recipe(ref, cur, F, lam, cost)
        A = PQ.summary(PQ.refine_frame(ref, cur, 16, F.mv, lam, None, cost))
        print(cost, "leaf field refined at 8x8:", r, "partition-wise:", A)
        assert r == recipe and A == ours
        # one vector per partition paid for, fewer bits and no more distortion
        assert A[1] < r[0] and A[2] <= r[1]
