"""The rate-constrained partition search's numpy restatement
(tests/partition_rd_ref.py) and the host-only side of the feature (CPU suite):
the restatement's two forms agree; identities E1 .. E5 of include/me.h hold
against partition_ref, rd_ref and a numpy compensation; Foreman 1 -> 2 (16x16,
+-7, zero predictor) gives the table DESIGN.md quotes; and
me_partition_rd_kernel_variant is pinned for every shape the GPU suite
(tests/test_gpu_partition_rd.py) runs."""
import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_rd_ref as Q
import partition_ref as P
import rd_ref as R
from motionestimation_amd import _lib

FAST, GENERIC = _lib.ME_PART_KERNEL_FAST, _lib.ME_PART_KERNEL_GENERIC
FAST_LAM = _lib.ME_RD_FAST_MAX_LAMBDA
TOP_LAM = _lib.ME_PART_RD_MAX_LAMBDA


def _pair(w, h, seed, shift=(2, -3)):
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    big = ((big.astype(np.uint16) + np.roll(big, 1, 0) + np.roll(big, 1, 1) +
            np.roll(big, (1, 1), (0, 1))) // 4).astype(np.uint8)
    ref = big[8:8 + h, 8:8 + w]
    cur = big[8 + shift[1]:8 + shift[1] + h, 8 + shift[0]:8 + shift[0] + w]
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


def _pred(w, h, B, seed, span=32768):
    n = P.counts(w, h, B)[0]
    return np.random.default_rng(seed).integers(-span, span, (n, 2)).astype(np.int16)


def _same(a, b):
    for k in range(4):
        for name in ("mv", "cost", "dist", "bits"):
            np.testing.assert_array_equal(getattr(a, name)[k], getattr(b, name)[k],
                                          err_msg=f"{name} {P.MODES[k]}")
    np.testing.assert_array_equal(a.mode, b.mode)
    np.testing.assert_array_equal(a.mode_cost, b.mode_cost)


@pytest.mark.parametrize("w,h,B,S,lam,span", [
    (44, 28, 16, 5, 16, 40), (9, 9, 16, 3, 1, 32768), (40, 24, 8, 7, 64, 20),
    (70, 40, 32, 4, 16, 32768), (33, 17, 16, 12, TOP_LAM, 100)])
def test_two_forms_agree(w, h, B, S, lam, span):
    ref, cur = _pair(w, h, w * h + B)
    pred = _pred(w, h, B, 3, span)
    _same(Q.search_loops(ref, cur, B, S, lam, pred), Q.search_frame(ref, cur, B, S, lam, pred))


def test_search_macroblock_agrees():
    w, h, B, S, lam = 44, 28, 16, 5, 16
    ref, cur = _pair(w, h, 9)
    pred = _pred(w, h, B, 4, 40)
    F = Q.search_frame(ref, cur, B, S, lam, pred)
    nbx, nby = P.grids(w, h, B)[0]
    seen = 0
    for by in range(nby):
        for bx in range(nbx):
            mb = by * nbx + bx
            rec, mode, cost = Q.search_macroblock(ref, cur, B, S, lam, pred[mb], bx, by)
            assert (mode, cost) == (F.mode[mb], F.mode_cost[mb])
            for (k, c), (mv, J, D, Rb) in rec.items():
                assert (tuple(F.mv[k][c]), F.cost[k][c], F.dist[k][c], F.bits[k][c]) == (mv, J, D, Rb)
            seen += len(rec)
    assert seen == sum(P.counts(w, h, B))


@pytest.mark.parametrize("pred", [None, (10, -10)])
def test_two_forms_agree_on_ties(pred):
    """A flat frame: every SAD ties, the rate decides, and bits(v) = bits(-v)
    leaves ties for the first raster candidate."""
    flat = np.full((28, 44), 7, np.uint8)
    p = None if pred is None else np.tile(np.int16(pred), (6, 1))
    a, b = Q.search_loops(flat, flat, 16, 4, 16, p), Q.search_frame(flat, flat, 16, 4, 16, p)
    _same(a, b)
    assert (a.dist[0] == 0).all()
    if pred is None:
        assert (a.mv[0] == 0).all() and (a.bits[3] == 2).all()
    else:
        # top left (d >= 0): |4 dx - 10| = 2 at dx = 2 and 3, the first wins.  Bottom
        # right (d <= 0): bits(4 dx - 10) = 9 at dx = -1 and 0, |4 dy + 10| = 2 at
        # dy = -3 and -2: the first of each in raster order
        assert tuple(a.mv[0][0]) == (2, 0) and tuple(a.mv[0][-1]) == (-1, -3)


# ---- E1: lambda = 0 is the partition search, whatever the predictor
@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 5), (70, 40, 32, 4), (40, 24, 8, 7)])
def test_e1_lambda_zero_is_the_partition_search(w, h, B, S):
    ref, cur = _pair(w, h, 4)
    F = Q.search_frame(ref, cur, B, S, 0, _pred(w, h, B, 5))
    G = P.search_frame(ref, cur, B, S, 0)
    for k in range(4):
        np.testing.assert_array_equal(F.mv[k], G.mv[k])
        np.testing.assert_array_equal(F.cost[k], G.cost[k])
        np.testing.assert_array_equal(F.dist[k], F.cost[k])
    np.testing.assert_array_equal(F.mode, G.mode)
    np.testing.assert_array_equal(F.mode_cost, G.mode_cost)


# ---- E2: the 2Nx2N records are the rate-constrained search's at B
@pytest.mark.parametrize("w,h,B,S,lam", [(44, 28, 16, 5, 16), (70, 40, 32, 9, 256),
                                          (40, 24, 8, 3, 1), (96, 64, 16, 7, FAST_LAM)])
def test_e2_2nx2n_is_the_rd_search(w, h, B, S, lam):
    ref, cur = _pair(w, h, 3)
    pred = _pred(w, h, B, 6, 64)
    F = Q.search_frame(ref, cur, B, S, lam, pred)
    mv, J, D, Rb = R.search_frame(ref, cur, B, S, lam, pred)
    np.testing.assert_array_equal(F.mv[0], mv)
    np.testing.assert_array_equal(F.cost[0], J)
    np.testing.assert_array_equal(F.dist[0], D)
    np.testing.assert_array_equal(F.bits[0], Rb)


# ---- E3: NxN records of unclamped full-size macroblocks are the B/2 search's
@pytest.mark.parametrize("w,h,B,S", [(96, 80, 16, 7), (128, 96, 32, 5)])
def test_e3_nxn_of_unclamped_macroblocks_is_the_half_size_rd_search(w, h, B, S):
    ref, cur = _pair(w, h, 5)
    pred = _pred(w, h, B, 7, 48)
    (nbx, nby), (nhx, nhy) = P.grids(w, h, B)[0], P.grids(w, h, B)[3]
    quarter = np.repeat(np.repeat(pred.reshape(nby, nbx, 2), 2, axis=0), 2, axis=1)[:nhy, :nhx]
    F = Q.search_frame(ref, cur, B, S, 16, pred)
    mv, J, D, Rb = R.search_frame(ref, cur, B // 2, S, 16, quarter.reshape(-1, 2))
    seen = 0
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * B, by * B
            if x0 + B > w or y0 + B > h:
                continue
            if x0 - S < 0 or y0 - S < 0 or x0 + B + S > w or y0 + B + S > h:
                continue
            for j in range(2):
                for i in range(2):
                    c = (2 * by + j) * nhx + 2 * bx + i
                    assert tuple(F.mv[3][c]) == tuple(mv[c]), (bx, by, i, j)
                    assert (F.cost[3][c], F.dist[3][c], F.bits[3][c]) == (J[c], D[c], Rb[c])
                    seen += 1
    assert seen >= 8


# ---- E4: a larger lambda never buys more bits nor less distortion
def test_e4_monotone_in_lambda():
    ref, cur = _pair(96, 64, 8)
    pred = _pred(96, 64, 16, 9, 40)
    tab = Q.quad_table(ref, cur, 16, 7)
    prev = None
    for lam in (0, 1, 4, 16, 64, 256, 4096, FAST_LAM, TOP_LAM):
        F = Q.search_frame(ref, cur, 16, 7, lam, pred, tab)
        if prev is not None:
            for k in range(4):
                assert (prev.bits[k] >= F.bits[k]).all() and (prev.dist[k] <= F.dist[k]).all()
        prev = F


# ---- E5: the leaf field compensated at B / 2 reproduces the chosen distortion
@pytest.mark.parametrize("w,h,B,lam", [(44, 28, 16, 16), (96, 64, 16, 4), (70, 40, 32, 64)])
def test_e5_leaf_compensation(w, h, B, lam):
    ref, cur = _pair(w, h, 11)
    F = Q.search_frame(ref, cur, B, 5, lam, _pred(w, h, B, 12, 24))
    hist, sum_j, sum_d, sum_b = Q.summary(F, lam)
    assert sum_j == sum_d + lam * (sum_b + int(np.dot(hist, Q.MBITS)))
    leaf = P.leaf_field(F)
    np.testing.assert_array_equal(
        leaf, me.partition_leaf_field(w, h, B, me.PartitionFields(F.mv, None, F.mode, None)))
    hb, nhx = B // 2, P.grids(w, h, B)[3][0]
    mc = np.zeros_like(cur)  # the integer compensation at block size B / 2, in numpy
    for c, (dx, dy) in enumerate(leaf):
        x0, y0 = (c % nhx) * hb, (c // nhx) * hb
        x1, y1 = min(w, x0 + hb), min(h, y0 + hb)
        mc[y0:y1, x0:x1] = ref[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    assert int(np.abs(mc.astype(np.int32) - cur.astype(np.int32)).sum()) == sum_d


# ---- Foreman 1 -> 2, 16x16, +-7, zero predictor: DESIGN.md "Rate-constrained
# partition search".  (lambda, mode histogram, sum J, sum dist, sum bits of the
# chosen modes; sum dist and sum bits of the 2Nx2N field)
FOREMAN = [(0, [77, 18, 10, 291], 255385, 255385, 14168, 290804, 3730),
           (1, [175, 55, 43, 123], 267754, 258214, 8456, 290893, 3586),
           (16, [356, 13, 24, 3], 340705, 280801, 3262, 294967, 2882),
           (64, [391, 0, 5, 0], 484257, 319393, 2170, 321438, 2168),
           (256, [396, 0, 0, 0], 844266, 472554, 1056, 472554, 1056)]


def test_foreman_table():
    import test_gpu_partition as TG
    import test_rd_ref as TR
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    tab = Q.quad_table(ref, cur, 16, 7)
    rd_rows = {row[0]: row for row in TR.FOREMAN}
    for lam, hist, sum_j, sum_d, sum_b, d0, b0 in FOREMAN:
        F = Q.search_frame(ref, cur, 16, 7, lam, None, tab)
        assert Q.summary(F, lam) == (hist, sum_j, sum_d, sum_b), lam
        got0 = (int(F.dist[0].astype(np.int64).sum()), int(F.bits[0].astype(np.int64).sum()))
        assert got0 == (d0, b0), lam
        # the 2Nx2N field against the rate-constrained search's table
        assert got0 == (rd_rows[lam][1], rd_rows[lam][2]), lam
    # the lambda = 0 row is the partition search's
    assert TG.FOREMAN[0] == (0,) + tuple(FOREMAN[0][1:4])


# ---- which kernel runs: every shape of tests/test_gpu_partition_rd.py
FAST_SHAPES = [(96, 64, 96, 7), (96, 64, 96, 16), (256, 144, 256, 32), (80, 48, 80, 64),
               (100, 72, 100, 7), (44, 28, 44, 5), (100, 64, 112, 7), (64, 48, 64, 4), (352, 288, 352, 7),
               (1920, 1080, 1920, 32), (3840, 2160, 3840, 64)]
GENERIC_SHAPES = [(9, 9, 9, 16, 5), (33, 17, 33, 16, 5), (40, 24, 40, 8, 5),
                  (70, 40, 70, 32, 5), (70, 40, 70, 32, 4), (96, 64, 99, 16, 7),
                  (96, 64, 110, 16, 7), (96, 64, 96, 16, 65)]


@pytest.mark.parametrize("w,h,pitch,S", FAST_SHAPES)
def test_fast_variant_is_pinned(w, h, pitch, S):
    for lam in (0, 1, 16, FAST_LAM):
        assert me.partition_rd_kernel_variant(w, h, pitch, 16, S, lam) == FAST
    for lam in (FAST_LAM + 1, TOP_LAM):
        assert me.partition_rd_kernel_variant(w, h, pitch, 16, S, lam) == GENERIC


@pytest.mark.parametrize("w,h,pitch,B,S", GENERIC_SHAPES)
def test_generic_variant_is_pinned(w, h, pitch, B, S):
    for lam in (0, 16, FAST_LAM, TOP_LAM):
        assert me.partition_rd_kernel_variant(w, h, pitch, B, S, lam) == GENERIC


def test_variant_follows_the_partition_search_below_the_fast_lambda():
    for w, h, pitch, B, S in [(96, 64, 96, 16, 7), (96, 64, 99, 16, 7), (98, 64, 100, 16, 7),
                              (96, 64, 96, 8, 7), (96, 64, 96, 16, 65), (9, 9, 12, 16, 3),
                              (96, 64, 96, 12, 7), (96, 64, 96, 16, 129), (0, 64, 96, 16, 7)]:
        assert me.partition_rd_kernel_variant(w, h, pitch, B, S, 16) == \
            me.partition_kernel_variant(w, h, pitch, B, S)


def test_lambda_above_the_maximum_is_rejected():
    """-1 from the planner (the entry points' ME_EINVAL needs a context:
    tests/test_gpu_partition_rd.py)."""
    assert me.partition_rd_kernel_variant(96, 64, 96, 16, 7, TOP_LAM) == GENERIC
    assert me.partition_rd_kernel_variant(96, 64, 96, 16, 7, TOP_LAM + 1) == -1
    assert me.partition_rd_kernel_variant(96, 64, 96, 16, 7, 1 << 24) == -1
    assert me.partition_rd_kernel_variant(96, 64, 96, 16, 7, -1) == -1


def test_constants_and_struct_match_header():
    import ctypes
    src = open(O.REPO + "/include/me.h").read()
    assert "#define ME_PART_RD_MAX_LAMBDA (1u << 23)" in src
    assert me.ME_PART_RD_MAX_LAMBDA == 1 << 23
    # J of the largest macroblock at the largest lambda fits u32
    assert 32 * 32 * 255 + (4 * 66 + 5) * me.ME_PART_RD_MAX_LAMBDA < 1 << 32
    # the fast kernel's lane key holds J in 26 bits
    assert 65280 + 66 * FAST_LAM < (1 << 26) - 1
    from motionestimation_amd.engine import PartFields, PartRdFields
    assert ctypes.sizeof(PartRdFields) == ctypes.sizeof(PartFields) + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert PartRdFields.f.offset == 0
