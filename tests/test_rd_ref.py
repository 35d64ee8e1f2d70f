"""The rate-constrained search's numpy restatement (tests/rd_ref.py) and the
host-only side of the feature (CPU suite): me_mv_bits is the exp-Golomb length,
the restatement's two forms agree, lambda = 0 is the oracle's full search
whatever the predictor, per block R never rises and D never falls as lambda
grows, Foreman 1 -> 2 (16x16, +-7, SAD, zero predictor) gives the table
DESIGN.md quotes, and me_rd_kernel_variant names the kernel of every shape the
GPU suite (tests/test_gpu_rd.py) runs."""
import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import qpel_ref as Q
import rd_ref as R
from motionestimation_amd import _lib

FAST, GENERIC = _lib.ME_RD_KERNEL_FAST, _lib.ME_RD_KERNEL_GENERIC
FAST_LAM = _lib.ME_RD_FAST_MAX_LAMBDA


def _pair(w, h, seed, shift=(2, -3)):
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    # smooth a little so that minima are not all isolated
    big = ((big.astype(np.uint16) + np.roll(big, 1, 0) + np.roll(big, 1, 1) +
            np.roll(big, (1, 1), (0, 1))) // 4).astype(np.uint8)
    ref = big[8:8 + h, 8:8 + w]
    cur = big[8 + shift[1]:8 + shift[1] + h, 8 + shift[0]:8 + shift[0] + w]
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


def _preds(n, seed):
    """Random full-range int16 predictors with both extremes present."""
    p = np.random.default_rng(seed).integers(-32768, 32768, (n, 2)).astype(np.int16)
    p[0] = (32767, -32767)
    p[-1] = (-32768, 32767)
    return p


def _same(a, b):
    for x, y, what in zip(a, b, ("mv", "J", "D", "R")):
        np.testing.assert_array_equal(x, y, err_msg=what)


# ---- bits
def test_mv_bits_is_the_exp_golomb_length():
    table = {0: 1, 1: 3, -1: 3, 2: 5, -2: 5, 3: 5, -3: 5, 4: 7, -4: 7, 7: 7, -7: 7, 8: 9, -8: 9}
    for v, n in table.items():
        assert me.mv_bits(v) == n
    v = np.arange(-40000, 40001)
    formula = 2 * np.floor(np.log2(2 * np.abs(v) + 1)).astype(np.int64) + 1  # exact below 2^53
    got = np.array([me.mv_bits(int(x)) for x in v])
    np.testing.assert_array_equal(got, formula)
    np.testing.assert_array_equal(R.bits(v), formula)
    # the largest argument of the definition: 4 * 1024 + 32,767 -> 33 bits
    assert me.mv_bits(4 * 1024 + 32767) == 33 and me.mv_bits(-(1 << 31)) == 65


# ---- the two forms
@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 5), (9, 9, 16, 3), (40, 24, 8, 7),
                                      (70, 40, 32, 4), (33, 17, 16, 40), (23, 17, 5, 3)])
@pytest.mark.parametrize("lam", [0, 16, 1 << 24])
def test_two_forms_agree(w, h, B, S, lam):
    ref, cur = _pair(w, h, w * h + B)
    n = me.num_blocks(w, h, B)
    for pred in (None, _preds(n, 3)):
        _same(R.search_loops(ref, cur, B, S, lam, pred), R.search_frame(ref, cur, B, S, lam, pred))


def test_search_block_is_the_loops_block_by_block():
    w, h, B, S = 44, 28, 16, 5
    ref, cur = _pair(w, h, 8)
    pred = _preds(me.num_blocks(w, h, B), 4)
    mv, J, D, Rb = R.search_loops(ref, cur, B, S, 16, pred)
    for b in range(len(mv)):
        got = R.search_block(ref, cur, B, S, 16, pred[b], b % 3, b // 3)
        assert got == (tuple(mv[b]), J[b], D[b], Rb[b]), b


@pytest.mark.parametrize("lam", [0, 7])
def test_two_forms_agree_on_a_flat_frame(lam):
    flat = np.full((28, 44), 7, np.uint8)
    a = R.search_loops(flat, flat, 16, 4, lam)
    _same(a, R.search_frame(flat, flat, 16, 4, lam))
    if lam:  # every SAD is 0: the cheapest vector to code wins
        assert (a[0] == 0).all() and (a[3] == 2).all()
    else:    # everything ties: the window's first displacement
        assert tuple(a[0][0]) == (0, 0) and tuple(a[0][-1]) != (0, 0)


@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 5), (70, 40, 32, 9), (40, 24, 8, 3)])
def test_lambda_zero_is_the_full_search(w, h, B, S):
    ref, cur = _pair(w, h, 3)
    mv, cost, _ = O.full_search(ref, cur, B, S, "sad")
    for pred in (None, _preds(me.num_blocks(w, h, B), 5)):
        got = R.search_frame(ref, cur, B, S, 0, pred)
        np.testing.assert_array_equal(got[0], mv)
        np.testing.assert_array_equal(got[1], cost)
        np.testing.assert_array_equal(got[2], cost)


@pytest.mark.parametrize("pred_seed", [None, 9])
def test_rate_falls_and_distortion_rises_with_lambda(pred_seed):
    """For exact minimisers of D + lam R: lam1 < lam2 gives R1 >= R2 and
    D1 <= D2 (add the two optimality inequalities), on every block."""
    w, h = 96, 64
    ref, cur = _pair(w, h, 11)
    pred = None if pred_seed is None else _preds(me.num_blocks(w, h, 16), pred_seed)
    prev = None
    for lam in (0, 1, 4, 16, 64, 256, 4096, 1 << 20):
        _, _, D, Rb = R.search_frame(ref, cur, 16, 7, lam, pred)
        if prev is not None:
            assert (Rb <= prev[1]).all() and (D >= prev[0]).all(), lam
        prev = (D, Rb)


# ---- Foreman 1 -> 2, 16x16, +-7, zero predictor: (lambda, sum D, sum R, zero vectors, sum J)
FOREMAN = [(0, 290804, 3730, 125, 290804), (1, 290893, 3586, 129, 294479),
           (4, 291719, 3238, 156, 304671), (16, 294967, 2882, 187, 341079),
           (64, 321438, 2168, 250, 460190), (256, 472554, 1056, 367, 742890),
           (1 << 20, 565944, 792, 396, 831038136)]


def test_foreman_table():
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    for lam, *want in FOREMAN:
        assert R.summary(*R.search_frame(ref, cur, 16, 7, lam)) == tuple(want), lam


# ---- refinement
@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_refinement_at_lambda_zero_is_the_plain_refinement(cost):
    ref, cur = _pair(50, 30, 4)
    mv, _, _ = O.full_search(ref, cur, 16, 4, "sad")
    q, c = Q.refine(ref, cur, 16, mv, cost)
    got = R.refine(ref, cur, 16, mv, 0, _preds(len(mv), 2), cost)
    np.testing.assert_array_equal(got[0], q)
    np.testing.assert_array_equal(got[1], c)
    np.testing.assert_array_equal(got[2], c)


def test_refinement_cost_is_distortion_plus_rate():
    ref, cur = _pair(50, 30, 4)
    mv, _, _ = O.full_search(ref, cur, 16, 4, "sad")
    pred = (4 * mv + 1).astype(np.int16)
    q, J, D = R.refine(ref, cur, 16, mv, 16, pred, "sad")
    rate = R.bits(q[:, 0].astype(np.int64) - pred[:, 0]) + R.bits(q[:, 1].astype(np.int64) - pred[:, 1])
    np.testing.assert_array_equal(J.astype(np.int64), D.astype(np.int64) + 16 * rate)
    # a large lambda pulls every block onto its predictor, one quarter step away
    q, _, _ = R.refine(ref, cur, 16, mv, 1 << 24, pred, "sad")
    np.testing.assert_array_equal(q, pred)


# ---- which kernel runs: every shape of tests/test_gpu_rd.py
FAST_SHAPES = [(96, 64, 96, 0), (96, 64, 96, 1), (96, 64, 96, 7), (96, 64, 96, 32),
               (96, 64, 96, 64), (160, 112, 160, 7), (100, 72, 100, 7), (96, 64, 128, 7),
               (352, 288, 352, 7), (96, 64, 96, 48), (96, 64, 96, 56), (160, 160, 160, 64)]
GENERIC_SHAPES = [(90, 50, 90, 16, 7), (40, 24, 40, 8, 7), (70, 40, 70, 32, 4), (23, 17, 23, 5, 3),
                  (130, 70, 130, 64, 2), (48, 32, 48, 16, 128)]


@pytest.mark.parametrize("w,h,pitch,S", FAST_SHAPES)
def test_kernel_variant_fast_shapes(w, h, pitch, S):
    for lam in (0, 1, 16, 4096, FAST_LAM):
        assert me.rd_kernel_variant(w, h, pitch, 16, S, lam) == FAST
    for lam in (FAST_LAM + 1, 1 << 20, 1 << 24):
        assert me.rd_kernel_variant(w, h, pitch, 16, S, lam) == GENERIC


@pytest.mark.parametrize("w,h,pitch,B,S", GENERIC_SHAPES)
def test_kernel_variant_generic_shapes(w, h, pitch, B, S):
    for lam in (0, 16, 1 << 24):
        assert me.rd_kernel_variant(w, h, pitch, B, S, lam) == GENERIC


def test_kernel_variant_bound_and_frame_size():
    # the lane key J << 6 | index holds J < 2^26: the bound is the last lambda that fits
    assert 66 * FAST_LAM + 65280 < 1 << 26 <= 66 * (FAST_LAM + 1) + 65280
    # decided by B, S, the row alignment and lambda, never by the frame size
    for w, h in ((16, 16), (96, 64), (1920, 1080), (3840, 2160)):
        assert me.rd_kernel_variant(w, h, w, 16, 64, 16) == FAST
        assert me.rd_kernel_variant(w, h, w, 16, 65, 16) == GENERIC
        assert me.rd_kernel_variant(w, h, w + 2, 16, 7, 16) == GENERIC
    assert me.rd_kernel_variant(12, 64, 12, 16, 7, 16) == GENERIC  # no full-size block


@pytest.mark.parametrize("args", [
    (96, 64, 96, 16, 129, 16),              # range above ME_RD_MAX_RANGE
    (96, 64, 96, 16, -1, 16),               # negative range
    (96, 64, 96, 16, 7, (1 << 24) + 1),     # lambda above ME_RD_MAX_LAMBDA
    (96, 64, 96, 0, 7, 16), (96, 64, 96, 65, 7, 16),  # block size
    (0, 64, 96, 16, 7, 16), (96, 0, 96, 16, 7, 16), (96, 64, 95, 16, 7, 16),
    (96, 64, 96, 16, 7, -1),
])
def test_kernel_variant_rejects(args):
    assert me.rd_kernel_variant(*args) == -1
