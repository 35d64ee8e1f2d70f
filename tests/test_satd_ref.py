"""The SATD oracle (tests/satd_ref.py) checked against itself and by hand (CPU
suite): its block-by-block and whole-frame forms agree, hand-worked tiles give
the figures the definition implies, sum |T| is even, the two identities of
include/me.h "SATD cost" hold on blocks of every size from 1x1 to 9x9, and on
Foreman 1 -> 2 (16x16, +-7) the figures DESIGN.md "SATD cost" records are the
ones the oracle gives."""
import numpy as np
import pytest

import oracle_lib as O
import qpel_ref as Q
import satd_ref as S

SHAPES = [(33, 17, 16), (23, 9, 4), (50, 40, 64), (40, 3, 1), (23, 17, 5)]


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w)).astype(np.uint8),
            rng.integers(0, 256, (h, w)).astype(np.uint8))


def _nblocks(w, h, blk):
    return len(list(Q._blocks(w, h, blk)))


# ---------------------------------------------------------- the two forms
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_forms_agree_on_block_costs(w, h, blk):
    cur, pred = _frames(w, h, 1)
    want = [S.satd(cur[y0:y0 + bh, x0:x0 + bw], pred[y0:y0 + bh, x0:x0 + bw])
            for x0, y0, bw, bh in Q._blocks(w, h, blk)]
    np.testing.assert_array_equal(S.block_costs(cur, pred, blk), want)


@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_forms_agree_on_refinement(w, h, blk):
    ref, cur = _frames(w, h, 2)
    rng = np.random.default_rng(3)
    n = _nblocks(w, h, blk)
    mv = rng.integers(-5, 6, (n, 2)).astype(np.int16)
    q, c = S.refine(ref, cur, blk, mv)
    bq, bc = S.refine_blockwise(ref, cur, blk, mv)
    np.testing.assert_array_equal(q, bq)
    np.testing.assert_array_equal(c, bc)
    pred = rng.integers(-40, 41, (n, 2)).astype(np.int16)
    for lam in (16, 1 << 24):
        for a, b in zip(S.refine_rd(ref, cur, blk, mv, lam, pred),
                        S.refine_rd_blockwise(ref, cur, blk, mv, lam, pred)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_forms_agree_on_bipred(w, h, blk):
    ref0, cur = _frames(w, h, 4)
    ref1, _ = _frames(w, h, 5)
    rng = np.random.default_rng(6)
    n = _nblocks(w, h, blk)
    q0 = rng.integers(-9, 10, (n, 2)).astype(np.int16)
    q1 = rng.integers(-9, 10, (n, 2)).astype(np.int16)
    for refine in (0, 1):
        for a, b in zip(S.bipred(ref0, ref1, cur, blk, q0, q1, refine),
                        S.bipred_blockwise(ref0, ref1, cur, blk, q0, q1, refine)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------ by hand
def test_hand_worked_tiles():
    zero = np.zeros((4, 4), np.int64)
    # one non-zero residual d: all 16 coefficients are +-d, sum |T| = 16 |d|
    for d in (1, -7, 255, -255):
        for at in ((0, 0), (2, 3), (3, 1)):
            c = zero.copy()
            c[at] = d
            assert S.satd(c, zero) == 8 * abs(d)
    # a 1x1 block is that tile
    assert S.satd(np.array([[200]]), np.array([[17]])) == 8 * 183
    # a constant residual d over a full tile: only the DC coefficient, 16 d
    for d in (1, -3, 255):
        assert S.satd(np.full((4, 4), d) + 300, np.full((4, 4), 300)) == 8 * abs(d)
    # a +-255 pattern whose 16 coefficients all have magnitude 1020 = 4 * 255:
    # d = 255 * (-1)^(x0 y0 + x1 y1) with x = x0 + 2 x1, y = y0 + 2 y1 (a bent
    # function of the 4 coordinate bits has a flat Hadamard spectrum)
    yy, xx = np.mgrid[0:4, 0:4]
    bent = 255 * (-1) ** ((xx & 1) * (yy & 1) + (xx >> 1) * (yy >> 1))
    t = S.tile_coefficients(bent)
    assert (np.abs(t) == 1020).all()
    assert S.satd(bent, zero) == 8160 == 16 * 1020 // 2
    # a tile's bound: |T| <= 16 * 255 and satd <= 8160 on +-255 residuals
    rng = np.random.default_rng(7)
    for _ in range(200):
        d = 255 * rng.choice([-1, 1], (4, 4))
        assert np.abs(S.tile_coefficients(d)).max() <= 4080
        assert S.satd(d, zero) <= 8160


def test_partial_tiles_are_zero_padded():
    """A 5x3 block is two tiles; its satd is that of the residual written into
    an 8x4 zero plane."""
    rng = np.random.default_rng(8)
    c, p = rng.integers(0, 256, (3, 5)), rng.integers(0, 256, (3, 5))
    big_c, big_p = np.zeros((4, 8), np.int64), np.zeros((4, 8), np.int64)
    big_c[:3, :5], big_p[:3, :5] = c, p
    assert S.satd(c, p) == S.satd(big_c[:, :4], big_p[:, :4]) + S.satd(big_c[:, 4:], big_p[:, 4:])


def test_evenness_and_identities():
    """sum |T| is even (so the shift loses nothing); SAD <= 2 satd <= 16 SAD;
    per tile sum T^2 = 16 sum d^2.  Blocks of every size from 1x1 to 9x9."""
    rng = np.random.default_rng(9)
    for bh in range(1, 10):
        for bw in range(1, 10):
            for _ in range(4):
                c, p = rng.integers(0, 256, (bh, bw)), rng.integers(0, 256, (bh, bw))
                d = np.zeros((12, 12), np.int64)
                d[:bh, :bw] = c - p
                total = 0
                for ty in range(0, 12, 4):
                    for tx in range(0, 12, 4):
                        tile = d[ty:ty + 4, tx:tx + 4]
                        t = S.tile_coefficients(tile)
                        assert int(np.abs(t).sum()) % 2 == 0
                        assert (t % 2 == tile.sum() % 2).all()
                        assert int((t * t).sum()) == 16 * int((tile * tile).sum())
                        total += int(np.abs(t).sum())
                s = S.satd(c, p)
                assert 2 * s == total
                sad = int(np.abs(c - p).sum())
                assert sad <= 2 * s <= 16 * sad


# ------------------------------------------------------- the procedures
@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (23, 17, 5)])
def test_lambda_zero_is_the_plain_refinement(w, h, blk):
    ref, cur = _frames(w, h, 10)
    rng = np.random.default_rng(11)
    n = _nblocks(w, h, blk)
    mv = rng.integers(-5, 6, (n, 2)).astype(np.int16)
    pred = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    q, c = S.refine(ref, cur, blk, mv)
    rq, rj, rd = S.refine_rd(ref, cur, blk, mv, 0, pred)
    np.testing.assert_array_equal(rq, q)
    np.testing.assert_array_equal(rj, c)
    np.testing.assert_array_equal(rd, c)


def test_zero_residual_does_not_move():
    """cur is ref displaced by whole pixels: the integer vector costs 0 and no
    candidate is strictly smaller."""
    rng = np.random.default_rng(12)
    ref = rng.integers(0, 256, (40, 56)).astype(np.uint8)
    cur = np.zeros_like(ref)
    cur[:, :] = Q.compensate(ref, 8, np.tile(np.array([[8, -4]]), (35, 1)))
    mv = np.tile(np.array([[2, -1]], np.int16), (35, 1))
    q, c = S.refine(ref, cur, 8, mv)
    np.testing.assert_array_equal(q, 4 * mv)
    assert not c.any()


def test_refinement_never_raises_the_cost():
    ref, cur = _frames(50, 40, 13)
    mv = np.zeros((_nblocks(50, 40, 16), 2), np.int16)
    before = S.block_costs(cur, Q.compensate(ref, 16, 4 * mv), 16)
    q, c = S.refine(ref, cur, 16, mv)
    assert (c <= before).all()
    np.testing.assert_array_equal(c, S.block_costs(cur, Q.compensate(ref, 16, q), 16))


# The figures DESIGN.md "SATD cost" records: summed satd at the integer field,
# summed satd after the SATD refinement, blocks whose SATD vector differs from
# the SAD refinement's, blocks in all.
FOREMAN = (557829, 424679, 146, 396)


def test_foreman_figures():
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    mv = O.full_search(ref, cur, 16, 7, "sad")[0]
    before = S.block_costs(cur, Q.compensate(ref, 16, 4 * mv), 16)
    q, c = S.refine(ref, cur, 16, mv)
    assert (c <= before).all()
    sq, _ = Q.refine(ref, cur, 16, mv, "sad")
    differ = int((q != sq).any(axis=1).sum())
    got = (int(before.sum()), int(c.astype(np.int64).sum()), differ, len(q))
    print("foreman satd figures:", got)
    assert got == FOREMAN
