"""The bi-prediction oracle (tests/bipred_ref.py) checked against itself (CPU
suite): the whole-frame form equals the literal block-by-block form, the
degenerate cases come out as the definition says, the refinement never raises a
cost and moves each vector by at most a quarter step, the block cost is the
cost of the compensated block, and on Foreman 1 -> 2 <- 4 (16x16, +-7) the cost
sums and mode histograms are the ones a separate prototype of the same
definition gave."""
import functools

import numpy as np
import pytest

import bipred_ref as B
import oracle_lib as O


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(3))


def _equal(a, b, msg=""):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=msg)


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (23, 9, 4), (50, 40, 64), (40, 3, 1)])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_whole_frame_form_equals_block_by_block(w, h, blk, cost):
    """Vectors inside, across and far outside the frame, refine 0 and 1."""
    rng = np.random.default_rng(11 * w + h)
    ref0, ref1, cur = _frames(w, h, 3)
    n = O.num_blocks(w, h, blk)
    fields = [(rng.integers(-24, 25, (n, 2)), rng.integers(-24, 25, (n, 2))),
              (rng.integers(-8 * w, 8 * w, (n, 2)), rng.integers(-8 * h, 8 * h, (n, 2))),
              (np.tile([[4 * w + 1, -4 * h - 3]], (n, 1)), np.tile([[-4 * w - 2, 4 * h + 1]], (n, 1))),
              (np.tile([[B.MAX_Q, -B.MAX_Q]], (n, 1)), np.tile([[-B.MAX_Q, B.MAX_Q]], (n, 1)))]
    for q0, q1 in fields:
        for refine in (0, 1):
            got = B.bipred(ref0, ref1, cur, blk, q0, q1, cost, refine)
            _equal(got, B.bipred_blockwise(ref0, ref1, cur, blk, q0, q1, cost, refine))
            o0, o1, mode = got[:3]
            np.testing.assert_array_equal(B.compensate(ref0, ref1, blk, o0, o1, mode),
                                          B.compensate_blockwise(ref0, ref1, blk, o0, o1, mode))
    # the compensation alone: any int16 vectors, every mode
    v0, v1 = rng.integers(-32768, 32768, (n, 2)), rng.integers(-32768, 32768, (n, 2))
    mode = rng.integers(0, 3, n)
    np.testing.assert_array_equal(B.compensate(ref0, ref1, blk, v0, v1, mode),
                                  B.compensate_blockwise(ref0, ref1, blk, v0, v1, mode))


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_same_reference_same_vector_is_l0(cost):
    """ref0 == ref1 and q0 == q1: the average of a block with itself is the
    block, the three costs are equal and the tie goes to L0."""
    ref, _, cur = _frames(50, 40, 5)
    n = O.num_blocks(50, 40, 8)
    q = np.random.default_rng(6).integers(-30, 31, (n, 2))
    o0, o1, mode, bc, c3 = B.bipred(ref, ref, cur, 8, q, q, cost, 0)
    np.testing.assert_array_equal(c3[:, 0], c3[:, 1])
    np.testing.assert_array_equal(c3[:, 0], c3[:, 2])
    assert not mode.any()
    np.testing.assert_array_equal(bc, c3[:, 0])
    np.testing.assert_array_equal(o0, q)
    np.testing.assert_array_equal(o1, q)


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_flat_references_keep_l0_and_the_vectors(cost):
    """Every candidate costs the same: nothing is strictly smaller."""
    _, _, cur = _frames(33, 17, 7)
    flat = np.full((17, 33), 120, np.uint8)
    n = O.num_blocks(33, 17, 16)
    rng = np.random.default_rng(8)
    q0, q1 = rng.integers(-20, 21, (n, 2)), rng.integers(-20, 21, (n, 2))
    o0, o1, mode, bc, c3 = B.bipred(flat, flat, cur, 16, q0, q1, cost, 1)
    assert not mode.any()
    np.testing.assert_array_equal(o0, q0)
    np.testing.assert_array_equal(o1, q1)
    np.testing.assert_array_equal(c3[:, 2], c3[:, 0])


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (130, 75, 8), (70, 40, 32)])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_refinement_properties(w, h, blk, cost):
    ref0, ref1, cur, q0, q1 = B.planted(w, h, blk, 100 + w)
    plain = B.bipred(ref0, ref1, cur, blk, q0, q1, cost, 0)
    o0, o1, mode, bc, c3 = B.bipred(ref0, ref1, cur, blk, q0, q1, cost, 1)
    # cb with refinement <= cb without; c0 and c1 do not depend on it
    assert (c3[:, 2] <= plain[4][:, 2]).all()
    np.testing.assert_array_equal(c3[:, :2], plain[4][:, :2])
    # |b - q| <= 1 per component, and only BI blocks carry a moved vector
    assert (np.abs(o0.astype(int) - q0) <= 1).all() and (np.abs(o1.astype(int) - q1) <= 1).all()
    moved = (o0 != q0).any(axis=1) | (o1 != q1).any(axis=1)
    assert not moved[mode != B.BI].any()
    np.testing.assert_array_equal(bc, c3.min(axis=1))
    # block_cost is the cost recomputed from the compensated frame
    for got in (plain, (o0, o1, mode, bc, c3)):
        mc = B.compensate(ref0, ref1, blk, got[0], got[1], got[2])
        np.testing.assert_array_equal(B.block_costs(cur, mc, blk, cost), got[3])


@functools.lru_cache(maxsize=None)
def foreman_inputs(cost):
    out = B.foreman(cost)
    for a in out:
        a.setflags(write=False)
    return out


FOREMAN = {  # cost: (L0 alone, L1 alone, best of three unrefined, refined, its modes L0 / L1 / BI)
    "ssd": (1633942, 6477577, 1195662, 1146937, (120, 31, 245)),
    "sad": (228712, 414129, 200931, 194980, (120, 21, 255)),
}


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_foreman_figures(cost):
    ref0, ref1, cur, q0, c0, q1, c1 = foreman_inputs(cost)
    s0, s1, plain_sum, refined_sum, hist = FOREMAN[cost]
    total = lambda a: int(a.astype(np.int64).sum())
    assert total(c0) == s0 and total(c1) == s1
    plain = B.bipred(ref0, ref1, cur, 16, q0, q1, cost, 0)
    o0, o1, mode, bc, c3 = B.bipred(ref0, ref1, cur, 16, q0, q1, cost, 1)
    np.testing.assert_array_equal(c3[:, 0], c0)
    np.testing.assert_array_equal(c3[:, 1], c1)
    assert total(plain[3]) == plain_sum
    assert total(bc) == refined_sum
    assert tuple(np.bincount(mode, minlength=3)) == hist
    mc = B.compensate(ref0, ref1, 16, o0, o1, mode)
    np.testing.assert_array_equal(B.block_costs(cur, mc, 16, cost), bc)
    if cost == "ssd":
        # the PSNR that follows from the sum (MAX is 255 in these frames)
        assert max(int(mc.max()), int(cur.max())) == 255
        psnr = O.psnr(mc, cur)
        assert abs(psnr - (20 * np.log10(255) - 10 * np.log10(refined_sum / (352 * 288)))) < 1e-12
        assert abs(psnr - 37.595) < 0.001
