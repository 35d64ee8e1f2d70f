"""The quarter-pel oracle (tests/qpel_ref.py) checked against itself and the
integer oracle (CPU suite): integer vectors reproduce the integer compensation,
half samples obey the 6-tap rule on hand-computed cases, refinement never
raises a block's cost, and on Foreman 1 -> 2 (16x16, +-7) the cost sums and
PSNRs are the ones a separate prototype of the same definition gave."""
import numpy as np
import pytest

import oracle_lib as O
import qpel_ref as Q


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w)).astype(np.uint8),
            rng.integers(0, 256, (h, w)).astype(np.uint8))


def _in_frame_field(w, h, blk, seed):
    """Random integer vectors that keep every block inside the frame."""
    rng = np.random.default_rng(seed)
    mv = []
    for x0, y0, bw, bh in Q._blocks(w, h, blk):
        mv.append((rng.integers(-x0, w - bw - x0 + 1), rng.integers(-y0, h - bh - y0 + 1)))
    return np.array(mv, np.int16)


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (50, 40, 8), (64, 64, 64), (7, 5, 4)])
def test_integer_vectors_equal_integer_compensation(w, h, blk):
    ref, _ = _frames(w, h, 1)
    mv = _in_frame_field(w, h, blk, 2)
    np.testing.assert_array_equal(Q.compensate(ref, blk, 4 * mv), O.motion_compensate(ref, blk, mv))


def test_half_samples_by_hand():
    # a flat plane stays flat at every phase
    flat = np.full((9, 11), 77, np.uint8)
    assert (Q.half_plane(flat, -6, 30, -6, 26) == 77).all()
    # one row 0 0 0 255 255 255: the half sample on the edge is
    # (1*0 - 5*0 + 20*0 + 20*255 - 5*255 + 255 + 16) >> 5 = 128
    row = np.array([[0, 0, 0, 255, 255, 255]], np.uint8)
    P = Q.half_plane(row, 0, 11, 0, 1)[0]
    assert list(P[0::2]) == [0, 0, 0, 255, 255, 255]
    assert P[5] == (20 * 255 - 5 * 255 + 255 + 16) >> 5 == 128
    # next to it the filter overshoots and clip255 cuts both ways
    assert P[3] == 0 and (-5 * 255 + 255 + 16) >> 5 < 0
    assert P[7] == 255 and (20 * 255 + 20 * 255 - 5 * 255 + 16) >> 5 > 255
    # the centre sample filters the unrounded intermediates: on a plane that
    # varies along x only, j1 = 32 * b1, so it equals the horizontal half sample
    cols = np.tile(np.array([10, 200, 30, 90, 250, 0, 60, 120], np.uint8), (8, 1))
    P = Q.half_plane(cols, 0, 15, 0, 15)
    np.testing.assert_array_equal(P[1::2, 1::2], P[0:-1:2, 1::2])


def test_quarter_samples_average_the_right_neighbours():
    ref, _ = _frames(12, 10, 3)
    P = Q.half_plane(ref, 0, 24, 0, 20).astype(int)
    B = Q._Block(ref, 4, 3, 2, 2)
    X, Y = 8, 6  # half coordinates of the block's first pixel
    avg = lambda a, b: (a + b + 1) >> 1
    assert B.predict(16, 12)[0, 0] == P[Y, X] == ref[3, 4]
    assert B.predict(17, 12)[0, 0] == avg(P[Y, X], P[Y, X + 1])        # a
    assert B.predict(19, 12)[0, 0] == avg(P[Y, X + 1], P[Y, X + 2])    # c
    assert B.predict(16, 13)[0, 0] == avg(P[Y, X], P[Y + 1, X])        # d
    assert B.predict(17, 13)[0, 0] == avg(P[Y, X + 1], P[Y + 1, X])    # e: b and h
    assert B.predict(19, 13)[0, 0] == avg(P[Y, X + 1], P[Y + 1, X + 2])  # g: b and m
    assert B.predict(17, 15)[0, 0] == avg(P[Y + 1, X], P[Y + 2, X + 1])  # p: h and s
    assert B.predict(19, 15)[0, 0] == avg(P[Y + 1, X + 2], P[Y + 2, X + 1])  # r: m and s
    assert B.predict(15, 11)[0, 0] == avg(P[Y - 1, X], P[Y, X - 1])    # negative fractions
    assert B.predict(18, 14)[1, 1] == P[Y + 3, X + 3]                  # j of the next pixel


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (23, 9, 4), (50, 40, 64), (40, 3, 1)])
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_whole_frame_form_equals_block_by_block(w, h, blk, cost):
    """refine / compensate work on whole frames with a clamped lookup; the
    block-by-block loop words the definition literally.  Vectors inside,
    across and far outside the frame."""
    rng = np.random.default_rng(7 * w + h)
    ref, cur = _frames(w, h, 5)
    n = O.num_blocks(w, h, blk)
    for mv in (rng.integers(-6, 7, (n, 2)), rng.integers(-2 * w, 2 * w, (n, 2)),
               np.tile([[w, -h]], (n, 1)), np.tile([[-8000, 8000]], (n, 1))):
        q, c = Q.refine(ref, cur, blk, mv, cost)
        qb, cb = Q.refine_blockwise(ref, cur, blk, mv, cost)
        np.testing.assert_array_equal(q, qb)
        np.testing.assert_array_equal(c, cb)
        np.testing.assert_array_equal(Q.compensate(ref, blk, q), Q.compensate_blockwise(ref, blk, q))
    qr = rng.integers(-32768, 32768, (n, 2))
    np.testing.assert_array_equal(Q.compensate(ref, blk, qr), Q.compensate_blockwise(ref, blk, qr))


def test_checkerboard_reaches_both_clip_ends():
    """The premise of the GPU tests' checkerboard frames: on the 0/255 board of
    period 3 each of the three rounding sites (horizontal, vertical, centre)
    is cut at 0 and at 255 somewhere."""
    yy, xx = np.mgrid[0:17, 0:33]
    pad = np.pad((((xx // 3 + yy // 3) & 1) * 255).astype(np.int64), 3, mode="edge")
    b1, h1 = Q._fir(pad, 1), Q._fir(pad, 0)
    for v, rnd, sh in ((b1, 16, 5), (h1, 16, 5), (Q._fir(b1, 0), 512, 10)):
        t = (v + rnd) >> sh
        assert t.min() < 0 and t.max() > 255


FOREMAN = {  # cost: (integer sum, refined sum, integer PSNR, refined PSNR) of the prototype
    "ssd": (2485420, 1633942, 34.230, 36.052),
    "sad": (290804, 228712, 34.067, 35.960),
}


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_foreman_refinement_figures(cost):
    """The cost sums are the prototype's, exactly.  Its four PSNR figures all
    sit 0.006 dB below oracle_lib.psnr (34.236 / 36.058 SSD, 34.073 / 35.966
    SAD), the integer field's included, which involves nothing of this
    definition; and for SSD the PSNR follows from the cost sum itself (the
    frame's sum of squares is the sum of the block SSDs, MAX is 255 in these
    frames): 20 log10(255) - 10 log10(2485420 / 101376) = 34.236.  So the
    prototype's PSNR rule differed from the reference's by a constant; the
    test pins the PSNR to the cost sums exactly, the gain to the prototype's
    three decimals, and the absolute figures to 0.01 dB."""
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    mv, c, _ = O.full_search(ref, cur, 16, 7, cost)
    q, qc = Q.refine(ref, cur, 16, mv, cost)
    assert (qc <= c).all()
    assert (np.abs(q.astype(int) - 4 * mv.astype(int)) <= 3).all()
    isum, qsum, ipsnr, qpsnr = FOREMAN[cost]
    assert int(c.astype(np.int64).sum()) == isum
    assert int(qc.astype(np.int64).sum()) == qsum
    np.testing.assert_array_equal(Q.compensate(ref, 16, 4 * mv), O.motion_compensate(ref, 16, mv))
    mc = Q.compensate(ref, 16, q)
    pi, pq = O.psnr(O.motion_compensate(ref, 16, mv), cur), O.psnr(mc, cur)
    assert max(int(ref.max()), int(cur.max())) == 255
    if cost == "ssd":
        of_sum = lambda s: 20 * np.log10(255) - 10 * np.log10(s / (352 * 288))
        assert abs(pi - of_sum(isum)) < 1e-12 and abs(pq - of_sum(qsum)) < 1e-12
    assert abs((pq - pi) - (qpsnr - ipsnr)) < 5e-4
    assert abs(pi - ipsnr) < 0.01 and abs(pq - qpsnr) < 0.01
    # the vacuity guard of the GPU end-to-end test holds with room to spare
    assert np.mean((q % 4 != 0).any(axis=1)) >= 0.85 and np.mean((q % 2 != 0).any(axis=1)) >= 0.7
    # the refined cost is the cost of the compensated block
    d = mc.astype(np.int64) - cur
    per_blk = (np.abs(d) if cost == "sad" else d * d).reshape(18, 16, 22, 16).sum(axis=(1, 3)).ravel()
    np.testing.assert_array_equal(per_blk, qc)
