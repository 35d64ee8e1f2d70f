"""The post-processing kernel (csrc/me_post.hip: motion compensation, the
residual planes, PSNR's sum of squares and MAX) against the oracle's
motionCompensatedFrame / imagePSNR (utils.c:94-164) and numpy, at geometries
Foreman CIF with searched MVs never meets: a pixel count that is no multiple of
the lane's 4 pixels, partial blocks, MVs that leave the frame, blocks of one
pixel and blocks larger than the frame, MAX taken from the data, identical
frames, and enough workgroups for the two atomics to matter.

Planes are compared byte for byte and PSNR with == as doubles: both sides
evaluate 20 log10(MAX) - 10 log10(sum / n) in host double arithmetic from an
exact integer sum below 2^53."""
import numpy as np
import pytest

import oracle_lib as O
import motionestimation_amd as me
from motionestimation_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [
    (7, 5, 4),        # 35 pixels: the last lane stops after 3
    (33, 17, 16),     # partial blocks right and below
    (130, 75, 8),     # several workgroups
    (641, 363, 16),   # 228 workgroups on the two atomics
    (1025, 3, 1),     # one-pixel blocks
    (64, 64, 64),     # the block is the frame
    (50, 40, 64),     # the block is larger than the frame
]
FIELDS = ["zeros", "near", "int16", "outside"]


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w)).astype(np.uint8),
            rng.integers(0, 256, (h, w)).astype(np.uint8))


def _field(kind, w, h, blk, seed):
    n = me.num_blocks(w, h, blk)
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((n, 2), np.int16)
    if kind == "near":
        return rng.integers(-12, 13, (n, 2)).astype(np.int16)
    if kind == "int16":
        mv = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        mv[0] = (-32768, 32767)
        mv[-1] = (32767, -32768)
        return mv
    # every pixel of every block lands outside the frame
    away = np.array([(w, 0), (-w, 0), (0, h), (0, -h), (w, -h)], np.int16)
    return away[rng.integers(0, len(away), n)]


def _expect(ref, cur, blk, mv):
    mc = O.motion_compensate(ref, blk, mv)
    d = lambda a, b: np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)
    return mc, np.concatenate([ref, cur, mc, d(ref, cur), d(mc, cur)]), O.psnr(mc, cur)


def _check(eng, ref, cur, blk, mv, msg):
    mc, planes, psnr = _expect(ref, cur, blk, mv)
    out, got = eng.compensate_planes(ref, cur, blk, mv)
    np.testing.assert_array_equal(out, planes, err_msg=msg)
    assert got == psnr, (msg, got, psnr)
    np.testing.assert_array_equal(eng.motion_compensate(ref, blk, mv), mc, err_msg=msg)
    return mc, got


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_compensate_planes_and_psnr(engine, w, h, blk, kind):
    ref, cur = _frames(w, h, 100 + w)
    mv = _field(kind, w, h, blk, 200 + h)
    mc, _ = _check(engine, ref, cur, blk, mv, f"{w}x{h} B{blk} {kind}")
    if kind == "zeros":
        np.testing.assert_array_equal(mc, ref)
    if kind == "outside":
        assert not mc.any()


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (130, 75, 8)])
def test_psnr_edges(engine, w, h, blk):
    """imagePSNR's branches: mse == 0 -> 99.0, and MAX = the largest pixel of
    either plane (utils.c:137-164), never 255 by default."""
    rng = np.random.default_rng(300 + w)
    zero = np.zeros((me.num_blocks(w, h, blk), 2), np.int16)
    near = _field("near", w, h, blk, 301)
    ref, cur = _frames(w, h, 302)
    # identical planes, zero MVs; all-zero planes (MAX = 0 is never used)
    assert _check(engine, ref, ref, blk, zero, "ref == cur")[1] == 99.0
    black = np.zeros((h, w), np.uint8)
    assert _check(engine, black, black, blk, near, "black")[1] == 99.0
    # dark planes: MAX from the data
    dref = rng.integers(0, 18, (h, w)).astype(np.uint8)
    dcur = rng.integers(0, 18, (h, w)).astype(np.uint8)
    _, p = _check(engine, dref, dcur, blk, near, "pixels <= 17")
    mcd = O.motion_compensate(dref, blk, near).astype(np.int64)
    mx = int(max(mcd.max(), dcur.max()))
    assert mx <= 17
    mse = float(((mcd - dcur) ** 2).sum()) / (w * h)
    assert abs(p - (20 * np.log10(mx) - 10 * np.log10(mse))) < 1e-9
    # MAX present only in cur, then only in mc (= ref under zero MVs)
    lo_ref = rng.integers(0, 101, (h, w)).astype(np.uint8)
    lo_cur = rng.integers(0, 101, (h, w)).astype(np.uint8)
    hi_cur = lo_cur.copy()
    hi_cur[h // 2, w - 1] = 231
    _check(engine, lo_ref, hi_cur, blk, near, "MAX in cur")
    hi_ref = lo_ref.copy()
    hi_ref[h - 1, w // 3] = 231
    mc, _ = _check(engine, hi_ref, lo_cur, blk, zero, "MAX in mc")
    assert mc.max() == 231 and lo_cur.max() <= 100


def test_post_shares_the_context_with_searches():
    """Searches and post-processing of different sizes share one context's
    planes and records: each call equals its reference."""
    with me.Engine(devices=[0]) as eng:
        ref, cur = synth.frame_pair(176, 144, 5, 2, -3)
        mv, c = eng.full_search(ref, cur, 16, 8, "sad")
        omv, oc, _ = O.full_search(ref, cur, 16, 8, "sad", threads=16)
        np.testing.assert_array_equal(mv, omv)
        np.testing.assert_array_equal(c, oc)
        _, planes, psnr = _expect(ref, cur, 16, mv)
        out, got = eng.compensate_planes(ref, cur, 16, mv)
        np.testing.assert_array_equal(out, planes)
        assert got == psnr
        ref2, cur2 = synth.frame_pair(330, 200, 6, -4, 1)
        mv2, c2 = eng.full_search(ref2, cur2, 8, 12, "ssd")
        omv2, oc2, _ = O.full_search(ref2, cur2, 8, 12, "ssd", threads=16)
        np.testing.assert_array_equal(mv2, omv2)
        np.testing.assert_array_equal(c2, oc2)
        np.testing.assert_array_equal(eng.motion_compensate(ref2, 8, mv2),
                                      O.motion_compensate(ref2, 8, mv2))
        # and back to the first size: planes shrink in use, not in capacity
        out, got = eng.compensate_planes(ref, cur, 16, mv)
        np.testing.assert_array_equal(out, planes)
        assert got == psnr
        eng.device_check()
