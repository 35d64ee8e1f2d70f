"""The partition search's numpy restatement (tests/partition_ref.py) and the
host-only side of the feature (CPU suite): the restatement's two forms agree,
its 2Nx2N field is the oracle's full search and the NxN records of unclamped
macroblocks the oracle's B/2 search, Foreman 1 -> 2 (16x16, +-7, SAD) gives the
figures DESIGN.md quotes, and me_partition_counts, me_partition_kernel_variant
and me_partition_leaf_field behave as include/me.h says."""
import ctypes

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_ref as P
from motionestimation_amd import _lib

# the small frame the GPU suite runs on the fast kernel
FAST_SHAPE = (96, 64)


def _pair(w, h, seed, shift=(2, -3)):
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    # smooth a little so that minima are not all isolated
    big = ((big.astype(np.uint16) + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) // 4)
    big = big.astype(np.uint8)
    ref = big[8:8 + h, 8:8 + w]
    cur = big[8 + shift[1]:8 + shift[1] + h, 8 + shift[0]:8 + shift[0] + w]
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


def _same(a, b):
    for k in range(4):
        np.testing.assert_array_equal(a.mv[k], b.mv[k], err_msg=P.MODES[k])
        np.testing.assert_array_equal(a.cost[k], b.cost[k], err_msg=P.MODES[k])
    np.testing.assert_array_equal(a.mode, b.mode)
    np.testing.assert_array_equal(a.mode_cost, b.mode_cost)


@pytest.fixture(scope="module")
def foreman():
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    return ref, cur, P.search_frame(ref, cur, 16, 7, 0)


@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 5), (9, 9, 16, 3), (40, 24, 8, 7),
                                      (70, 40, 32, 4), (33, 17, 16, 40)])
def test_two_forms_agree(w, h, B, S):
    ref, cur = _pair(w, h, w * h + B)
    _same(P.search_loops(ref, cur, B, S, 16), P.search_frame(ref, cur, B, S, 16))


def test_two_forms_agree_on_ties():
    flat = np.full((28, 44), 7, np.uint8)
    _same(P.search_loops(flat, flat, 16, 4, 0), P.search_frame(flat, flat, 16, 4, 0))


@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 5), (70, 40, 32, 9), (40, 24, 8, 3)])
def test_2nx2n_is_the_full_search(w, h, B, S):
    ref, cur = _pair(w, h, 3)
    F = P.search_frame(ref, cur, B, S)
    mv, cost, _ = O.full_search(ref, cur, B, S, "sad")
    np.testing.assert_array_equal(F.mv[0], mv)
    np.testing.assert_array_equal(F.cost[0], cost)


@pytest.mark.parametrize("w,h,B,S", [(96, 80, 16, 7), (128, 96, 32, 5)])
def test_nxn_of_unclamped_macroblocks_is_the_half_size_search(w, h, B, S):
    ref, cur = _pair(w, h, 5)
    F = P.search_frame(ref, cur, B, S)
    mv, cost, _ = O.full_search(ref, cur, B // 2, S, "sad")
    (nbx, nby), (nhx, _) = P.grids(w, h, B)[0], P.grids(w, h, B)[3]
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
                    cell = (2 * by + j) * nhx + 2 * bx + i
                    assert tuple(F.mv[3][cell]) == tuple(mv[cell]), (bx, by, i, j)
                    assert F.cost[3][cell] == cost[cell]
                    seen += 1
    assert seen >= 8


def test_foreman_field_sums(foreman):
    _, _, F = foreman
    sums = [int(c.astype(np.int64).sum()) for c in F.cost]
    assert sums == [290804, 275534, 274959, 255385]


@pytest.mark.parametrize("lam,hist,sum_j,sum_d", [
    (0, [77, 18, 10, 291], 255385, 255385),
    (16, [207, 56, 48, 85], 271059, 258979),
    (64, [299, 40, 36, 21], 300737, 266497),
    (256, [377, 6, 12, 1], 387209, 280457),
    (100000, [396, 0, 0, 0], 39890804, 290804)])
def test_foreman_mode_table(foreman, lam, hist, sum_j, sum_d):
    ref, cur, F = foreman
    F = P.decide(F, lam)
    assert P.summary(F, lam) == (hist, sum_j, sum_d)
    if lam == 0:  # every macroblock is full size here: NxN is never beaten
        assert sum_j == int(F.cost[3].astype(np.int64).sum())
    # the leaf field through the library's host function and the oracle's
    # integer compensation at B / 2 reproduces the distortion
    fields = me.PartitionFields(F.mv, None, F.mode, None)
    leaf = me.partition_leaf_field(352, 288, 16, fields)
    np.testing.assert_array_equal(leaf, P.leaf_field(F))
    mc = O.motion_compensate(ref, 8, leaf)
    assert int(np.abs(mc.astype(np.int32) - cur.astype(np.int32)).sum()) == sum_d


def test_leaf_field_on_clipped_frame():
    ref, cur = _pair(44, 28, 11)
    F = P.search_frame(ref, cur, 16, 5, 16)
    assert len(set(F.mode.tolist())) > 1
    leaf = me.partition_leaf_field(44, 28, 16, me.PartitionFields(F.mv, None, F.mode, None))
    np.testing.assert_array_equal(leaf, P.leaf_field(F))
    mc = O.motion_compensate(ref, 8, leaf)
    _, _, dist = P.summary(F, 16)
    assert int(np.abs(mc.astype(np.int32) - cur.astype(np.int32)).sum()) == dist


def test_leaf_field_rejects_bad_mode_and_nulls():
    F = P.search_frame(*_pair(32, 32, 2), 16, 2, 0)
    F.mode[1] = 4
    with pytest.raises(me.MEError) as e:
        me.partition_leaf_field(32, 32, 16, me.PartitionFields(F.mv, None, F.mode, None))
    assert e.value.status == _lib.ME_EINVAL
    L = _lib.lib()
    leaf = np.zeros((16, 2), np.int16)
    assert L.me_partition_leaf_field(32, 32, 16, None, leaf.ctypes.data) == _lib.ME_EINVAL
    st = me.PartitionFields(F.mv, None, F.mode, None).struct()
    st.mv_nx2n = None
    assert L.me_partition_leaf_field(32, 32, 16, ctypes.byref(st), leaf.ctypes.data) == _lib.ME_EINVAL


@pytest.mark.parametrize("w,h,B", [(352, 288, 16), (1920, 1080, 16), (9, 9, 16), (33, 17, 16),
                                    (44, 28, 16), (40, 24, 8), (70, 40, 32), (100, 75, 16)])
def test_partition_counts(w, h, B):
    assert me.partition_counts(w, h, B) == P.counts(w, h, B)
    assert me.partition_counts(w, h, B)[0] == me.num_blocks(w, h, B)
    assert me.partition_counts(w, h, B)[3] == me.num_blocks(w, h, B // 2)


def test_partition_counts_rejects():
    L = _lib.lib()
    out = (ctypes.c_int * 4)()
    for args in [(0, 10, 16), (10, -1, 16), (10, 10, 0), (10, 10, 7)]:
        assert L.me_partition_counts(*args, out) == _lib.ME_EINVAL, args
    assert L.me_partition_counts(16, 16, 16, None) == _lib.ME_EINVAL


FAST, GENERIC = _lib.ME_PART_KERNEL_FAST, _lib.ME_PART_KERNEL_GENERIC


@pytest.mark.parametrize("w,h,stride,B,S,want", [
    (1920, 1080, 1920, 16, 32, FAST),
    (3840, 2160, 3840, 16, 64, FAST),
    (FAST_SHAPE[0], FAST_SHAPE[1], FAST_SHAPE[0], 16, 7, FAST),
    (FAST_SHAPE[0], FAST_SHAPE[1], FAST_SHAPE[0], 16, 16, FAST),
    (256, 144, 256, 16, 32, FAST),
    (352, 288, 352, 16, 7, FAST),
    (100, 64, 112, 16, 7, FAST),       # rows of 112 bytes: aligned
    (1920, 1080, 1920, 8, 32, GENERIC),
    (1920, 1080, 1920, 32, 32, GENERIC),
    (96, 64, 99, 16, 7, GENERIC),      # unaligned pitch
    (98, 64, 100, 16, 7, GENERIC),     # width no multiple of 4
    (1920, 1080, 1920, 16, 65, GENERIC),
    (9, 9, 12, 16, 3, GENERIC),        # no full-size macroblock
    # rejected by the search
    (1920, 1080, 1920, 12, 32, -1),
    (1920, 1080, 1920, 16, 129, -1),
    (1920, 1080, 1919, 16, 32, -1),
    (0, 1080, 1920, 16, 32, -1),
    (1920, 1080, 1920, 16, -1, -1),
    (65536, 32768, 65536, 16, 32, -1),
])
def test_kernel_variant_is_pinned(w, h, stride, B, S, want):
    assert me.partition_kernel_variant(w, h, stride, B, S) == want


def test_variant_does_not_depend_on_frame_size():
    for w, h in [(16, 16), (64, 48), (352, 288), (4096, 2304)]:
        assert me.partition_kernel_variant(w, h, w, 16, 32) == FAST


def test_constants_match_header():
    src = open(O.REPO + "/include/me.h").read()
    assert "#define ME_PART_MAX_RANGE 128" in src
    assert "#define ME_PART_MAX_LAMBDA (1u << 24)" in src
    assert (me.ME_PART_MAX_RANGE, me.ME_PART_MAX_LAMBDA) == (128, 1 << 24)
    assert (me.ME_PART_2Nx2N, me.ME_PART_2NxN, me.ME_PART_Nx2N, me.ME_PART_NxN) == (0, 1, 2, 3)
