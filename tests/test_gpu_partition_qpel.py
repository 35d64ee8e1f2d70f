"""Partition-wise quarter-pel refinement (include/me.h) on the GPU: every record
of all four grids, mode and mode_cost against the numpy restatement
tests/partition_qpel_ref.py bit for bit, over clipped and odd shapes, the three
costs, lambda up to the maximum and predictors over the whole int16 range;
hand-made integer fields; the identities Q1, Q2 and Q5 against the library's own
me_refine_qpel_rd_device and me_compensate_planes_qpel; in-place buffers, NULL
optional arrays, a captured launch, the composite and the host entry points and
every refused argument."""
import ctypes
import functools

import numpy as np
import pytest

import motionestimation_amd as me
import partition_qpel_ref as PQ
import partition_rd_ref as PR
import partition_ref as P
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

TOP_LAM = _lib.ME_PART_RD_MAX_LAMBDA
MAX_MV = _lib.ME_QPEL_MAX_MV


@functools.lru_cache(maxsize=None)
def _content(w, h, tile, seed=7, B=None):
    ref, cur = PQ.content(w, h, tile, seed, B)
    ref.setflags(write=False)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def _searched(w, h, tile, B, S, lam, seed=7, per_b=True):
    """The integer grids of the partition-RD search of a content (the restatement's)."""
    ref, cur = _content(w, h, tile, seed, B if per_b else None)
    return PR.search_frame(ref, cur, B, S, lam).mv


@functools.lru_cache(maxsize=None)
def _want_searched(w, h, tile, B, S, lam, cost, per_b=True, seed=7):
    """The restatement's refinement of a searched content with a NULL predictor."""
    ref, cur = _content(w, h, tile, seed, B if per_b else None)
    return PQ.refine_frame(ref, cur, B, _searched(w, h, tile, B, S, lam, seed, per_b), lam, None, cost)


def _pred(kind, w, h, B, seed=0):
    n = P.counts(w, h, B)[0]
    if kind == "null":
        return None
    rng = np.random.default_rng(300 + seed)
    if kind == "near":
        return rng.integers(-24, 25, (n, 2)).astype(np.int16)
    p = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)  # "random": the whole int16 range
    p[0::3] = (32767, -32767)
    p[1::3, 1] = 32767
    return p


def _random_fields(w, h, B, lim, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-lim, lim + 1, (n, 2)).astype(np.int16) for n in P.counts(w, h, B)]


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _fields(w, h, B, frames=1):
    """Device fields, every record a sentinel."""
    F = me.PartitionRdFields.device(w, h, B, frames)
    for t in F.mv:
        t.fill_(-777)
    for t in F.cost + F.dist + [F.mode_cost]:
        t.fill_(-1)
    for t in F.bits + [F.mode]:
        t.fill_(199)
    return F


def _in_fields(mv):
    """Device PartitionFields holding the integer grids mv (frames concatenated)."""
    import torch
    tm = [_t(np.ascontiguousarray(m)) for m in mv]
    return me.PartitionFields(tm, None, torch.zeros(1, dtype=torch.uint8, device="cuda"), None)


def _device(eng, ref, cur, B, mv, lam, pred, cost, width=None, stream=None):
    import torch
    rt = ref if isinstance(ref, torch.Tensor) else _t(ref)
    ct = cur if isinstance(cur, torch.Tensor) else _t(cur)
    h, w = rt.shape[-2], width or rt.shape[-1]
    frames = rt.shape[0] if rt.dim() == 3 else 1
    F = _fields(w, h, B, frames)
    pt = _t(pred) if pred is not None else None
    fin = _in_fields(mv)
    torch.cuda.synchronize()
    eng.partition_refine_qpel_device(rt, ct, B, cost, lam, fin, F, pt, stream=stream, width=w)
    torch.cuda.synchronize()
    eng.device_check()
    return F.numpy()


def _check(got, want, frame=0):
    n = P.counts(want.w, want.h, want.B)
    for k in range(4):
        sl = slice(frame * n[k], (frame + 1) * n[k])
        for name in ("mv", "cost", "dist", "bits"):
            np.testing.assert_array_equal(getattr(got, name)[k][sl], getattr(want, name)[k],
                                          err_msg=f"{name} {P.MODES[k]}")
    sl = slice(frame * n[0], (frame + 1) * n[0])
    np.testing.assert_array_equal(got.mode[sl], want.mode)
    np.testing.assert_array_equal(got.mode_cost[sl], want.mode_cost)


def _counts(want, mv):
    """(cells, cells that left the centre in stage 1, cells that moved again in stage 2)."""
    return (sum(len(m) for m in mv),
            sum(int((want.q1[k] != 4 * mv[k].astype(np.int64)).any(1).sum()) for k in range(4)),
            sum(int((want.q1[k] != want.mv[k]).any(1).sum()) for k in range(4)))


def _distinct(w, h, B, mv):
    """Macroblocks whose partitions hold more than one integer vector."""
    g = P.grids(w, h, B)
    n = 0
    for by in range(g[0][1]):
        for bx in range(g[0][0]):
            vs = set()
            for gi, i, j, *_ in P._partitions(B, min(B, w - bx * B), min(B, h - by * B)):
                sx, sy = PR.REP[gi]
                vs.add(tuple(mv[gi][(sy * by + j) * g[gi][0] + sx * bx + i]))
            n += len(vs) > 1
    return n


# ---- searched fields of content whose motion differs per partition.  The
# asserts on the restatement's output keep the cases from being vacuous: a
# kernel that ignores partitions cannot pass.
@pytest.mark.parametrize("cost,hist", [("sad", [5, 1, 2, 4]), ("satd", [5, 1, 2, 4]),
                                       ("ssd", [6, 1, 1, 4])])
def test_56x40_empty_lower_halves(engine, cost, hist):
    w, h, B, S, lam = 56, 40, 16, 4, 4
    ref, cur = _content(w, h, 8, 7, B)
    mv = _searched(w, h, 8, B, S, lam)
    want = _want_searched(w, h, 8, B, S, lam, cost)
    assert np.bincount(want.mode, minlength=4).tolist() == hist  # all four modes
    cells, s1, s2 = _counts(want, mv)
    assert cells == 88 and 2 * s1 >= cells and 10 * s2 >= cells, (s1, s2)
    assert 2 * _distinct(w, h, B, mv) >= len(want.mode)
    _check(_device(engine, ref, cur, B, mv, lam, None, cost), want)
    pred = _pred("random", w, h, B, 1)
    _check(_device(engine, ref, cur, B, mv, lam, pred, cost),
           PQ.refine_frame(ref, cur, B, mv, lam, pred, cost))


# (w, h, pitch, B, tile, S, lambda, predictor).  The content's seed: 7, and 15
# at B = 8, where seed 7 leaves SSD and SATD with two modes.
_seed = lambda B: 15 if B == 8 else 7
SHAPES = [
    (50, 38, 64, 16, 8, 3, 4, "near"),   # clipped to 2 wide and 6 high
    (17, 17, 17, 16, 8, 2, 0, "random"),  # 1 wide, 1 high
    (16, 16, 16, 16, 8, 2, 4, "null"),
    (29, 21, 29, 8, 4, 3, 2, "null"),
    (29, 21, 32, 8, 4, 3, 2, "random"),
    (72, 40, 80, 32, 8, 3, 8, "near"),
]


@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,pitch,B,tile,S,lam,kind", SHAPES)
def test_shapes(engine, w, h, pitch, B, tile, S, lam, kind, cost):
    ref, cur = _content(w, h, tile, _seed(B), None if B == 32 else B)
    mv = _searched(w, h, tile, B, S, lam, _seed(B), B != 32)
    pred = _pred(kind, w, h, B, w)
    want = _want_searched(w, h, tile, B, S, lam, cost, B != 32, _seed(B)) if pred is None else \
        PQ.refine_frame(ref, cur, B, mv, lam, pred, cost)
    rp = np.full((h, pitch), 99, np.uint8)
    cp = np.full((h, pitch), 44, np.uint8)
    rp[:, :w], cp[:, :w] = ref, cur
    _check(_device(engine, rp, cp, B, mv, lam, pred, cost, width=w), want)


def test_the_cases_exercise_the_modes():
    """On the restatement's output: at B = 8 (4-pixel tiles) at least three
    modes, at B = 32 at SSD all four, and every mode somewhere in SHAPES."""
    seen = set()
    for w, h, pitch, B, tile, S, lam, kind in SHAPES:
        for cost in PQ.COSTS:
            modes = set(_want_searched(w, h, tile, B, S, lam, cost, B != 32, _seed(B)).mode.tolist())
            if B == 8:
                assert len(modes) >= 3, (cost, modes)
            if B == 32 and cost == "ssd":
                assert len(modes) == 4, modes
            seen |= modes
    assert seen == {0, 1, 2, 3}


def test_largest_lambda_ssd_b32(engine):
    """J up to 66,585,600 + 269 * 2^23 in u32: the restatement computes in int64."""
    w, h, B = 72, 40, 32
    ref, cur = _content(w, h, 8, 7, None)
    mv = _searched(w, h, 8, B, 3, 8, 7, False)
    pred = _pred("random", w, h, B, 2)
    _check(_device(engine, ref, cur, B, mv, TOP_LAM, pred, "ssd"),
           PQ.refine_frame(ref, cur, B, mv, TOP_LAM, pred, "ssd"))
    # the largest values: SSD at its maximum, 33 bits per component (vectors at
    # +-ME_QPEL_MAX_MV against predictors at the other end of int16) on the
    # first macroblocks, random vectors on the others
    ref2 = np.zeros((h, w), np.uint8)
    cur2 = np.full((h, w), 255, np.uint8)
    mv = _random_fields(w, h, B, MAX_MV, 5)
    g = P.grids(w, h, B)
    for k in range(4):
        sx, sy = PR.REP[k]
        m = mv[k].reshape(g[k][1], g[k][0], 2)
        m[:sy, :2 * sx] = (MAX_MV, -MAX_MV)
    pred[:2] = (-32767, 32767)
    want = PQ.refine_frame(ref2, cur2, B, mv, TOP_LAM, pred, "ssd")
    assert int(want.dist[0].max()) == 32 * 32 * 255 * 255 and int(want.bits[3].max()) == 66
    # the mode decision sums four such J: J(NxN) needs all 32 bits
    assert int(PR._per_macroblock(want, want.cost)[3].max()) + 5 * TOP_LAM > 1 << 31
    _check(_device(engine, ref2, cur2, B, mv, TOP_LAM, pred, "ssd"), want)


# ---- hand-made integer fields, independent of any search
@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,lim", [(56, 40, 16, 6), (56, 40, 16, 40), (56, 40, 16, MAX_MV),
                                       (29, 21, 8, 6), (72, 40, 32, 6), (50, 38, 16, 6)])
def test_hand_made_fields(engine, w, h, B, lim, cost):
    ref, cur = _content(w, h, B // 2, 11, B)
    mv = _random_fields(w, h, B, lim, lim + B)
    pred = _pred("near", w, h, B, 3)
    _check(_device(engine, ref, cur, B, mv, 4, pred, cost),
           PQ.refine_frame(ref, cur, B, mv, 4, pred, cost))


@pytest.mark.parametrize("cost", PQ.COSTS)
def test_constant_planes_tie_everywhere(engine, cost):
    w, h, B = 50, 38, 16
    ref = np.full((h, w), 90, np.uint8)
    cur = np.full((h, w), 97, np.uint8)
    mv = _random_fields(w, h, B, 6, 2)
    got = _device(engine, ref, cur, B, mv, 0, None, cost)
    for k in range(4):
        np.testing.assert_array_equal(got.mv[k], 4 * mv[k])  # every vector is its centre
    assert not got.mode.any()
    _check(got, PQ.refine_frame(ref, cur, B, mv, 0, None, cost))


# ---- batching: two frames of different content, frame strides above a frame,
# a caller's stream, per-frame predictors
@pytest.mark.parametrize("cost", ["sad", "satd"])
def test_batch_on_a_stream(engine, cost):
    import torch
    w, h, B, S, lam = 56, 40, 16, 4, 4
    pairs = [_content(w, h, 8, 7 + f, B) for f in range(2)]
    mvs = [_searched(w, h, 8, B, S, lam, 7 + f) for f in range(2)]
    preds = [_pred(k, w, h, B, f) for f, k in enumerate(("near", "random"))]
    rt = torch.full((2, h + 3, w), 17, dtype=torch.uint8, device="cuda")
    ct = torch.full((2, h + 5, w), 29, dtype=torch.uint8, device="cuda")
    for f, (r, c) in enumerate(pairs):
        rt[f, :h] = _t(r)
        ct[f, :h] = _t(c)
    st = torch.cuda.Stream()
    mv = [np.concatenate([mvs[0][k], mvs[1][k]]) for k in range(4)]
    got = _device(engine, rt[:, :h], ct[:, :h], B, mv, lam, np.concatenate(preds), cost,
                  stream=ctypes.c_void_p(st.cuda_stream))
    for f in range(2):
        _check(got, PQ.refine_frame(*pairs[f], B, mvs[f], lam, preds[f], cost), frame=f)


# ---- identities on the device, against the library's own block refinement
@pytest.mark.parametrize("cost", PQ.COSTS)
@pytest.mark.parametrize("w,h,B,tile", [(56, 40, 16, 8), (50, 38, 16, 8), (29, 21, 8, 4), (72, 40, 32, 8)])
def test_q1_q2_against_refine_qpel_rd(engine, w, h, B, tile, cost):
    import torch
    ref, cur = _content(w, h, tile, 7, B)
    mv = _random_fields(w, h, B, 5, 9)
    pred = _pred("near", w, h, B, 4)
    rt, ct = _t(ref), _t(cur)
    got = _device(engine, rt, ct, B, mv, 4, pred, cost)
    for k, blk in ((0, B), (3, B // 2)):
        p = PQ.cell_pred(pred, w, h, B, k).astype(np.int16)
        q_t = torch.zeros((len(mv[k]), 2), dtype=torch.int16, device="cuda")
        j_t = torch.zeros(len(mv[k]), dtype=torch.int32, device="cuda")
        d_t = torch.zeros(len(mv[k]), dtype=torch.int32, device="cuda")
        engine.refine_qpel_rd_device(rt, ct, blk, cost, 4, _t(mv[k]), q_t, j_t, d_t, _t(p))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.mv[k], q_t.cpu().numpy())
        np.testing.assert_array_equal(got.cost[k], j_t.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(got.dist[k], d_t.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("w,h,B,tile,lam", [(56, 40, 16, 8, 4), (50, 38, 16, 8, 16), (72, 40, 32, 8, 8)])
def test_q5_leaf_field_and_compensation(engine, w, h, B, tile, lam):
    import torch
    ref, cur = _content(w, h, tile, 7, B)
    mv = _searched(w, h, tile, B, 4, lam)
    rt, ct = _t(ref), _t(cur)
    F = _fields(w, h, B)
    engine.partition_refine_qpel_device(rt, ct, B, "sad", lam, _in_fields(mv), F)
    leaf_t = torch.full((P.counts(w, h, B)[3], 2), -555, dtype=torch.int16, device="cuda")
    engine.partition_leaf_field_device(w, h, B, F, leaf_t)
    torch.cuda.synchronize()
    got, leaf = F.numpy(), leaf_t.cpu().numpy()
    want = PQ.refine_frame(ref, cur, B, mv, lam, None, "sad")
    _check(got, want)
    np.testing.assert_array_equal(leaf, P.leaf_field(want))
    out5, _ = engine.compensate_planes_qpel(ref, cur, B // 2, leaf)
    assert int(out5[4 * h:].astype(np.int64).sum()) == PQ.summary(want)[2]


# ---- plumbing
def test_in_place(engine):
    import torch
    w, h, B, lam = 56, 40, 16, 4
    ref, cur = _content(w, h, 8, 7, B)
    mv = _searched(w, h, 8, B, 4, lam)
    F = _fields(w, h, B)
    for t, m in zip(F.mv, mv):
        t.copy_(_t(m))
    engine.partition_refine_qpel_device(_t(ref), _t(cur), B, "satd", lam, F, F)
    torch.cuda.synchronize()
    _check(F.numpy(), PQ.refine_frame(ref, cur, B, mv, lam, None, "satd"))


def test_null_optional_arrays(engine):
    import torch
    w, h, B, lam = 56, 40, 16, 4
    ref, cur = _content(w, h, 8, 7, B)
    mv = _searched(w, h, 8, B, 4, lam)
    F = me.PartitionRdFields.device(w, h, B)
    F.cost, F.mode_cost, F.dist, F.bits = None, None, None, None
    engine.partition_refine_qpel_device(_t(ref), _t(cur), B, "sad", lam, _in_fields(mv), F)
    torch.cuda.synchronize()
    want = PQ.refine_frame(ref, cur, B, mv, lam, None, "sad")
    got = F.numpy()
    for k in range(4):
        np.testing.assert_array_equal(got.mv[k], want.mv[k])
    np.testing.assert_array_equal(got.mode, want.mode)


def test_captured_without_warm_up():
    """Search, refinement and leaf field in one graph (a linear chain) on a
    fresh context, replayed on new contents."""
    import torch
    w, h, B, S, lam = 56, 40, 16, 4, 4
    ref0, cur0 = _content(w, h, 8, 8, B)
    ref1, cur1 = _content(w, h, 8, 7, B)
    st = torch.cuda.Stream()
    sh = ctypes.c_void_p(st.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(st):
        rt, ct = _t(ref0), _t(cur0)
        F = _fields(w, h, B)
        leaf_t = torch.zeros((P.counts(w, h, B)[3], 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: (
            eng.partition_rd_search_device(rt, ct, B, S, lam, F, stream=sh),
            eng.partition_refine_qpel_device(rt, ct, B, "satd", lam, F, F, stream=sh),
            eng.partition_leaf_field_device(w, h, B, F, leaf_t, stream=sh)))
        rt.copy_(_t(ref1))
        ct.copy_(_t(cur1))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        want = PQ.refine_frame(ref1, cur1, B, _searched(w, h, 8, B, S, lam), lam, None, "satd")
        _check(F.numpy(), want)
        np.testing.assert_array_equal(leaf_t.cpu().numpy(), P.leaf_field(want))


@pytest.mark.parametrize("cost", ["sad", "satd"])
@pytest.mark.parametrize("w,h,pitch,B,tile,S", [(56, 40, 56, 16, 8, 4), (50, 38, 64, 16, 8, 3),
                                                (72, 40, 72, 32, 8, 3)])
def test_composite_equals_the_steps_by_hand(engine, w, h, pitch, B, tile, S, cost):
    import torch
    lam = 4
    ref, cur = _content(w, h, tile, 7, B)
    rp = np.full((h, pitch), 99, np.uint8)
    cp = np.full((h, pitch), 44, np.uint8)
    rp[:, :w], cp[:, :w] = ref, cur
    pred = _pred("near", w, h, B, 6)
    got, leaf = engine.partition_search_qpel(rp, cp, B, S, lam, pred, cost, width=w)
    # by hand on the device
    rt, ct, pt = _t(rp), _t(cp), _t(pred)
    F = _fields(w, h, B)
    engine.partition_rd_search_device(rt, ct, B, S, lam, F, pt, width=w)
    engine.partition_refine_qpel_device(rt, ct, B, cost, lam, F, F, pt, width=w)
    leaf_t = torch.zeros((P.counts(w, h, B)[3], 2), dtype=torch.int16, device="cuda")
    engine.partition_leaf_field_device(w, h, B, F, leaf_t)
    torch.cuda.synchronize()
    hand = F.numpy()
    want = PQ.refine_frame(ref, cur, B, PR.search_frame(ref, cur, B, S, lam, pred).mv, lam, pred, cost)
    _check(hand, want)
    _check(got, want)
    np.testing.assert_array_equal(leaf, leaf_t.cpu().numpy())
    np.testing.assert_array_equal(leaf, P.leaf_field(want))
    none, no_leaf = engine.partition_search_qpel(rp, cp, B, S, lam, None, cost, width=w, leaf=False)
    assert no_leaf is None
    _check(none, PQ.refine_frame(ref, cur, B, PR.search_frame(ref, cur, B, S, lam).mv, lam, None, cost))


@pytest.mark.parametrize("w,h,pitch,B,tile", [(56, 40, 56, 16, 8), (50, 38, 64, 16, 8),
                                              (29, 21, 29, 8, 4), (72, 40, 80, 32, 8)])
def test_host_entry_point(engine, w, h, pitch, B, tile):
    ref, cur = _content(w, h, tile, 7, B)
    rp = np.full((h, pitch), 99, np.uint8)
    cp = np.full((h, pitch), 44, np.uint8)
    rp[:, :w], cp[:, :w] = ref, cur
    mv = _random_fields(w, h, B, 5, 4)
    fin = me.PartitionFields(mv, None, np.zeros(1, np.uint8), None)
    for kind, cost in (("null", "sad"), ("near", "ssd"), ("random", "satd")):
        pred = _pred(kind, w, h, B, 7)
        want = PQ.refine_frame(ref, cur, B, mv, 4, pred, cost)
        _check(engine.partition_refine_qpel(rp, cp, B, fin, 4, pred, cost, width=w), want)
        _check(_device(engine, rp, cp, B, mv, 4, pred, cost, width=w), want)


# ---- refusals
@pytest.mark.parametrize("kw,status", [
    (dict(lam=TOP_LAM + 1), _lib.ME_EINVAL),
    (dict(lam=1 << 24), _lib.ME_EINVAL),
    (dict(blk=12), _lib.ME_EUNSUPPORTED),
    (dict(blk=4), _lib.ME_EUNSUPPORTED),
    (dict(blk=64), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssim"), _lib.ME_EUNSUPPORTED),
])
def test_rejected_arguments(engine, kw, status):
    w, h = 56, 40
    ref, cur = _content(w, h, 8, 7, 16)
    a = dict(blk=16, lam=4, cost="sad")
    a.update(kw)
    ok = a["blk"] in (8, 16, 32)
    counts = P.counts(w, h, a["blk"] if ok else 16)
    mv = [np.zeros((n, 2), np.int16) for n in counts]
    rt, ct = _t(ref), _t(cur)
    F = me.PartitionRdFields.device(w, h, a["blk"] if ok else 16)
    with pytest.raises(me.MEError) as e:
        engine.partition_refine_qpel_device(rt, ct, a["blk"], a["cost"], a["lam"], _in_fields(mv), F)
    assert e.value.status == status
    # the host call through the C ABI (the Engine method sizes its arrays by the block size)
    fin, fout = me.PartitionFields(mv, None, np.zeros(1, np.uint8), None), me.PartitionRdFields.host(w, h, 16)
    sin, sout = fin.struct(), fout.rd_struct()
    p8 = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert _lib.lib().me_partition_refine_qpel(
        engine._h, p8(ref), p8(cur), w, h, w, a["blk"], me.engine.cost_code(a["cost"]), a["lam"], None,
        ctypes.byref(sin), ctypes.byref(sout)) == status


def test_rejected_vectors_nulls_frames_and_stripe_context(engine):
    w, h, B = 56, 40, 16
    ref, cur = _content(w, h, 8, 7, B)
    rt, ct = _t(ref), _t(cur)
    # a component beyond ME_QPEL_MAX_MV in any of the four grids (host call)
    for k in range(4):
        mv = [np.zeros((n, 2), np.int16) for n in P.counts(w, h, B)]
        mv[k][-1, 1] = -(MAX_MV + 1)
        with pytest.raises(me.MEError) as e:
            engine.partition_refine_qpel(ref, cur, B, me.PartitionFields(mv, None, np.zeros(1, np.uint8), None))
        assert e.value.status == _lib.ME_EINVAL
        mv[k][-1, 1] = -MAX_MV
        engine.partition_refine_qpel(ref, cur, B, me.PartitionFields(mv, None, np.zeros(1, np.uint8), None))
    mv = [np.zeros((n, 2), np.int16) for n in P.counts(w, h, B)]
    fin, F = _in_fields(mv), me.PartitionRdFields.device(w, h, B)
    fn = _lib.lib().me_partition_refine_qpel_device

    def call(si, so, ref_p=rt.data_ptr(), frames=1, rfs=0, pitch=w):
        return fn(engine._h, ref_p, rfs, ct.data_ptr(), 0, w, h, pitch, B, _lib.ME_COST_SAD, 4, frames,
                  None, si, so, None)
    si, so = fin.struct(), F.rd_struct()
    so.f.mv_nx2n = None
    assert call(ctypes.byref(si), ctypes.byref(so)) == _lib.ME_EINVAL   # a required output
    so = F.rd_struct()
    so.f.mode = None
    assert call(ctypes.byref(si), ctypes.byref(so)) == _lib.ME_EINVAL
    so = F.rd_struct()
    si.mv_2nxn = None
    assert call(ctypes.byref(si), ctypes.byref(so)) == _lib.ME_EINVAL   # a required input
    si = fin.struct()
    assert call(None, ctypes.byref(so)) == _lib.ME_EINVAL
    assert call(ctypes.byref(si), None) == _lib.ME_EINVAL
    assert call(ctypes.byref(si), ctypes.byref(so), ref_p=None) == _lib.ME_EINVAL
    assert call(ctypes.byref(si), ctypes.byref(so), frames=0) == _lib.ME_EINVAL
    assert call(ctypes.byref(si), ctypes.byref(so), frames=2, rfs=w) == _lib.ME_EINVAL  # overlapping frames
    assert call(ctypes.byref(si), ctypes.byref(so), pitch=w - 1) == _lib.ME_EINVAL
    assert call(ctypes.byref(si), ctypes.byref(so), pitch=(1 << 31) // h + 1) == _lib.ME_EUNSUPPORTED
    assert call(ctypes.byref(si), ctypes.byref(so)) == _lib.ME_OK
    # the composite call: SAD and SATD only, with me_full_search_rd_qpel's statuses
    for cost in ("ssd", "ssim"):
        with pytest.raises(me.MEError) as e:
            engine.partition_search_qpel(ref, cur, B, 4, 4, None, cost)
        assert e.value.status == _lib.ME_EUNSUPPORTED
    with pytest.raises(me.MEError) as e:
        engine.partition_search_qpel(ref, cur, B, 4, TOP_LAM + 1)
    assert e.value.status == _lib.ME_EINVAL
    # a context over repeated device ids works in stripes: not offered
    with me.Engine(devices=[0, 0]) as two:
        with pytest.raises(me.MEError) as e:
            two.partition_refine_qpel(ref, cur, B, me.PartitionFields(mv, None, np.zeros(1, np.uint8), None))
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.partition_refine_qpel_device(rt, ct, B, "sad", 4, fin, F)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.partition_search_qpel(ref, cur, B, 4, 4)
        assert e.value.status == _lib.ME_EUNSUPPORTED
