"""Rate-constrained partition search on the GPU against
tests/partition_rd_ref.py, record for record (assert_array_equal on every
vector, J, distortion, rate, mode and mode cost of every grid): the fast
kernel's shapes with and without a generic rim, clipped and generic shapes, row
pitches, every predictor kind, lambda over both kernels' ranges, the tie rule,
saturation, identities E1, E2 and E5 on device outputs, batches on a caller's
stream, NULL optional arrays, a captured launch, the host entry point, rejected
arguments and the Foreman table of DESIGN.md.
me_partition_rd_kernel_variant names the kernel; tests/test_partition_rd_ref.py
pins it per shape."""
import ctypes
import functools

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_rd_ref as Q
import partition_ref as P
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

FAST, GENERIC = _lib.ME_PART_KERNEL_FAST, _lib.ME_PART_KERNEL_GENERIC
FAST_LAM = _lib.ME_RD_FAST_MAX_LAMBDA
TOP_LAM = _lib.ME_PART_RD_MAX_LAMBDA
SHIFT = (2, -3)
CORNERS = [(-32768, -32768), (32767, -32768), (-32768, 32767), (32767, 32767)]


def _noise(w, h, seed, shift=SHIFT):
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    big = ((big.astype(np.uint16) + np.roll(big, 1, 0) + np.roll(big, 1, 1) +
            np.roll(big, (1, 1), (0, 1))) // 4).astype(np.uint8)
    ref = big[8:8 + h, 8:8 + w]
    cur = big[8 + shift[1]:8 + shift[1] + h, 8 + shift[0]:8 + shift[0] + w]
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


@functools.lru_cache(maxsize=None)
def _case(w, h, seed):
    ref, cur = _noise(w, h, seed)
    ref.setflags(write=False)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def _table(w, h, seed, B, S):
    """The quadrant SADs of a case: one table serves every lambda and predictor."""
    return Q.quad_table(*_case(w, h, seed), B, S)


def _pred(kind, w, h, B, seed=0):
    """int16 [macroblocks, 2] quarter-pel predictors, or None."""
    n = P.counts(w, h, B)[0]
    if kind == "null":
        return None
    if kind == "zeros":
        return np.zeros((n, 2), np.int16)
    if kind == "random":  # the whole int16 range
        return np.random.default_rng(100 + seed).integers(-32768, 32768, (n, 2)).astype(np.int16)
    if kind == "corners":
        return np.array([CORNERS[i % 4] for i in range(n)], np.int16)
    if kind == "shift":  # 4 x the true displacement of _noise
        return np.tile(np.int16([4 * SHIFT[0], 4 * SHIFT[1]]), (n, 1))
    if kind == "near":  # a few quarter-pels around the true displacement
        return (np.random.default_rng(200 + seed).integers(-24, 25, (n, 2)) +
                [4 * SHIFT[0], 4 * SHIFT[1]]).astype(np.int16)
    raise ValueError(kind)


def _want(w, h, seed, B, S, lam, pred):
    return Q.search_frame(*_case(w, h, seed), B, S, lam, pred, _table(w, h, seed, B, S))


def _t(a):
    """A device copy of a (possibly read-only) numpy array."""
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


def _device(eng, ref, cur, B, S, lam, pred=None, width=None, stream=None, cost="sad"):
    """Search (H, pitch) planes or [F, H, pitch] batches (numpy or torch) on
    the device.  Returns numpy fields."""
    import torch
    rt = ref if isinstance(ref, torch.Tensor) else _t(ref)
    ct = cur if isinstance(cur, torch.Tensor) else _t(cur)
    h, w = rt.shape[-2], width or rt.shape[-1]
    frames = rt.shape[0] if rt.dim() == 3 else 1
    F = _fields(w, h, B, frames)
    pt = _t(pred) if pred is not None else None
    torch.cuda.synchronize()
    eng.partition_rd_search_device(rt, ct, B, S, lam, F, pt, cost=cost, width=w, stream=stream)
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


def _summary(got, w, h, B, lam):
    """partition_rd_ref.summary of one frame's device records."""
    F = Q.Fields(w, h, B)
    F.mv, F.cost, F.dist, F.bits = got.mv, got.cost, got.dist, got.bits
    F.mode, F.mode_cost = got.mode, got.mode_cost
    return Q.summary(F, lam)


def _run(eng, w, h, seed, B, S, lam, kind):
    ref, cur = _case(w, h, seed)
    pred = _pred(kind, w, h, B, seed)
    _check(_device(eng, ref, cur, B, S, lam, pred), _want(w, h, seed, B, S, lam, pred))


# (predictor kind, lambda): every predictor kind and every lambda of the list
# {0, 1, 16, FAST_LAM, FAST_LAM + 1, TOP_LAM} at least once
ALL = [("null", 16), ("zeros", 1), ("random", 0), ("random", 16), ("corners", FAST_LAM),
       ("shift", 16), ("near", FAST_LAM + 1), ("corners", TOP_LAM), ("near", 64)]
FEW = [("null", 16), ("near", 1), ("corners", FAST_LAM), ("random", FAST_LAM + 1)]


def _variant(w, h, pitch, B, S, lam, fast_ok=True):
    """The kernel a (shape, lambda) must report: FAST up to FAST_LAM on a fast
    shape, GENERIC above it and on a generic shape."""
    want = FAST if fast_ok and lam <= FAST_LAM else GENERIC
    assert me.partition_rd_kernel_variant(w, h, pitch, B, S, lam) == want, (w, h, B, S, lam)


# ---- the fast kernel: every macroblock of 96x64 has a clamped window at S =
# 16, every macroblock of 80x48 at S = 64 on both axes
@pytest.mark.parametrize("w,h,S,combos", [(96, 64, 7, ALL), (96, 64, 16, ALL),
                                           (256, 144, 32, FEW), (80, 48, 64, FEW)])
def test_fast_path(engine, w, h, S, combos):
    for kind, lam in combos:
        _variant(w, h, w, 16, S, lam)
        _run(engine, w, h, 3, 16, S, lam, kind)


def test_fast_path_with_generic_rim(engine):
    """Full-size macroblocks on the fast kernel, the right column (4 wide) and
    the bottom row (8 high) on the generic one, in one call."""
    for kind, lam in ALL:
        _variant(100, 72, 100, 16, 7, lam)
        _run(engine, 100, 72, 4, 16, 7, lam, kind)


# ---- clipped and generic shapes: frames below a macroblock, remainders <= h
# and > h, B = 8 and B = 32
@pytest.mark.parametrize("w,h,B", [(9, 9, 16), (33, 17, 16), (44, 28, 16), (40, 24, 8),
                                    (70, 40, 32)])
def test_clipped_and_generic_shapes(engine, w, h, B):
    for kind, lam in ALL:
        _run(engine, w, h, 1, B, 5, lam, kind)


# ---- row pitch: rows of 112 bytes (fast kernel) and unaligned pitches (generic)
@pytest.mark.parametrize("w,pitch,fast", [(100, 112, True), (96, 99, False), (96, 110, False)])
def test_row_pitch(engine, w, pitch, fast):
    ref, cur = _case(w, 64, 5)
    planes = []
    for a in (ref, cur):
        p = np.full((64, pitch), 201, np.uint8)  # the padding must not be read as pixels
        p[:, :w] = a
        planes.append(_t(p))
    for kind, lam in FEW:
        _variant(w, 64, pitch, 16, 7, lam, fast)
        pred = _pred(kind, w, 64, 16, 5)
        _check(_device(engine, planes[0], planes[1], 16, 7, lam, pred, width=w),
               _want(w, 64, 5, 16, 7, lam, pred))


# ---- ties: every SAD ties on flat and checkerboard frames, so the rate decides,
# and bits(v) = bits(-v) leaves ties that go to the first raster candidate
def _board(w, h, period):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // period) + (y // period)) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (44, 28, 16, 5), (70, 40, 32, 3)])
@pytest.mark.parametrize("pattern", ["flat", "board1", "board3"])
def test_ties_go_to_the_first_raster_candidate(engine, w, h, B, S, pattern):
    if pattern == "flat":
        ref = cur = np.full((h, w), 93, np.uint8)
    else:
        ref = _board(w, h, int(pattern[-1]))
        cur = np.roll(ref, 1, axis=1)
    tab = Q.quad_table(ref, cur, B, S)
    n = P.counts(w, h, B)[0]
    # zero, and off-centre predictors half way between two displacements:
    # |4 d - 10| = 2 at d = 2 and 3, |4 d + 6| = 2 at d = -2 and -1
    for p in (None, (0, 0), (10, -6), (-6, 10)):
        pred = None if p is None else np.tile(np.int16(p), (n, 1))
        for lam in (1, 16):
            want = Q.search_frame(ref, cur, B, S, lam, pred, tab)
            if pattern == "flat":
                assert (want.dist[0] == 0).all()
                if p == (10, -6) and (w, h, B, S) == (96, 64, 16, 7):
                    # macroblock (1, 1) has the whole window: the first of each pair
                    assert tuple(want.mv[0][7]) == (2, -2)
            _check(_device(engine, ref, cur, B, S, lam, pred), want)


# ---- saturation: 0 / 255 planes at the top lambda of each kernel; macroblock
# 0's predictor (-32768, -32768) and its window (d >= 0) give R = 66
@pytest.mark.parametrize("w,h,B,top,lam,variant", [
    (64, 48, 16, 65280, FAST_LAM, FAST), (64, 48, 16, 65280, TOP_LAM, GENERIC),
    (70, 40, 32, 261120, TOP_LAM, GENERIC)])
def test_saturation(engine, w, h, B, top, lam, variant):
    assert me.partition_rd_kernel_variant(w, h, w, B, 4, lam) == variant
    ref, cur = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    pred = _pred("corners", w, h, B)
    want = Q.search_frame(ref, cur, B, 4, lam, pred)
    assert want.dist[0][0] == top and want.bits[0][0] == 66
    assert want.cost[0][0] == top + 66 * lam
    _check(_device(engine, ref, cur, B, 4, lam, pred), want)


# ---- E1: lambda = 0 is partition_search_device at lambda = 0, whatever the predictor
@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (100, 72, 16, 7), (70, 40, 32, 5)])
def test_e1_against_the_partition_search(engine, w, h, B, S):
    import torch
    ref, cur = _case(w, h, 6)
    got = _device(engine, ref, cur, B, S, 0, _pred("random", w, h, B, 6))
    G = me.PartitionFields.device(w, h, B)
    engine.partition_search_device(_t(ref), _t(cur), B, S, 0, G)
    torch.cuda.synchronize()
    G = G.numpy()
    for k in range(4):
        np.testing.assert_array_equal(got.mv[k], G.mv[k])
        np.testing.assert_array_equal(got.cost[k], G.cost[k])
        np.testing.assert_array_equal(got.dist[k], got.cost[k])
    np.testing.assert_array_equal(got.mode, G.mode)
    np.testing.assert_array_equal(got.mode_cost, G.mode_cost)


# ---- E2: the 2Nx2N records are rd_search_device's at (B, S, lambda, predictor)
@pytest.mark.parametrize("w,h,B,S,lam", [(96, 64, 16, 7, 16), (100, 72, 16, 7, FAST_LAM),
                                          (96, 64, 16, 16, FAST_LAM + 1), (40, 24, 8, 5, 16),
                                          (70, 40, 32, 5, TOP_LAM)])
def test_e2_against_the_rd_search(engine, w, h, B, S, lam):
    import torch
    ref, cur = _case(w, h, 7)
    pred = _pred("near", w, h, B, 7)
    got = _device(engine, ref, cur, B, S, lam, pred)
    n = P.counts(w, h, B)[0]
    mv = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
    J, D = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    Rb = torch.zeros(n, dtype=torch.uint8, device="cuda")
    engine.rd_search_device(_t(ref), _t(cur), B, S, lam, mv, J, D, Rb, _t(pred))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.mv[0], mv.cpu().numpy())
    np.testing.assert_array_equal(got.cost[0], J.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got.dist[0], D.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got.bits[0], Rb.cpu().numpy())


# ---- E5: the leaf field compensated at B / 2 reproduces the chosen distortion
@pytest.mark.parametrize("w,h,B,lam", [(96, 64, 16, 16), (100, 72, 16, 4), (70, 40, 32, 64)])
def test_e5_leaf_field_and_compensation(engine, w, h, B, lam):
    import torch
    ref, cur = _case(w, h, 8)
    pred = _pred("near", w, h, B, 8)
    F = _fields(w, h, B)
    engine.partition_rd_search_device(_t(ref), _t(cur), B, 5, lam, F, _t(pred))
    leaf_t = torch.full((me.partition_counts(w, h, B)[3], 2), -555, dtype=torch.int16,
                        device="cuda")
    engine.partition_leaf_field_device(w, h, B, F, leaf_t)
    torch.cuda.synchronize()
    got, leaf = F.numpy(), leaf_t.cpu().numpy()
    want = _want(w, h, 8, B, 5, lam, pred)
    _check(got, want)
    np.testing.assert_array_equal(leaf, P.leaf_field(want))
    np.testing.assert_array_equal(leaf, me.partition_leaf_field(w, h, B, got))
    out5, _ = engine.compensate_planes(ref, cur, B // 2, leaf)
    sad = int(out5[4 * h:].astype(np.int64).sum())
    hist, sum_j, sum_d, sum_b = _summary(got, w, h, B, lam)
    assert sad == sum_d == sum_j - lam * (sum_b + int(np.dot(hist, Q.MBITS)))


# ---- batching: three frames, frame strides above a frame, a caller's stream,
# per-frame predictors
@pytest.mark.parametrize("w,h,S", [(96, 64, 7), (44, 28, 5)])
def test_batch_on_a_stream(engine, w, h, S):
    import torch
    pairs = [_case(w, h, 10 + f) for f in range(3)]
    preds = [_pred(k, w, h, 16, 10 + f) for f, k in enumerate(("near", "random", "corners"))]
    rt = torch.full((3, h + 3, w), 17, dtype=torch.uint8, device="cuda")
    ct = torch.full((3, h + 5, w), 29, dtype=torch.uint8, device="cuda")
    for f, (r, c) in enumerate(pairs):
        rt[f, :h] = _t(r)
        ct[f, :h] = _t(c)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    got = _device(engine, rt[:, :h], ct[:, :h], 16, S, 16, np.concatenate(preds),
                  stream=ctypes.c_void_p(st.cuda_stream))
    for f in range(3):
        _check(got, _want(w, h, 10 + f, 16, S, 16, preds[f]), frame=f)


def test_null_optional_arrays(engine):
    import torch
    ref, cur = _case(96, 64, 3)
    pred = _pred("near", 96, 64, 16, 3)
    F = me.PartitionRdFields.device(96, 64, 16)
    F.cost, F.mode_cost, F.dist, F.bits = None, None, None, None
    engine.partition_rd_search_device(_t(ref), _t(cur), 16, 7, 16, F, _t(pred))
    torch.cuda.synchronize()
    want = _want(96, 64, 3, 16, 7, 16, pred)
    got = F.numpy()
    for k in range(4):
        np.testing.assert_array_equal(got.mv[k], want.mv[k])
    np.testing.assert_array_equal(got.mode, want.mode)


# ---- captured step: no context scratch, so no warm-up call before capture
def test_captured_search_and_leaf_field():
    """Search (fast kernel, then the rim on the generic one) and leaf field in
    one graph (a linear chain) on a fresh context, replayed on new contents."""
    import torch
    w, h = 100, 72
    ref0, cur0 = _case(w, h, 20)
    ref1, cur1 = _case(w, h, 21)
    pred = _pred("near", w, h, 16, 21)
    st = torch.cuda.Stream()
    sh = ctypes.c_void_p(st.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(st):
        rt, ct, pt = _t(ref0), _t(cur0), _t(np.zeros_like(pred))
        F = _fields(w, h, 16)
        leaf_t = torch.zeros((me.partition_counts(w, h, 16)[3], 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: (
            eng.partition_rd_search_device(rt, ct, 16, 7, 16, F, pt, stream=sh),
            eng.partition_leaf_field_device(w, h, 16, F, leaf_t, stream=sh)))
        rt.copy_(_t(ref1))
        ct.copy_(_t(cur1))
        pt.copy_(_t(pred))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        want = _want(w, h, 21, 16, 7, 16, pred)
        _check(F.numpy(), want)
        np.testing.assert_array_equal(leaf_t.cpu().numpy(), P.leaf_field(want))


# ---- host planes: the synchronous entry point equals the restatement
@pytest.mark.parametrize("w,h,B,S,width", [(96, 64, 16, 7, None), (44, 28, 16, 5, None),
                                            (70, 40, 32, 5, None), (112, 64, 16, 7, 100)])
def test_host_entry_point(engine, w, h, B, S, width):
    ref, cur = _case(w, h, 7)
    fw = width or w
    for kind in ("null", "near"):
        pred = _pred(kind, fw, h, B, 7)
        want = Q.search_frame(ref[:, :fw], cur[:, :fw], B, S, 16, pred)
        _check(engine.partition_rd_search(ref, cur, B, S, 16, pred, width=width), want)
        _check(_device(engine, ref, cur, B, S, 16, pred, width=width), want)


# ---- rejected arguments
@pytest.mark.parametrize("kw,status", [
    (dict(lam=TOP_LAM + 1), _lib.ME_EINVAL),
    (dict(lam=1 << 24), _lib.ME_EINVAL),
    (dict(blk=12), _lib.ME_EUNSUPPORTED),
    (dict(span=129), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssd"), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssim"), _lib.ME_EUNSUPPORTED),
    (dict(span=-1), _lib.ME_EINVAL),
])
def test_rejected_arguments(engine, kw, status):
    ref, cur = _case(96, 64, 3)
    a = dict(blk=16, span=7, lam=16, cost="sad")
    a.update(kw)
    with pytest.raises(me.MEError) as e:
        engine.partition_rd_search(ref, cur, a["blk"], a["span"], a["lam"], None, a["cost"])
    assert e.value.status == status
    rt, ct = _t(ref), _t(cur)
    F = me.PartitionRdFields.device(96, 64, a["blk"])
    with pytest.raises(me.MEError) as e:
        engine.partition_rd_search_device(rt, ct, a["blk"], a["span"], a["lam"], F,
                                          cost=a["cost"])
    assert e.value.status == status


def test_rejected_nulls_frames_and_stripe_context(engine):
    ref, cur = _case(96, 64, 3)
    rt, ct = _t(ref), _t(cur)
    F = me.PartitionRdFields.device(96, 64, 16)
    fn = _lib.lib().me_partition_rd_search_device

    def call(st, ref_p=rt.data_ptr(), frames=1, rfs=0):
        return fn(engine._h, ref_p, rfs, ct.data_ptr(), 0, 96, 64, 96, 16, 7, _lib.ME_COST_SAD,
                  16, frames, None, st, None)
    st = F.rd_struct()
    st.f.mv_2nxn = None
    assert call(ctypes.byref(st)) == _lib.ME_EINVAL      # a required field
    st = F.rd_struct()
    st.f.mode = None
    assert call(ctypes.byref(st)) == _lib.ME_EINVAL
    st = F.rd_struct()
    assert call(None) == _lib.ME_EINVAL                  # no field struct
    assert call(ctypes.byref(st), ref_p=None) == _lib.ME_EINVAL
    assert call(ctypes.byref(st), frames=0) == _lib.ME_EINVAL
    assert call(ctypes.byref(st), frames=2, rfs=96) == _lib.ME_EINVAL  # overlapping frames
    # a context over repeated device ids searches in stripes: not offered
    with me.Engine(devices=[0, 0]) as two:
        with pytest.raises(me.MEError) as e:
            two.partition_rd_search(ref, cur, 16, 7, 16)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.partition_rd_search_device(rt, ct, 16, 7, 16, F)
        assert e.value.status == _lib.ME_EUNSUPPORTED


# ---- Foreman 1 -> 2, 16x16, +-7, zero predictor: the table of DESIGN.md
# "Rate-constrained partition search" (tests/test_partition_rd_ref.py computes
# it from the restatement)
def test_foreman_table(engine):
    from test_partition_rd_ref import FOREMAN
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    assert me.partition_rd_kernel_variant(352, 288, 352, 16, 7, 256) == FAST
    tab = Q.quad_table(ref, cur, 16, 7)
    rt, ct = _t(ref), _t(cur)
    for lam, hist, sum_j, sum_d, sum_b, d0, b0 in FOREMAN:
        got = _device(engine, rt, ct, 16, 7, lam)
        _check(got, Q.search_frame(ref, cur, 16, 7, lam, None, tab))
        assert _summary(got, 352, 288, 16, lam) == (hist, sum_j, sum_d, sum_b)
        assert int(got.dist[0].astype(np.int64).sum()) == d0
        assert int(got.bits[0].astype(np.int64).sum()) == b0
