"""Partition search on the GPU against tests/partition_ref.py, record for
record (assert_array_equal throughout): clipped macroblocks, the range
envelope, the fast kernel's small shapes (me_partition_kernel_variant names the
kernel; tests/test_partition_ref.py pins it per shape), the tie rule in all
nine minima, u16 / u32 saturation, row pitches, batches on a caller's stream,
lambda's range, rejected arguments, the Foreman figures of DESIGN.md with the
leaf field compensated at B / 2, and the host entry point."""
import ctypes
import functools

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import partition_ref as P
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

FAST, GENERIC = _lib.ME_PART_KERNEL_FAST, _lib.ME_PART_KERNEL_GENERIC


def _noise(w, h, seed, shift=(2, -3)):
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
def _expected(w, h, seed, B, S):
    """The restatement's fields at lambda = 0 (decide() gives the other lambdas)."""
    ref, cur = _case(w, h, seed)
    return P.search_frame(ref, cur, B, S, 0)


def _t(a):
    """A device copy of a (possibly read-only) numpy array."""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _device(eng, ref, cur, B, S, lam, width=None, stream=None, cost="sad"):
    """Search (H, pitch) planes or [F, H, pitch] batches (numpy or torch) on
    the device; every record starts as a sentinel.  Returns numpy fields."""
    import torch
    rt = ref if isinstance(ref, torch.Tensor) else _t(ref)
    ct = cur if isinstance(cur, torch.Tensor) else _t(cur)
    h, w = rt.shape[-2], width or rt.shape[-1]
    frames = rt.shape[0] if rt.dim() == 3 else 1
    F = me.PartitionFields.device(w, h, B, frames)
    for t in F.mv:
        t.fill_(-777)
    for t in F.cost + [F.mode_cost]:
        t.fill_(-1)
    F.mode.fill_(9)
    torch.cuda.synchronize()
    eng.partition_search_device(rt, ct, B, S, lam, F, cost=cost, width=w, stream=stream)
    torch.cuda.synchronize()
    eng.device_check()
    return F.numpy()


def _check(got, want, frame=0):
    n = P.counts(want.w, want.h, want.B)
    for k in range(4):
        sl = slice(frame * n[k], (frame + 1) * n[k])
        np.testing.assert_array_equal(got.mv[k][sl], want.mv[k], err_msg=f"mv {P.MODES[k]}")
        np.testing.assert_array_equal(got.cost[k][sl], want.cost[k], err_msg=f"cost {P.MODES[k]}")
    sl = slice(frame * n[0], (frame + 1) * n[0])
    np.testing.assert_array_equal(got.mode[sl], want.mode)
    np.testing.assert_array_equal(got.mode_cost[sl], want.mode_cost)


def _run(eng, w, h, seed, B, S, lam=16):
    ref, cur = _case(w, h, seed)
    want = P.decide(_expected(w, h, seed, B, S), lam)
    _check(_device(eng, ref, cur, B, S, lam), want)


# ---- macroblock clipping: frames below a macroblock, remainders <= h and > h
@pytest.mark.parametrize("w,h,B", [(9, 9, 16), (33, 17, 16), (44, 28, 16), (40, 24, 8),
                                    (70, 40, 32)])
def test_clipped_macroblocks(engine, w, h, B):
    _run(engine, w, h, 1, B, 5)


# ---- ranges
@pytest.mark.parametrize("w,h,B,S", [(44, 28, 16, 0), (96, 64, 16, 0), (96, 64, 16, 3),
                                      (96, 64, 16, 5), (44, 28, 16, 7), (33, 17, 16, 40),
                                      (40, 24, 8, 64), (64, 64, 32, 9), (128, 96, 16, 128)])
def test_ranges(engine, w, h, B, S):
    _run(engine, w, h, 2, B, S)


# ---- the fast kernel: every macroblock of 96x64 has a clamped window at S = 16
@pytest.mark.parametrize("w,h,S", [(96, 64, 7), (96, 64, 16), (256, 144, 32), (80, 48, 64)])
def test_fast_path(engine, w, h, S):
    assert me.partition_kernel_variant(w, h, w, 16, S) == FAST
    _run(engine, w, h, 3, 16, S)


def test_fast_path_with_clipped_rim(engine):
    """Full-size macroblocks on the fast kernel, the right column (4 wide) and
    the bottom row (12 high) on the generic one, in one call."""
    assert me.partition_kernel_variant(100, 76, 100, 16, 7) == FAST
    _run(engine, 100, 76, 4, 16, 7)


# ---- tie rule: the first raster candidate wins in all nine minima
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
    want = P.search_frame(ref, cur, B, S, 16)
    if pattern == "flat":  # everything ties: the window's first displacement
        assert (want.cost[0] == 0).all()
        assert tuple(want.mv[3][0]) == (0, 0) and tuple(want.mv[0][-1]) != (0, 0)
    _check(_device(engine, ref, cur, B, S, 16), want)


# ---- saturation: 65,280 in packed u16 (B = 16), 261,120 in u32 (B = 32)
@pytest.mark.parametrize("w,h,B,top", [(64, 48, 16, 65280), (70, 40, 32, 261120)])
def test_saturation(engine, w, h, B, top):
    ref, cur = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    want = P.search_frame(ref, cur, B, 4, 16)
    assert want.cost[0][0] == top
    _check(_device(engine, ref, cur, B, 4, 16), want)


# ---- row pitch: rows of 112 bytes (fast kernel) and an unaligned pitch (generic)
@pytest.mark.parametrize("w,pitch,variant", [(100, 112, FAST), (96, 99, GENERIC), (96, 110, GENERIC)])
def test_row_pitch(engine, w, pitch, variant):
    import torch
    assert me.partition_kernel_variant(w, 64, pitch, 16, 7) == variant
    ref, cur = _case(w, 64, 5)
    planes = []
    for a in (ref, cur):
        p = np.full((64, pitch), 201, np.uint8)  # the padding must not be read as pixels
        p[:, :w] = a
        planes.append(_t(p))
    want = P.decide(_expected(w, 64, 5, 16, 7), 16)
    _check(_device(engine, planes[0], planes[1], 16, 7, 16, width=w), want)


# ---- batching: three frames, frame strides above a frame, a caller's stream
@pytest.mark.parametrize("w,h,S", [(96, 64, 7), (44, 28, 5)])
def test_batch_on_a_stream(engine, w, h, S):
    import torch
    pairs = [_case(w, h, 10 + f) for f in range(3)]
    rt = torch.full((3, h + 3, w), 17, dtype=torch.uint8, device="cuda")
    ct = torch.full((3, h + 5, w), 29, dtype=torch.uint8, device="cuda")
    for f, (r, c) in enumerate(pairs):
        rt[f, :h] = _t(r)
        ct[f, :h] = _t(c)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    got = _device(engine, rt[:, :h], ct[:, :h], 16, S, 16, stream=ctypes.c_void_p(st.cuda_stream))
    for f in range(3):
        _check(got, P.decide(_expected(w, h, 10 + f, 16, S), 16), frame=f)


# ---- lambda over its range
@pytest.mark.parametrize("lam", [0, 16, 1 << 24])
@pytest.mark.parametrize("w,h,B", [(96, 64, 16), (44, 28, 16), (70, 40, 32)])
def test_lambda(engine, w, h, B, lam):
    _run(engine, w, h, 6, B, 5, lam)


def test_null_cost_arrays(engine):
    import torch
    ref, cur = _case(96, 64, 3)
    F = me.PartitionFields.device(96, 64, 16)
    F.cost, F.mode_cost = None, None
    engine.partition_search_device(_t(ref), _t(cur), 16, 7,
                                   16, F)
    torch.cuda.synchronize()
    want = P.decide(_expected(96, 64, 3, 16, 7), 16)
    got = F.numpy()
    for k in range(4):
        np.testing.assert_array_equal(got.mv[k], want.mv[k])
    np.testing.assert_array_equal(got.mode, want.mode)


# ---- rejected arguments
@pytest.mark.parametrize("kw,status", [
    (dict(lam=(1 << 24) + 1), _lib.ME_EINVAL),
    (dict(blk=12), _lib.ME_EUNSUPPORTED),
    (dict(span=129), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssd"), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssim"), _lib.ME_EUNSUPPORTED),
    (dict(span=-1), _lib.ME_EINVAL),
])
def test_rejected_arguments(engine, kw, status):
    import torch
    ref, cur = _case(96, 64, 3)
    a = dict(blk=16, span=7, lam=16, cost="sad")
    a.update(kw)
    with pytest.raises(me.MEError) as e:
        engine.partition_search(ref, cur, a["blk"], a["span"], a["lam"], a["cost"])
    assert e.value.status == status
    rt, ct = _t(ref), _t(cur)
    F = me.PartitionFields.device(96, 64, a["blk"])
    with pytest.raises(me.MEError) as e:
        engine.partition_search_device(rt, ct, a["blk"], a["span"], a["lam"], F, cost=a["cost"])
    assert e.value.status == status


def test_rejected_null_field_and_stripe_context(engine):
    import torch
    ref, cur = _case(96, 64, 3)
    rt, ct = _t(ref), _t(cur)
    F = me.PartitionFields.device(96, 64, 16)
    st = F.struct()
    st.mv_2nxn = None
    s = _lib.lib().me_partition_search_device(engine._h, rt.data_ptr(), 0, ct.data_ptr(), 0, 96, 64,
                                              96, 16, 7, _lib.ME_COST_SAD, 16, 1, ctypes.byref(st),
                                              None)
    assert s == _lib.ME_EINVAL
    # a context over repeated device ids searches in stripes: not offered
    with me.Engine(devices=[0, 0]) as two:
        with pytest.raises(me.MEError) as e:
            two.partition_search(ref, cur, 16, 7, 16)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.partition_search_device(rt, ct, 16, 7, 16, F)
        assert e.value.status == _lib.ME_EUNSUPPORTED


# ---- Foreman 1 -> 2, 16x16, +-7: the tables of DESIGN.md "Partition search"
FOREMAN = [(0, [77, 18, 10, 291], 255385, 255385), (16, [207, 56, 48, 85], 271059, 258979),
           (64, [299, 40, 36, 21], 300737, 266497), (256, [377, 6, 12, 1], 387209, 280457),
           (100000, [396, 0, 0, 0], 39890804, 290804)]


def test_foreman_tables_and_leaf_compensation(engine):
    import torch
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    want = P.search_frame(ref, cur, 16, 7, 0)
    rt, ct = _t(ref), _t(cur)
    for lam, hist, sum_j, sum_d in FOREMAN:
        got = _device(engine, rt, ct, 16, 7, lam)
        _check(got, P.decide(want, lam))
        assert [int(c.astype(np.int64).sum()) for c in got.cost] == [290804, 275534, 274959, 255385]
        assert P.summary(got, lam) == (hist, sum_j, sum_d)
    # lambda = 16 on the device: leaf field -> the integer compensation at B / 2
    F = me.PartitionFields.device(352, 288, 16)
    engine.partition_search_device(rt, ct, 16, 7, 16, F)
    leaf_t = torch.full((me.partition_counts(352, 288, 16)[3], 2), -555, dtype=torch.int16,
                        device="cuda")
    engine.partition_leaf_field_device(352, 288, 16, F, leaf_t)
    torch.cuda.synchronize()
    leaf = leaf_t.cpu().numpy()
    np.testing.assert_array_equal(leaf, P.leaf_field(P.decide(want, 16)))
    np.testing.assert_array_equal(leaf, me.partition_leaf_field(352, 288, 16, F.numpy()))
    out5, _ = engine.compensate_planes(ref, cur, 8, leaf)
    assert int(out5[4 * 288:].astype(np.int64).sum()) == 258979


def test_leaf_field_device_batch(engine):
    import torch
    w, h = 44, 28
    refs = np.stack([_case(w, h, 10 + f)[0] for f in range(3)])
    curs = np.stack([_case(w, h, 10 + f)[1] for f in range(3)])
    F = me.PartitionFields.device(w, h, 16, 3)
    engine.partition_search_device(_t(refs), _t(curs), 16,
                                   5, 16, F)
    n3 = me.partition_counts(w, h, 16)[3]
    leaf_t = torch.full((3 * n3, 2), -555, dtype=torch.int16, device="cuda")
    engine.partition_leaf_field_device(w, h, 16, F, leaf_t, frames=3)
    torch.cuda.synchronize()
    leaf = leaf_t.cpu().numpy()
    for f in range(3):
        want = P.leaf_field(P.decide(_expected(w, h, 10 + f, 16, 5), 16))
        np.testing.assert_array_equal(leaf[f * n3:(f + 1) * n3], want)


# ---- captured step: no context scratch, so no warm-up call before capture
def test_captured_search_and_leaf_field():
    """Search (fast kernel, then the rim on the generic one) and leaf field in
    one graph (a linear chain) on a fresh context, replayed on new contents."""
    import torch
    w, h = 100, 76
    ref0, cur0 = _case(w, h, 20)
    ref1, cur1 = _case(w, h, 21)
    st = torch.cuda.Stream()
    sh = ctypes.c_void_p(st.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(st):
        rt, ct = _t(ref0), _t(cur0)
        F = me.PartitionFields.device(w, h, 16)
        leaf_t = torch.zeros((me.partition_counts(w, h, 16)[3], 2), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: (eng.partition_search_device(rt, ct, 16, 7, 16, F, stream=sh),
                                     eng.partition_leaf_field_device(w, h, 16, F, leaf_t, stream=sh)))
        rt.copy_(_t(ref1))
        ct.copy_(_t(cur1))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        want = P.decide(_expected(w, h, 21, 16, 7), 16)
        _check(F.numpy(), want)
        np.testing.assert_array_equal(leaf_t.cpu().numpy(), P.leaf_field(want))


# ---- host planes: the synchronous entry point equals the device one
@pytest.mark.parametrize("w,h,B,S,width", [(96, 64, 16, 7, None), (44, 28, 16, 5, None),
                                            (70, 40, 32, 5, None), (112, 64, 16, 7, 100)])
def test_host_entry_point(engine, w, h, B, S, width):
    ref, cur = _case(w, h, 7)
    got = engine.partition_search(ref, cur, B, S, 16, width=width)
    fw = width or w
    want = P.search_frame(ref[:, :fw], cur[:, :fw], B, S, 16)
    _check(got, want)
    _check(_device(engine, ref, cur, B, S, 16, width=width), want)
