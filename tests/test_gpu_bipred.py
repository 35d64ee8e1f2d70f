"""GPU: bi-predictive mode decision, joint refinement and compensation
(csrc/me_subpel.hip through the C ABI) against tests/bipred_ref.py, the numpy
restatement of the definition in include/me.h.  Everything is exact integer
arithmetic: vectors, modes, costs and planes are compared with
assert_array_equal, PSNR doubles with ==.

Shapes cover one-pixel blocks, partial blocks and every tile size the kernels
are built for (4, 8, 16, 32, 64).  "Planted" frames (bipred_ref.planted) have a
known answer of every mode and inputs one quarter step off it, so that the
mode decision and both refinement passes have something to find; the oracle's
own result is checked for that before the kernel's is compared with it."""
import ctypes
import functools

import numpy as np
import pytest

import bipred_ref as B
import oracle_lib as O
import qpel_ref as Q
import motionestimation_amd as me
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5, 4), (33, 17, 16), (130, 75, 8), (1025, 3, 1), (192, 70, 64), (70, 40, 32)]
POST_SHAPES = SHAPES + [(641, 363, 16)]


def _equal(got, want, msg=""):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (msg, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=msg)


@functools.lru_cache(maxsize=None)
def _planted(w, h, blk):
    out = B.planted(w, h, blk, 100 + w)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _planted_oracle(w, h, blk, cost, refine):
    out = B.bipred(*_planted(w, h, blk)[:3], blk, *_planted(w, h, blk)[3:], cost, refine)
    for a in out:
        a.setflags(write=False)
    return out


def _stream():
    import torch
    s = torch.cuda.Stream()
    return s, ctypes.c_void_p(s.cuda_stream)


# ------------------------------------------------------------ parity
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_planted_parity(engine, w, h, blk, cost):
    ref0, ref1, cur, q0, q1 = _planted(w, h, blk)
    plain = _planted_oracle(w, h, blk, cost, 0)
    fine = _planted_oracle(w, h, blk, cost, 1)
    n = len(q0)
    if n >= 6:
        # not vacuous: every mode is chosen on at least 10 % of the blocks and
        # the joint refinement moves a vector (strictly lowers cb) in at
        # least half of them
        assert (np.bincount(fine[2], minlength=3) >= 0.1 * n).all(), np.bincount(fine[2])
        assert np.mean(fine[4][:, 2] < plain[4][:, 2]) >= 0.5
    for refine, want in ((0, plain), (1, fine)):
        got = engine.bipred(ref0, ref1, cur, blk, q0, q1, cost, refine)
        _equal(got, want, f"{w}x{h} B{blk} {cost} refine {refine}")


def _checker(w, h, p=3):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx // p + yy // p) & 1) * 255).astype(np.uint8)


def _parked(kind, w, h, blk, rng):
    """Quarter-pel fields whose blocks sit in the frame's corners (taps over
    the edge) or wholly outside it (clamping defines them), plus a fraction."""
    blocks = list(Q._blocks(w, h, blk))
    if kind == "corners":
        mv = np.array([(((n & 1) * (w - bw)) - x0, ((n >> 1 & 1) * (h - bh)) - y0)
                       for n, (x0, y0, bw, bh) in enumerate(blocks)])
    else:
        away = np.array([(w, 0), (-w, 0), (0, h), (0, -h), (w, -h)])
        mv = away[(np.arange(len(blocks)) + int(rng.integers(0, 5))) % len(away)]
    return (4 * mv + rng.integers(-3, 4, mv.shape)).astype(np.int16)


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_checkerboard_and_parked_fields_parity(engine, w, h, blk, cost):
    """0/255 checkerboards of period 3 (the clip255 sites reach both ends,
    test_qpel_ref.py) against a random cur, and random references with fields
    in the corners and outside the frame."""
    rng = np.random.default_rng(200 + w)
    n = O.num_blocks(w, h, blk)
    cur = rng.integers(0, 256, (h, w)).astype(np.uint8)
    board0, board1 = _checker(w, h), 255 - _checker(w, h)[:, ::-1]
    rnd0 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    rnd1 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    cases = [("checker", board0, board1, rng.integers(-9, 10, (n, 2)).astype(np.int16),
              rng.integers(-9, 10, (n, 2)).astype(np.int16))]
    for kind in ("corners", "outside"):
        cases.append((kind, rnd0, rnd1, _parked(kind, w, h, blk, rng), _parked(kind, w, h, blk, rng)))
    for name, ref0, ref1, q0, q1 in cases:
        for refine in (0, 1):
            got = engine.bipred(ref0, ref1, cur, blk, q0, q1, cost, refine)
            _equal(got, B.bipred(ref0, ref1, cur, blk, q0, q1, cost, refine),
                   f"{w}x{h} B{blk} {cost} {name} refine {refine}")


# ------------------------------------------------------------ device entry
@pytest.mark.parametrize("cost,blk", [("sad", 16), ("ssd", 32)])
def test_device_entry_batch_pitch_in_place(engine, cost, blk):
    """Three frames of width 90 in rows of 96 bytes whose pad columns and spare
    rows hold other data, three different frame strides, outputs in place;
    then out of place without the optional outputs."""
    import torch
    w, h, pitch = 90, 70, 96
    rng = np.random.default_rng(71)
    big = [rng.integers(0, 256, (3, rows, pitch)).astype(np.uint8) for rows in (75, 77, 72)]
    n = me.num_blocks(w, h, blk)
    q0 = rng.integers(-40, 41, (3 * n, 2)).astype(np.int16)
    q1 = rng.integers(-40, 41, (3 * n, 2)).astype(np.int16)
    r0t, r1t, ct = (torch.from_numpy(a).cuda()[:, :h] for a in big)
    assert len({t.stride(0) for t in (r0t, r1t, ct)}) == 3
    want = [B.bipred(big[0][f, :h, :w], big[1][f, :h, :w], big[2][f, :h, :w], blk,
                     q0[f * n:(f + 1) * n], q1[f * n:(f + 1) * n], cost, 1) for f in range(3)]
    want = [np.concatenate([wf[k] for wf in want]) for k in range(5)]
    a0, a1 = torch.from_numpy(q0.copy()).cuda(), torch.from_numpy(q1.copy()).cuda()
    mode = torch.full((3 * n,), 9, dtype=torch.uint8, device="cuda")
    cost_t = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    cost3_t = torch.zeros((3 * n, 3), dtype=torch.int32, device="cuda")
    engine.bipred_device(r0t, r1t, ct, blk, cost, a0, a1, mode, None, None, cost_t, cost3_t,
                         width=w, height=h)
    torch.cuda.synchronize()
    got = (a0.cpu().numpy(), a1.cpu().numpy(), mode.cpu().numpy(),
           cost_t.cpu().numpy().view(np.uint32), cost3_t.cpu().numpy().view(np.uint32))
    _equal(got, want)
    # out of place, no cost arrays: the inputs stay as they were
    i0, i1 = torch.from_numpy(q0.copy()).cuda(), torch.from_numpy(q1.copy()).cuda()
    o0, o1 = torch.zeros_like(i0), torch.zeros_like(i1)
    mode.fill_(9)
    engine.bipred_device(r0t, r1t, ct, blk, cost, i0, i1, mode, o0, o1, None, None,
                         width=w, height=h)
    torch.cuda.synchronize()
    _equal((o0.cpu().numpy(), o1.cpu().numpy(), mode.cpu().numpy()), want[:3])
    np.testing.assert_array_equal(i0.cpu().numpy(), q0)
    np.testing.assert_array_equal(i1.cpu().numpy(), q1)
    engine.device_check()


def test_captured_without_warm_up():
    """The first call of a fresh context is the captured one: the kernel uses
    no context scratch.  Replayed once, on new frame contents."""
    import torch
    w, h, blk = 130, 75, 8
    ref0, ref1, cur, q0, q1 = _planted(w, h, blk)
    n = len(q0)
    s, sh = _stream()
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(s):
        r0t, r1t, ct = (torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(3))
        i0, i1 = torch.zeros((n, 2), dtype=torch.int16, device="cuda"), \
            torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        o0, o1 = torch.zeros_like(i0), torch.zeros_like(i1)
        mode = torch.zeros(n, dtype=torch.uint8, device="cuda")
        cost_t = torch.zeros(n, dtype=torch.int32, device="cuda")
        cost3_t = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: eng.bipred_device(r0t, r1t, ct, blk, "ssd", i0, i1, mode, o0,
                                                      o1, cost_t, cost3_t, stream=sh))
        for t, a in ((r0t, ref0), (r1t, ref1), (ct, cur), (i0, q0), (i1, q1)):
            t.copy_(torch.from_numpy(np.array(a)))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        got = (o0.cpu().numpy(), o1.cpu().numpy(), mode.cpu().numpy(),
               cost_t.cpu().numpy().view(np.uint32), cost3_t.cpu().numpy().view(np.uint32))
    _equal(got, _planted_oracle(w, h, blk, "ssd", 1))


# ------------------------------------------------------------ end to end
FOREMAN_SUM = {"ssd": 1146937, "sad": 194980}


@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_foreman_full_search_bipred(engine, cost):
    ref0, ref1, cur, q0, _, q1, _ = B.foreman(cost)
    want = B.bipred(ref0, ref1, cur, 16, q0, q1, cost, 1)
    hist = np.bincount(want[2], minlength=3)
    assert hist[0] >= 100 and hist[1] >= 20 and hist[2] >= 200, hist
    got = engine.full_search_bipred(ref0, ref1, cur, 16, 7, cost)
    _equal(got, want[:4], cost)
    assert int(got[3].astype(np.int64).sum()) == FOREMAN_SUM[cost]
    # the chain's steps one by one give the same
    f0, f1 = engine.full_search_qpel(ref0, cur, 16, 7, cost)[0], \
        engine.full_search_qpel(ref1, cur, 16, 7, cost)[0]
    np.testing.assert_array_equal(f0, q0)
    np.testing.assert_array_equal(f1, q1)
    _equal(engine.bipred(ref0, ref1, cur, 16, f0, f1, cost, 1), want, cost)
    mc = B.compensate(ref0, ref1, 16, want[0], want[1], want[2])
    out, psnr = engine.compensate_planes_bipred(ref0, ref1, cur, 16, got[0], got[1], got[2])
    np.testing.assert_array_equal(out, Q.planes(ref0, cur, mc))
    assert psnr == O.psnr(mc, cur)
    _, psnr0 = engine.compensate_planes_qpel(ref0, cur, 16, q0)
    assert psnr > psnr0


# ---------------------------------------------------------- compensation
@pytest.mark.parametrize("w,h,blk", POST_SHAPES)
def test_compensation_parity(engine, w, h, blk):
    rng = np.random.default_rng(80 + w)
    ref0, ref1, cur = (rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(3))
    n = me.num_blocks(w, h, blk)
    mode = rng.integers(0, 3, n).astype(np.uint8)
    # random quarter-pel vectors within +-12 pixels, and any int16
    for lo, hi in ((-48, 49), (-32768, 32768)):
        v0 = rng.integers(lo, hi, (n, 2)).astype(np.int16)
        v1 = rng.integers(lo, hi, (n, 2)).astype(np.int16)
        mc = B.compensate(ref0, ref1, blk, v0, v1, mode)
        np.testing.assert_array_equal(engine.motion_compensate_bipred(ref0, ref1, blk, v0, v1, mode), mc)
        out, psnr = engine.compensate_planes_bipred(ref0, ref1, cur, blk, v0, v1, mode)
        np.testing.assert_array_equal(out, Q.planes(ref0, cur, mc))
        assert psnr == O.psnr(mc, cur)
        # all L0: the quarter-pel compensation from ref0, byte for byte
        l0 = np.zeros(n, np.uint8)
        out0, psnr0 = engine.compensate_planes_bipred(ref0, ref1, cur, blk, v0, v1, l0)
        outq, psnrq = engine.compensate_planes_qpel(ref0, cur, blk, v0)
        np.testing.assert_array_equal(out0, outq)
        assert psnr0 == psnrq
        np.testing.assert_array_equal(
            engine.motion_compensate_bipred(ref0, ref1, blk, v0, v1, np.ones(n, np.uint8)),
            engine.motion_compensate_qpel(ref1, blk, v1))
    # identical planes and zero fields: the mse == 0 branch, in BI mode
    z = np.zeros((n, 2), np.int16)
    _, psnr = engine.compensate_planes_bipred(ref0, ref0, ref0, blk, z, z, np.full(n, 2, np.uint8))
    assert psnr == 99.0


# ---------------------------------------------------------------- errors
def test_errors(engine):
    import torch
    L, h = _lib.lib(), engine._h
    w, ht, blk = 48, 32, 16
    n = me.num_blocks(w, ht, blk)
    ref = np.zeros((ht, w), np.uint8)
    q = np.zeros((n, 2), np.int16)
    o0, o1 = np.zeros((n, 2), np.int16), np.zeros((n, 2), np.int16)
    mode = np.zeros(n, np.uint8)
    out = np.zeros((5 * ht, w), np.uint8)
    p = lambda a: a.ctypes.data

    def failed(status, want):
        assert status == want, (status, want)
        assert L.me_last_error(h), "me_last_error is empty"

    # SSIM
    with pytest.raises(me.MEError) as ei:
        engine.bipred(ref, ref, ref, blk, q, q, "ssim")
    assert ei.value.status == _lib.ME_EUNSUPPORTED and L.me_last_error(h)
    with pytest.raises(me.MEError) as ei:
        engine.full_search_bipred(ref, ref, ref, blk, 4, "ssim")
    assert ei.value.status == _lib.ME_EUNSUPPORTED and L.me_last_error(h)
    # a context with several devices
    with me.Engine(devices=[0, 0]) as two:
        with pytest.raises(me.MEError) as ei:
            two.full_search_bipred(ref, ref, ref, blk, 4, "sad")
        assert ei.value.status == _lib.ME_EUNSUPPORTED
    # the range of an input component
    for which in (0, 1):
        for bad in (32767, -32767, -32768):
            far = [q.copy(), q.copy()]
            far[which][n - 1, 1] = bad
            with pytest.raises(me.MEError) as ei:
                engine.bipred(ref, ref, ref, blk, far[0], far[1], "sad")
            assert ei.value.status == _lib.ME_EINVAL and L.me_last_error(h)
    edge = q.copy()
    edge[0] = (_lib.ME_BIPRED_MAX_Q, -_lib.ME_BIPRED_MAX_Q)
    got = engine.bipred(ref, ref, ref, blk, edge, edge, "sad")
    np.testing.assert_array_equal(got[0], edge)  # flat frames: L0, unchanged
    assert not got[2].any()
    # a mode byte above 2
    bad_mode = mode.copy()
    bad_mode[n - 1] = 3
    with pytest.raises(me.MEError) as ei:
        engine.compensate_planes_bipred(ref, ref, ref, blk, q, q, bad_mode)
    assert ei.value.status == _lib.ME_EINVAL and L.me_last_error(h)
    with pytest.raises(me.MEError) as ei:
        engine.motion_compensate_bipred(ref, ref, blk, q, q, bad_mode)
    assert ei.value.status == _lib.ME_EINVAL and L.me_last_error(h)
    # null pointers, one argument at a time
    good = [p(ref), p(ref), p(ref), w, ht, w, blk, 1, 1, p(q), p(q), p(o0), p(o1), p(mode), None, None]
    for k in (0, 1, 2, 9, 10, 11, 12, 13):
        a = list(good)
        a[k] = None
        failed(L.me_bipred(h, *a), _lib.ME_EINVAL)
    good = [p(ref), p(ref), p(ref), w, ht, w, blk, 4, 1, p(o0), p(o1), p(mode), None]
    for k in (0, 1, 2, 9, 10, 11):
        a = list(good)
        a[k] = None
        failed(L.me_full_search_bipred(h, *a), _lib.ME_EINVAL)
    good = [p(ref), p(ref), p(ref), w, ht, blk, p(q), p(q), p(mode), p(out), None]
    for k in (0, 1, 2, 6, 7, 8, 9):
        a = list(good)
        a[k] = None
        failed(L.me_compensate_planes_bipred(h, *a), _lib.ME_EINVAL)
    good = [p(ref), p(ref), w, ht, blk, p(q), p(q), p(mode), p(out)]
    for k in (0, 1, 5, 6, 7, 8):
        a = list(good)
        a[k] = None
        failed(L.me_motion_compensate_bipred(h, *a), _lib.ME_EINVAL)
    # the device entry
    rt = torch.from_numpy(ref).cuda()
    qt = torch.from_numpy(q).cuda()
    mt = torch.from_numpy(mode).cuda()
    d = lambda t: t.data_ptr()
    good = [d(rt), 0, d(rt), 0, d(rt), 0, w, ht, w, blk, 1, 1, 1, d(qt), d(qt), d(qt), d(qt), d(mt),
            None, None, None]
    for k in (0, 2, 4, 13, 14, 15, 16, 17):
        a = list(good)
        a[k] = None
        failed(L.me_bipred_device(h, *a), _lib.ME_EINVAL)
    for frames in (0, -1):
        a = list(good)
        a[12] = frames
        failed(L.me_bipred_device(h, *a), _lib.ME_EINVAL)
    a = list(good)
    a[10] = 2  # ME_COST_SSIM
    failed(L.me_bipred_device(h, *a), _lib.ME_EUNSUPPORTED)
    a = list(good)
    a[12], a[1], a[3], a[5] = 2, w * ht, w, w * ht  # overlapping ref1 frames of a batch
    failed(L.me_bipred_device(h, *a), _lib.ME_EINVAL)
    torch.cuda.synchronize()
    engine.device_check()
