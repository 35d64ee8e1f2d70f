"""GPU: quarter-pel refinement and sub-pel compensation (csrc/me_subpel.hip
through the C ABI) against tests/qpel_ref.py, the numpy restatement of the
definition in include/me.h.  Everything is exact integer arithmetic: vectors,
costs and planes are compared with assert_array_equal, PSNR doubles with ==.

Shapes cover one-pixel blocks, partial blocks, a block that is the frame and
one larger than it, every tile size the kernels are built for (4, 8, 16, 64;
32 through the batch test) and a row pitch wider than the frame.  Frames are
random bytes and 0/255 checkerboards of period 1 and 3, whose edges drive the
three clip255 sites to both ends; fields are searched, random, parked in the
frame's corners (taps over the edge) and wholly outside the frame (clamping
defines them)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import qpel_ref as Q
import motionestimation_amd as me
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5, 4), (33, 17, 16), (130, 75, 8), (96, 64, 16), (1025, 3, 1), (64, 64, 64),
          (50, 40, 64)]
POST_SHAPES = [(7, 5, 4), (33, 17, 16), (130, 75, 8), (641, 363, 16), (1025, 3, 1), (64, 64, 64),
               (50, 40, 64)]
FRAMES = ["random", "checker1", "checker3"]
FIELDS = ["searched", "inframe", "corners", "outside"]


def _frames(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    cur = rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "random":
        return rng.integers(0, 256, (h, w)).astype(np.uint8), cur
    p = int(kind[-1])
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx // p + yy // p) & 1) * 255).astype(np.uint8)), cur


def _field(kind, ref, cur, blk, cost, seed):
    h, w = ref.shape
    rng = np.random.default_rng(seed)
    blocks = list(Q._blocks(w, h, blk))
    if kind == "searched":
        return O.full_search(ref, cur, blk, 3, cost, threads=16)[0]
    if kind == "inframe":
        return np.array([(rng.integers(-x0, w - bw - x0 + 1), rng.integers(-y0, h - bh - y0 + 1))
                         for x0, y0, bw, bh in blocks], np.int16)
    if kind == "corners":
        return np.array([(((n & 1) * (w - bw)) - x0, ((n >> 1 & 1) * (h - bh)) - y0)
                         for n, (x0, y0, bw, bh) in enumerate(blocks)], np.int16)
    away = np.array([(w, 0), (-w, 0), (0, h), (0, -h), (w, -h)], np.int16)
    return away[np.arange(len(blocks)) % len(away)]


@functools.lru_cache(maxsize=None)
def _foreman():
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    ref.setflags(write=False)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def _foreman_ref(cost):
    """(integer field, its costs, oracle q, oracle costs), computed once."""
    ref, cur = _foreman()
    mv, c, _ = O.full_search(ref, cur, 16, 7, cost, threads=16)
    q, qc = Q.refine(ref, cur, 16, mv, cost)
    for a in (mv, c, q, qc):
        a.setflags(write=False)
    return mv, c, q, qc


def _stream():
    import torch
    s = torch.cuda.Stream()
    return s, ctypes.c_void_p(s.cuda_stream)


# ------------------------------------------------------------ refinement
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_refinement_parity(engine, w, h, blk, cost):
    for fk in FRAMES:
        ref, cur = _frames(fk, w, h, 10 + w)
        for k in FIELDS:
            mv = _field(k, ref, cur, blk, cost, 20 + h)
            q, c = engine.refine_qpel(ref, cur, blk, mv, cost)
            oq, oc = Q.refine(ref, cur, blk, mv, cost)
            msg = f"{w}x{h} B{blk} {cost} {fk} {k}"
            np.testing.assert_array_equal(q, oq, err_msg=msg)
            np.testing.assert_array_equal(c, oc, err_msg=msg)


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_refinement_device_entry_with_pitch(engine, cost):
    """Width 100 in rows of 112 bytes; the pad columns hold other data."""
    import torch
    w, h, blk, pitch = 100, 40, 16, 112
    rng = np.random.default_rng(31)
    big_r = rng.integers(0, 256, (h, pitch)).astype(np.uint8)
    big_c = rng.integers(0, 256, (h, pitch)).astype(np.uint8)
    ref, cur = big_r[:, :w].copy(), big_c[:, :w].copy()
    n = me.num_blocks(w, h, blk)
    for k in FIELDS:
        mv = _field(k, ref, cur, blk, cost, 32)
        rt, ct = torch.from_numpy(big_r).cuda(), torch.from_numpy(big_c).cuda()
        mvt = torch.from_numpy(mv.copy()).cuda()
        qt = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        cot = torch.zeros(n, dtype=torch.int32, device="cuda")
        engine.refine_qpel_device(rt, ct, blk, cost, mvt, qt, cot, width=w, height=h)
        torch.cuda.synchronize()
        oq, oc = Q.refine(ref, cur, blk, mv, cost)
        np.testing.assert_array_equal(qt.cpu().numpy(), oq, err_msg=k)
        np.testing.assert_array_equal(cot.cpu().numpy().view(np.uint32), oc, err_msg=k)
        np.testing.assert_array_equal(mvt.cpu().numpy(), mv)  # the input field is untouched
        # without a cost array
        qt.zero_()
        engine.refine_qpel_device(rt, ct, blk, cost, mvt, qt, None, width=w, height=h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(qt.cpu().numpy(), oq, err_msg=k)


@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (50, 40, 64), (40, 24, 8)])
@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_ties_keep_the_integer_vector(engine, w, h, blk, cost):
    """Flat frames: every candidate costs 0, the centre keeps the tie."""
    flat = np.full((h, w), 93, np.uint8)
    rng = np.random.default_rng(41)
    mv = rng.integers(-40, 41, (me.num_blocks(w, h, blk), 2)).astype(np.int16)
    q, c = engine.refine_qpel(flat, flat, blk, mv, cost)
    np.testing.assert_array_equal(q, 4 * mv)
    assert not c.any()


@pytest.mark.parametrize("cost,blk", [("sad", 16), ("ssd", 32)])
def test_batch_in_place_equals_single_frames(engine, cost, blk):
    """Three frames whose strides exceed a frame, refined in place."""
    import torch
    w, h, pitch, rows = 90, 70, 96, 75
    rng = np.random.default_rng(51)
    big_r = rng.integers(0, 256, (3, rows, pitch)).astype(np.uint8)
    big_c = rng.integers(0, 256, (3, rows + 2, pitch)).astype(np.uint8)
    n = me.num_blocks(w, h, blk)
    mv = rng.integers(-9, 10, (3 * n, 2)).astype(np.int16)
    rt = torch.from_numpy(big_r).cuda()[:, :h]
    ct = torch.from_numpy(big_c).cuda()[:, :h]
    assert rt.stride(0) == rows * pitch and ct.stride(0) == (rows + 2) * pitch
    mvt = torch.from_numpy(mv.copy()).cuda()
    cot = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    engine.refine_qpel_device(rt, ct, blk, cost, mvt, None, cot, width=w, height=h)
    torch.cuda.synchronize()
    got_q, got_c = mvt.cpu().numpy(), cot.cpu().numpy().view(np.uint32)
    for f in range(3):
        ref, cur = big_r[f, :h, :w].copy(), big_c[f, :h, :w].copy()
        one = torch.from_numpy(mv[f * n:(f + 1) * n].copy()).cuda()
        one_c = torch.zeros(n, dtype=torch.int32, device="cuda")
        engine.refine_qpel_device(rt[f], ct[f], blk, cost, one, None, one_c, width=w, height=h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got_q[f * n:(f + 1) * n], one.cpu().numpy())
        np.testing.assert_array_equal(got_c[f * n:(f + 1) * n], one_c.cpu().numpy().view(np.uint32))
        oq, oc = Q.refine(ref, cur, blk, mv[f * n:(f + 1) * n], cost)
        np.testing.assert_array_equal(got_q[f * n:(f + 1) * n], oq)
        np.testing.assert_array_equal(got_c[f * n:(f + 1) * n], oc)


# ------------------------------------------------------------ end to end
@pytest.mark.parametrize("cost", ["ssd", "sad"])
def test_foreman_end_to_end(engine, cost):
    ref, cur = _foreman()
    mv, c, oq, oc = _foreman_ref(cost)
    # not vacuous: the oracle's own field is mostly fractional
    assert np.mean((oq % 4 != 0).any(axis=1)) >= 0.5
    assert np.mean((oq % 2 != 0).any(axis=1)) >= 0.5
    q, qc = engine.full_search_qpel(ref, cur, 16, 7, cost)
    imv, ic = engine.full_search(ref, cur, 16, 7, cost)
    np.testing.assert_array_equal(imv, mv)
    q2, qc2 = engine.refine_qpel(ref, cur, 16, imv, cost)
    np.testing.assert_array_equal(q, q2)
    np.testing.assert_array_equal(qc, qc2)
    np.testing.assert_array_equal(q, oq)
    np.testing.assert_array_equal(qc, oc)
    assert (qc <= ic).all()
    mc = Q.compensate(ref, 16, oq)
    out, psnr = engine.compensate_planes_qpel(ref, cur, 16, q)
    np.testing.assert_array_equal(out, Q.planes(ref, cur, mc))
    assert psnr == O.psnr(mc, cur)
    _, ipsnr = engine.compensate_planes(ref, cur, 16, imv)
    assert psnr > ipsnr


# ---------------------------------------------------------- compensation
@pytest.mark.parametrize("w,h,blk", POST_SHAPES)
def test_compensation_parity(engine, w, h, blk):
    rng = np.random.default_rng(60 + w)
    ref = rng.integers(0, 256, (h, w)).astype(np.uint8)
    cur = rng.integers(0, 256, (h, w)).astype(np.uint8)
    n = me.num_blocks(w, h, blk)
    # in-frame multiples of 4: the integer compensation, byte for byte
    mv = _field("inframe", ref, cur, blk, "ssd", 61)
    imc = engine.motion_compensate(ref, blk, mv)
    np.testing.assert_array_equal(imc, O.motion_compensate(ref, blk, mv))
    np.testing.assert_array_equal(engine.motion_compensate_qpel(ref, blk, 4 * mv), imc)
    # random quarter-pel vectors within +-12 pixels, and any int16
    for q in (rng.integers(-48, 49, (n, 2)).astype(np.int16),
              rng.integers(-32768, 32768, (n, 2)).astype(np.int16)):
        mc = Q.compensate(ref, blk, q)
        np.testing.assert_array_equal(engine.motion_compensate_qpel(ref, blk, q), mc)
        out, psnr = engine.compensate_planes_qpel(ref, cur, blk, q)
        np.testing.assert_array_equal(out, Q.planes(ref, cur, mc))
        assert psnr == O.psnr(mc, cur)
    # identical planes and a zero field: the mse == 0 branch
    out, psnr = engine.compensate_planes_qpel(ref, ref, blk, np.zeros((n, 2), np.int16))
    assert psnr == 99.0


# ---------------------------------------------------------------- errors
def test_errors(engine):
    import torch
    L, h = _lib.lib(), engine._h
    w, ht, blk = 48, 32, 16
    n = me.num_blocks(w, ht, blk)
    ref = np.zeros((ht, w), np.uint8)
    mv = np.zeros((n, 2), np.int16)
    q = np.zeros((n, 2), np.int16)
    p = lambda a: a.ctypes.data

    def failed(status, want):
        assert status == want, (status, want)
        assert L.me_last_error(h), "me_last_error is empty"

    for fn in (engine.refine_qpel, engine.full_search_qpel):
        with pytest.raises(me.MEError) as ei:
            fn(ref, ref, blk, mv if fn == engine.refine_qpel else 4, "ssim")
        assert ei.value.status == _lib.ME_EUNSUPPORTED and L.me_last_error(h)
    failed(L.me_refine_qpel(h, p(ref), p(ref), w, ht, w, blk, 0, p(mv), None, None), _lib.ME_EINVAL)
    failed(L.me_refine_qpel(h, p(ref), p(ref), w, ht, w, blk, 0, None, p(q), None), _lib.ME_EINVAL)
    failed(L.me_full_search_qpel(h, p(ref), p(ref), w, ht, w, blk, 4, 0, None, None), _lib.ME_EINVAL)
    failed(L.me_motion_compensate_qpel(h, p(ref), w, ht, blk, p(q), None), _lib.ME_EINVAL)
    failed(L.me_compensate_planes_qpel(h, p(ref), p(ref), w, ht, blk, p(q), None, None),
           _lib.ME_EINVAL)
    for bad in (_lib.ME_QPEL_MAX_MV + 1, -_lib.ME_QPEL_MAX_MV - 1):
        far = mv.copy()
        far[n - 1, 1] = bad
        with pytest.raises(me.MEError) as ei:
            engine.refine_qpel(ref, ref, blk, far, "sad")
        assert ei.value.status == _lib.ME_EINVAL and L.me_last_error(h)
    edge = mv.copy()
    edge[0] = (_lib.ME_QPEL_MAX_MV, -_lib.ME_QPEL_MAX_MV)
    got, _ = engine.refine_qpel(ref, ref, blk, edge, "sad")
    np.testing.assert_array_equal(got, 4 * edge)
    # the device entry
    rt = torch.from_numpy(ref).cuda()
    mvt = torch.from_numpy(mv).cuda()
    d = lambda t: t.data_ptr()
    for frames in (0, -1):
        failed(L.me_refine_qpel_device(h, d(rt), 0, d(rt), 0, w, ht, w, blk, 1, frames, d(mvt),
                                       d(mvt), None, None), _lib.ME_EINVAL)
    failed(L.me_refine_qpel_device(h, d(rt), 0, d(rt), 0, w, ht, w, blk, 1, 1, d(mvt), None, None,
                                   None), _lib.ME_EINVAL)
    failed(L.me_refine_qpel_device(h, d(rt), 0, d(rt), 0, w, ht, w, blk, 1, 1, None, d(mvt), None,
                                   None), _lib.ME_EINVAL)
    failed(L.me_refine_qpel_device(h, d(rt), 0, d(rt), 0, w, ht, w, blk, 2, 1, d(mvt), d(mvt), None,
                                   None), _lib.ME_EUNSUPPORTED)
    # overlapping frames of a batch
    failed(L.me_refine_qpel_device(h, d(rt), w, d(rt), w, w, ht, w, blk, 1, 2, d(mvt), d(mvt), None,
                                   None), _lib.ME_EINVAL)
    torch.cuda.synchronize()
    engine.device_check()


# --------------------------------------------------------- captured step
def test_captured_search_and_refinement():
    """Search then refinement in one graph (a linear chain), replayed on new
    frame contents.  Only the search runs uncaptured first: the refinement
    uses no context scratch."""
    import torch
    from motionestimation_amd import synth
    w, h, blk, span = 176, 144, 16, 8
    ref0, cur0 = synth.frame_pair(w, h, 7, 2, -1)
    ref1, cur1 = synth.frame_pair(w, h, 8, -3, 2)
    n = me.num_blocks(w, h, blk)
    s, sh = _stream()
    for cost in ("sad", "ssd"):
        with me.Engine(devices=[0]) as eng, torch.cuda.stream(s):
            rt, ct = torch.from_numpy(ref0).cuda(), torch.from_numpy(cur0).cuda()
            mvt = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
            qt = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
            cot = torch.zeros(n, dtype=torch.int32, device="cuda")
            search = lambda: eng.full_search_device(rt, ct, blk, span, cost, mvt, cot, stream=sh)
            refine = lambda: eng.refine_qpel_device(rt, ct, blk, cost, mvt, qt, cot, stream=sh)
            search()
            torch.cuda.synchronize()
            g = eng.capture(sh, lambda: (search(), refine()))
            rt.copy_(torch.from_numpy(ref1))
            ct.copy_(torch.from_numpy(cur1))
            qt.zero_()
            g.launch(sh)
            torch.cuda.synchronize()
            eng.device_check()
            omv = O.full_search(ref1, cur1, blk, span, cost, threads=16)[0]
            oq, oc = Q.refine(ref1, cur1, blk, omv, cost)
            np.testing.assert_array_equal(mvt.cpu().numpy(), omv)
            np.testing.assert_array_equal(qt.cpu().numpy(), oq)
            np.testing.assert_array_equal(cot.cpu().numpy().view(np.uint32), oc)


# -------------------------------------------------------- context sharing
def test_context_still_serves_integer_calls(engine):
    """After the quarter-pel calls above, the shared context's integer search
    and compensation still equal the oracle."""
    from motionestimation_amd import synth
    ref, cur = synth.frame_pair(176, 144, 5, 2, -3)
    q, _ = engine.full_search_qpel(ref, cur, 16, 8, "sad")
    mv, c = engine.full_search(ref, cur, 16, 8, "sad")
    omv, oc, _ = O.full_search(ref, cur, 16, 8, "sad", threads=16)
    np.testing.assert_array_equal(mv, omv)
    np.testing.assert_array_equal(c, oc)
    np.testing.assert_array_equal(q, Q.refine(ref, cur, 16, omv, "sad")[0])
    mc = O.motion_compensate(ref, 16, mv)
    out, psnr = engine.compensate_planes(ref, cur, 16, mv)
    np.testing.assert_array_equal(out, Q.planes(ref, cur, mc))
    assert psnr == O.psnr(mc, cur)
    engine.device_check()
