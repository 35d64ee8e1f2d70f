"""GPU: the SATD cost (include/me.h "SATD cost") in the quarter-pel refinement,
the rate-constrained refinement, the bi-prediction and their composite entry
points (csrc/me_subpel.hip through the C ABI) against tests/satd_ref.py, the
numpy restatement of the definition.  Everything is exact integer arithmetic:
vectors, modes and costs are compared with assert_array_equal.

Shapes cover every tile size the kernels are built for (4, 8, 16, 32, 64),
block sizes that are not multiples of 4 (partial Hadamard tiles on both
edges), one-pixel blocks, a block that is the frame and one larger than it.
Frames and fields are those of test_gpu_qpel.py (generators copied): random
bytes and 0/255 checkerboards; searched, random, corner and out-of-frame
fields."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import qpel_ref as Q
import satd_ref as S
import motionestimation_amd as me
from motionestimation_amd import _lib, synth

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5, 4), (23, 17, 5), (33, 17, 16), (130, 75, 8), (96, 64, 16), (70, 40, 32),
          (1025, 3, 1), (64, 64, 64), (50, 40, 64)]
BIPRED_SHAPES = [(7, 5, 4), (33, 17, 16), (130, 75, 8), (70, 40, 32), (192, 70, 64)]
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


def _field(kind, ref, cur, blk, seed):
    h, w = ref.shape
    rng = np.random.default_rng(seed)
    blocks = list(Q._blocks(w, h, blk))
    if kind == "searched":  # the integer step of an SATD refinement runs at SAD
        return O.full_search(ref, cur, blk, 3, "sad", threads=16)[0]
    if kind == "inframe":
        return np.array([(rng.integers(-x0, w - bw - x0 + 1), rng.integers(-y0, h - bh - y0 + 1))
                         for x0, y0, bw, bh in blocks], np.int16)
    if kind == "corners":
        return np.array([(((n & 1) * (w - bw)) - x0, ((n >> 1 & 1) * (h - bh)) - y0)
                         for n, (x0, y0, bw, bh) in enumerate(blocks)], np.int16)
    away = np.array([(w, 0), (-w, 0), (0, h), (0, -h), (w, -h)], np.int16)
    return away[np.arange(len(blocks)) % len(away)]


def _stream():
    import torch
    s = torch.cuda.Stream()
    return s, ctypes.c_void_p(s.cuda_stream)


def _equal(got, want, msg=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{msg} [output {k}]")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------ refinement
@pytest.mark.parametrize("w,h,blk", SHAPES)
def test_refinement_parity(engine, w, h, blk):
    for fk in FRAMES:
        ref, cur = _frames(fk, w, h, 10 + w)
        for k in FIELDS:
            mv = _field(k, ref, cur, blk, 20 + h)
            q, c = engine.refine_qpel(ref, cur, blk, mv, "satd")
            oq, oc = S.refine(ref, cur, blk, mv)
            msg = f"{w}x{h} B{blk} {fk} {k}"
            np.testing.assert_array_equal(q, oq, err_msg=msg)
            np.testing.assert_array_equal(c, oc, err_msg=msg)


@functools.lru_cache(maxsize=None)
def _discriminating():
    """synth.frame_pair(96, 64, 7, 2, -1), 16x16, every block started at
    (2, -1): (ref, cur, mv, SATD oracle q, its costs, SAD oracle q)."""
    ref, cur = synth.frame_pair(96, 64, 7, 2, -1)
    mv = np.tile(np.array([[2, -1]], np.int16), (24, 1))
    q, c = S.refine(ref, cur, 16, mv)
    sq, _ = Q.refine(ref, cur, 16, mv, "sad")
    for a in (ref, cur, mv, q, c, sq):
        a.setflags(write=False)
    return ref, cur, mv, q, c, sq


def test_satd_is_not_sad(engine):
    """The two costs choose different vectors here (13 of 24 blocks when this
    was written), so a kernel that quietly costs SAD fails."""
    ref, cur, mv, q, c, sq = _discriminating()
    assert (q != sq).any(axis=1).sum() >= 1
    gq, gc = engine.refine_qpel(ref, cur, 16, mv, "satd")
    np.testing.assert_array_equal(gq, q)
    np.testing.assert_array_equal(gc, c)
    # and the SAD call of the same context is still the SAD oracle's
    np.testing.assert_array_equal(engine.refine_qpel(ref, cur, 16, mv, "sad")[0], sq)


def test_flat_frames_keep_the_integer_vector(engine):
    flat = np.full((40, 50), 93, np.uint8)
    rng = np.random.default_rng(41)
    for blk in (5, 16, 64):
        mv = rng.integers(-40, 41, (me.num_blocks(50, 40, blk), 2)).astype(np.int16)
        q, c = engine.refine_qpel(flat, flat, blk, mv, "satd")
        np.testing.assert_array_equal(q, 4 * mv)
        assert not c.any()


# ---------------------------------------------------------- device entry
def test_device_entry_with_pitch(engine):
    """Width 100 in rows of 112 bytes; the pad columns hold other data.  With
    and without a cost array, out of place and in place."""
    import torch
    w, h, blk, pitch = 100, 40, 16, 112
    rng = np.random.default_rng(31)
    big_r = rng.integers(0, 256, (h, pitch)).astype(np.uint8)
    big_c = rng.integers(0, 256, (h, pitch)).astype(np.uint8)
    ref, cur = big_r[:, :w].copy(), big_c[:, :w].copy()
    n = me.num_blocks(w, h, blk)
    rt, ct = torch.from_numpy(big_r).cuda(), torch.from_numpy(big_c).cuda()
    for k in FIELDS:
        mv = _field(k, ref, cur, blk, 32)
        oq, oc = S.refine(ref, cur, blk, mv)
        mvt = torch.from_numpy(mv.copy()).cuda()
        qt = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
        cot = torch.zeros(n, dtype=torch.int32, device="cuda")
        engine.refine_qpel_device(rt, ct, blk, "satd", mvt, qt, cot, width=w, height=h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(qt.cpu().numpy(), oq, err_msg=k)
        np.testing.assert_array_equal(_u32(cot), oc, err_msg=k)
        np.testing.assert_array_equal(mvt.cpu().numpy(), mv)  # the input field is untouched
        qt.zero_()
        engine.refine_qpel_device(rt, ct, blk, "satd", mvt, qt, None, width=w, height=h)
        engine.refine_qpel_device(rt, ct, blk, "satd", mvt, None, None, width=w, height=h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(qt.cpu().numpy(), oq, err_msg=k)
        np.testing.assert_array_equal(mvt.cpu().numpy(), oq, err_msg=k)
    engine.device_check()


def test_batch_in_place(engine):
    """Three frames at B = 32 whose strides exceed a frame, refined in place."""
    import torch
    w, h, pitch, rows, blk = 90, 70, 96, 75, 32
    rng = np.random.default_rng(51)
    big_r = rng.integers(0, 256, (3, rows, pitch)).astype(np.uint8)
    big_c = rng.integers(0, 256, (3, rows + 2, pitch)).astype(np.uint8)
    n = me.num_blocks(w, h, blk)
    mv = rng.integers(-9, 10, (3 * n, 2)).astype(np.int16)
    rt = torch.from_numpy(big_r).cuda()[:, :h]
    ct = torch.from_numpy(big_c).cuda()[:, :h]
    mvt = torch.from_numpy(mv.copy()).cuda()
    cot = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    engine.refine_qpel_device(rt, ct, blk, "satd", mvt, None, cot, width=w, height=h)
    torch.cuda.synchronize()
    got_q, got_c = mvt.cpu().numpy(), _u32(cot)
    for f in range(3):
        oq, oc = S.refine(big_r[f, :h, :w], big_c[f, :h, :w], blk, mv[f * n:(f + 1) * n])
        np.testing.assert_array_equal(got_q[f * n:(f + 1) * n], oq)
        np.testing.assert_array_equal(got_c[f * n:(f + 1) * n], oc)
    engine.device_check()


def test_captured_without_warm_up():
    """The first call of a fresh context is the captured one: the SATD kernels
    use no context scratch.  Replayed once, on new frame contents."""
    import torch
    ref, cur, mv, q, c, _ = _discriminating()
    s, sh = _stream()
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(s):
        rt = torch.zeros((64, 96), dtype=torch.uint8, device="cuda")
        ct = torch.zeros_like(rt)
        mvt = torch.zeros((24, 2), dtype=torch.int16, device="cuda")
        qt = torch.zeros_like(mvt)
        cot = torch.zeros(24, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: eng.refine_qpel_device(rt, ct, 16, "satd", mvt, qt, cot,
                                                           stream=sh))
        for t, a in ((rt, ref), (ct, cur), (mvt, mv)):
            t.copy_(torch.from_numpy(np.array(a)))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        np.testing.assert_array_equal(qt.cpu().numpy(), q)
        np.testing.assert_array_equal(_u32(cot), c)


# ------------------------------------------- rate-constrained refinement
@pytest.mark.parametrize("w,h,blk", [(33, 17, 16), (130, 75, 8), (70, 40, 32), (23, 17, 5),
                                     (50, 40, 64)])
def test_rate_constrained_refinement(engine, w, h, blk):
    ref, cur = _frames("random", w, h, 60 + w)
    rng = np.random.default_rng(61)
    n = me.num_blocks(w, h, blk)
    mv = _field("inframe", ref, cur, blk, 62)
    plain = engine.refine_qpel(ref, cur, blk, mv, "satd")
    preds = {"null": None, "near": plain[0],
             "random": rng.integers(-32768, 32768, (n, 2)).astype(np.int16)}
    for name, pred in preds.items():
        for lam in (0, 16, 1 << 24):
            got = engine.refine_qpel_rd(ref, cur, blk, mv, lam, pred, "satd")
            _equal(got, S.refine_rd(ref, cur, blk, mv, lam, pred), f"{w}x{h} B{blk} {name} {lam}")
            if lam == 0:  # the plain SATD refinement bit for bit, whatever the predictor
                _equal(got, (plain[0], plain[1], plain[1]), f"{name} lambda 0")


def test_rate_constrained_device_entry(engine):
    import torch
    ref, cur, mv, q, _, _ = _discriminating()
    rng = np.random.default_rng(63)
    pred = rng.integers(-60, 61, (24, 2)).astype(np.int16)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    rt, ct, mvt, pt = t(ref), t(cur), t(mv), t(pred)
    jt = torch.zeros(24, dtype=torch.int32, device="cuda")
    dt = torch.zeros(24, dtype=torch.int32, device="cuda")
    engine.refine_qpel_rd_device(rt, ct, 16, "satd", 16, mvt, None, jt, dt, pt)
    torch.cuda.synchronize()
    _equal((mvt.cpu().numpy(), _u32(jt), _u32(dt)), S.refine_rd(ref, cur, 16, mv, 16, pred))
    engine.device_check()


# ----------------------------------------------------------- bi-prediction
def _limit_field(n, rng):
    """Quarter-pel vectors at the int16 limits of the entry point and near 0."""
    q = rng.integers(-9, 10, (n, 2)).astype(np.int16)
    lim = _lib.ME_BIPRED_MAX_Q
    ends = np.array([(lim, -lim), (-lim, lim), (lim, lim), (-lim, -lim), (lim, 0)], np.int16)
    q[::3] = ends[np.arange(len(q[::3])) % len(ends)]
    return q


@pytest.mark.parametrize("w,h,blk", BIPRED_SHAPES)
def test_bipred_parity(engine, w, h, blk):
    rng = np.random.default_rng(200 + w)
    n = me.num_blocks(w, h, blk)
    ref0, cur = _frames("random", w, h, 70 + w)
    ref1, _ = _frames("checker3", w, h, 71)
    # cur near the average of two displaced references, so every mode occurs
    near = lambda: rng.integers(-9, 10, (n, 2)).astype(np.int16)
    qa, qb = near(), near()
    mix = (Q.compensate(ref0, blk, qa).astype(np.int64) + Q.compensate(ref1, blk, qb) + 1) >> 1
    pick = (np.arange(n) % 3)[Q._Frame(ref0, blk).bidx]
    planted = np.where(pick == 0, Q.compensate(ref0, blk, qa),
                       np.where(pick == 1, Q.compensate(ref1, blk, qb), mix))
    planted = np.clip(planted + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    jit = lambda q: (q + rng.integers(-1, 2, (n, 2))).astype(np.int16)
    cases = [("planted", planted, jit(qa), jit(qb)), ("random", cur, near(), near()),
             ("limits", cur, _limit_field(n, rng), _limit_field(n, rng)[::-1].copy())]
    modes = set()
    for name, c, q0, q1 in cases:
        for refine in (0, 1):
            want = S.bipred(ref0, ref1, c, blk, q0, q1, refine)
            modes |= set(want[2].tolist())
            got = engine.bipred(ref0, ref1, c, blk, q0, q1, "satd", refine)
            _equal(got, want, f"{w}x{h} B{blk} {name} refine {refine}")
    if n >= 12:  # not vacuous: the oracle itself chooses every mode
        assert modes == {0, 1, 2}


def test_bipred_device_entry_in_place(engine):
    """Three frames at B = 32 in rows of 96 bytes, outputs in place; then out of
    place without the optional outputs."""
    import torch
    w, h, pitch, blk = 90, 70, 96, 32
    rng = np.random.default_rng(71)
    big = [rng.integers(0, 256, (3, rows, pitch)).astype(np.uint8) for rows in (75, 77, 72)]
    n = me.num_blocks(w, h, blk)
    q0 = rng.integers(-40, 41, (3 * n, 2)).astype(np.int16)
    q1 = rng.integers(-40, 41, (3 * n, 2)).astype(np.int16)
    r0t, r1t, ct = (torch.from_numpy(a).cuda()[:, :h] for a in big)
    want = [S.bipred(big[0][f, :h, :w], big[1][f, :h, :w], big[2][f, :h, :w], blk,
                     q0[f * n:(f + 1) * n], q1[f * n:(f + 1) * n], 1) for f in range(3)]
    want = [np.concatenate([wf[k] for wf in want]) for k in range(5)]
    a0, a1 = torch.from_numpy(q0.copy()).cuda(), torch.from_numpy(q1.copy()).cuda()
    mode = torch.full((3 * n,), 9, dtype=torch.uint8, device="cuda")
    cost_t = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    cost3_t = torch.zeros((3 * n, 3), dtype=torch.int32, device="cuda")
    engine.bipred_device(r0t, r1t, ct, blk, "satd", a0, a1, mode, None, None, cost_t, cost3_t,
                         width=w, height=h)
    torch.cuda.synchronize()
    _equal((a0.cpu().numpy(), a1.cpu().numpy(), mode.cpu().numpy(), _u32(cost_t), _u32(cost3_t)),
           want)
    i0, i1 = torch.from_numpy(q0.copy()).cuda(), torch.from_numpy(q1.copy()).cuda()
    o0, o1 = torch.zeros_like(i0), torch.zeros_like(i1)
    mode.fill_(9)
    engine.bipred_device(r0t, r1t, ct, blk, "satd", i0, i1, mode, o0, o1, None, None,
                         width=w, height=h)
    torch.cuda.synchronize()
    _equal((o0.cpu().numpy(), o1.cpu().numpy(), mode.cpu().numpy()), want[:3])
    np.testing.assert_array_equal(i0.cpu().numpy(), q0)
    engine.device_check()


# -------------------------------------------------------------- composites
def test_composites_equal_their_steps(engine):
    """Each composite with "satd" is its separate calls with SAD for the
    integer step, and the oracle's result."""
    w, h, blk, span = 176, 144, 16, 8
    ref0, cur = synth.frame_pair(w, h, 7, 2, -1)
    ref1, _ = synth.frame_pair(w, h, 8, -3, 2)
    n = me.num_blocks(w, h, blk)
    # search + refinement
    mv0, _ = engine.full_search(ref0, cur, blk, span, "sad")
    step = engine.refine_qpel(ref0, cur, blk, mv0, "satd")
    _equal(engine.full_search_qpel(ref0, cur, blk, span, "satd"), step, "full_search_qpel")
    _equal(step, S.refine(ref0, cur, blk, mv0), "refine_qpel")
    # rate-constrained search + refinement, one lambda and predictor
    rng = np.random.default_rng(81)
    pred = rng.integers(-40, 41, (n, 2)).astype(np.int16)
    for lam, p in ((16, pred), (0, None)):
        rmv = engine.rd_search(ref0, cur, blk, span, lam, p, "sad")[0]
        rstep = engine.refine_qpel_rd(ref0, cur, blk, rmv, lam, p, "satd")
        _equal(engine.full_search_rd_qpel(ref0, cur, blk, span, lam, p, "satd"), rstep[:2],
               f"full_search_rd_qpel lambda {lam}")
        _equal(rstep, S.refine_rd(ref0, cur, blk, rmv, lam, p), "refine_qpel_rd")
    # both searches, both refinements, bi-prediction
    mv1, _ = engine.full_search(ref1, cur, blk, span, "sad")
    q0, q1 = step[0], engine.refine_qpel(ref1, cur, blk, mv1, "satd")[0]
    bi = engine.bipred(ref0, ref1, cur, blk, q0, q1, "satd", True)
    _equal(engine.full_search_bipred(ref0, ref1, cur, blk, span, "satd"), bi[:4],
           "full_search_bipred")
    _equal(bi, S.bipred(ref0, ref1, cur, blk, q0, q1, 1), "bipred")
    engine.device_check()


# ------------------------------------------------------------------ errors
def test_errors(engine):
    import torch
    L, h = _lib.lib(), engine._h
    w, ht, blk = 64, 48, 16
    n = me.num_blocks(w, ht, blk)
    ref = np.zeros((ht, w), np.uint8)
    mv = np.zeros((n, 2), np.int16)

    def raises(status, fn, *a, **k):
        with pytest.raises(me.MEError) as ei:
            fn(*a, **k)
        assert ei.value.status == status, (ei.value.status, status)
        assert L.me_last_error(h), "me_last_error is empty"

    # a valid request the integer searches do not serve
    U = _lib.ME_EUNSUPPORTED
    raises(U, engine.full_search, ref, ref, blk, 4, "satd")
    raises(U, engine.partition_search, ref, ref, blk, 4, 0, "satd")
    raises(U, engine.rd_search, ref, ref, blk, 4, 16, None, "satd")
    raises(U, engine.partition_rd_search, ref, ref, blk, 4, 16, None, "satd")
    rt = torch.from_numpy(np.zeros((2, ht, w), np.uint8)).cuda()
    mvt = torch.zeros((2 * n, 2), dtype=torch.int16, device="cuda")
    raises(U, engine.search_batch_device, rt, 0, rt, 0, w, ht, blk, 4, "satd", 0, ht // blk, mvt)
    raises(U, engine.full_search_device, rt[0], rt[0], blk, 4, "satd", mvt)
    # a value outside 0..3 stays ME_EINVAL where SATD is served
    p = lambda a: a.ctypes.data
    q = np.zeros((n, 2), np.int16)
    md = np.zeros(n, np.uint8)
    for bad in (4, -1):
        for st in (L.me_refine_qpel(h, p(ref), p(ref), w, ht, w, blk, bad, p(mv), p(q), None),
                   L.me_refine_qpel_rd(h, p(ref), p(ref), w, ht, w, blk, bad, 16, None, p(mv), p(q),
                                       None, None),
                   L.me_bipred(h, p(ref), p(ref), p(ref), w, ht, w, blk, bad, 1, p(mv), p(mv), p(q),
                               p(q), p(md), None, None),
                   L.me_full_search_qpel(h, p(ref), p(ref), w, ht, w, blk, 4, bad, p(q), None),
                   L.me_full_search(h, p(ref), p(ref), w, ht, w, blk, 4, bad, p(q), None)):
            assert st == _lib.ME_EINVAL, (bad, st)
            assert L.me_last_error(h)
    # SSIM stays unsupported where it was
    raises(U, engine.refine_qpel, ref, ref, blk, mv, "ssim")
    raises(U, engine.bipred, ref, ref, ref, blk, mv, mv, "ssim")
    torch.cuda.synchronize()
    engine.device_check()
