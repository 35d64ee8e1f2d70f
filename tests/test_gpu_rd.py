"""Rate-constrained search and refinement on the GPU against tests/rd_ref.py,
record for record (assert_array_equal throughout): the fast kernel's small
shapes and the generic kernel's (me_rd_kernel_variant names the kernel;
tests/test_rd_ref.py pins it per shape), lambda over its range on both sides of
the fast bound, predictors (none, zero, full-range, the field itself), ties and
saturation, lambda = 0 against the plain full search, batches on a caller's
stream, optional outputs, a captured call, the per-block rate / distortion
monotonicity, the Foreman table of DESIGN.md, the host entry points, the
refinement with its rate term, and rejected arguments."""
import ctypes
import functools

import numpy as np
import pytest

import motionestimation_amd as me
import oracle_lib as O
import rd_ref as R
from motionestimation_amd import _lib

pytestmark = pytest.mark.gpu

FAST, GENERIC = _lib.ME_RD_KERNEL_FAST, _lib.ME_RD_KERNEL_GENERIC
FAST_LAM = _lib.ME_RD_FAST_MAX_LAMBDA
FAST_LAMBDAS = [0, 1, 16, 4096, FAST_LAM]


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
def _table(w, h, seed, B, S):
    """The restatement's SAD table: it serves every lambda and predictor."""
    ref, cur = _case(w, h, seed)
    return R.sad_table(ref, cur, B, S)


def _want(w, h, seed, B, S, lam, pred=None):
    ref, cur = _case(w, h, seed)
    return R.search_frame(ref, cur, B, S, lam, pred, table=_table(w, h, seed, B, S))


def _pred(kind, w, h, seed, B, S):
    """none: a NULL pointer; zero; random: full-range int16 with both extremes;
    field: 4 x the lambda = 0 field (every block's predictor is its own best
    vector in quarter units)."""
    n = me.num_blocks(w, h, B)
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((n, 2), np.int16)
    if kind == "random":
        p = np.random.default_rng(seed + 100).integers(-32768, 32768, (n, 2)).astype(np.int16)
        p[0] = (32767, -32767)
        p[-1] = (-32767, 32767)
        p[n // 2] = (-32768, -32768)
        return p
    return (4 * _want(w, h, seed, B, S, 0)[0]).astype(np.int16)


def _t(a):
    """A device copy of a (possibly read-only) numpy array."""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _device(eng, ref, cur, B, S, lam, pred=None, width=None, stream=None, cost="sad",
            dist=True, bits=True):
    """Search (H, pitch) planes or [F, H, pitch] batches (numpy or torch) on
    the device; every record starts as a sentinel.  Returns numpy (mv, J, D, R)
    (D / R None when not asked for)."""
    import torch
    rt = ref if isinstance(ref, torch.Tensor) else _t(ref)
    ct = cur if isinstance(cur, torch.Tensor) else _t(cur)
    h, w = rt.shape[-2], width or rt.shape[-1]
    frames = rt.shape[0] if rt.dim() == 3 else 1
    n = frames * me.num_blocks(w, h, B)
    mv = torch.full((n, 2), -777, dtype=torch.int16, device="cuda")
    j = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d = torch.full((n,), -1, dtype=torch.int32, device="cuda") if dist else None
    r = torch.full((n,), 255, dtype=torch.uint8, device="cuda") if bits else None
    pt = _t(pred) if pred is not None else None
    torch.cuda.synchronize()
    eng.rd_search_device(rt, ct, B, S, lam, mv, j, d, r, pt, cost=cost, stream=stream, width=w)
    torch.cuda.synchronize()
    eng.device_check()
    u = lambda t: t.cpu().numpy().view(np.uint32) if t is not None else None
    return mv.cpu().numpy(), u(j), u(d), r.cpu().numpy() if r is not None else None


def _check(got, want, frame=0):
    n = len(want[0])
    sl = slice(frame * n, (frame + 1) * n)
    for g, w, what in zip(got, want, ("mv", "J", "D", "R")):
        if g is not None:
            np.testing.assert_array_equal(g[sl], w, err_msg=what)


def _run(eng, w, h, seed, B, S, lam, kind="random"):
    ref, cur = _case(w, h, seed)
    pred = _pred(kind, w, h, seed, B, S)
    _check(_device(eng, ref, cur, B, S, lam, pred), _want(w, h, seed, B, S, lam, pred))


# ---- the fast kernel
@pytest.mark.parametrize("lam", FAST_LAMBDAS)
@pytest.mark.parametrize("S", [0, 1, 7, 32, 64])
def test_fast_clamped_windows(engine, S, lam):
    """96x64: every block's window is clamped on some side."""
    assert me.rd_kernel_variant(96, 64, 96, 16, S, lam) == FAST
    _run(engine, 96, 64, 3, 16, S, lam)


@pytest.mark.parametrize("lam", FAST_LAMBDAS)
def test_fast_interior_blocks_and_short_tile(engine, lam):
    """160x112 at +-7: interior blocks with unclamped windows; 10 block columns
    are tiles of 4 + 4 + 2."""
    assert me.rd_kernel_variant(160, 112, 160, 16, 7, lam) == FAST
    _run(engine, 160, 112, 4, 16, 7, lam)


@pytest.mark.parametrize("lam", [16, FAST_LAM])
@pytest.mark.parametrize("w,h,S", [(96, 64, 48), (96, 64, 56), (160, 160, 64)])
def test_fast_large_ranges(engine, w, h, S, lam):
    """The ranges between the issue's: the kernel walks 6 or 10 dy rows per lane
    by the range (10 at 48 and 64, 6 at 56 and up to 32); 160x160 has blocks
    whose +-64 window is not clamped on any side."""
    assert me.rd_kernel_variant(w, h, w, 16, S, lam) == FAST
    _run(engine, w, h, 14, 16, S, lam)


@pytest.mark.parametrize("lam", FAST_LAMBDAS)
def test_fast_with_clipped_rim(engine, lam):
    """100x72 at pitch 100: the full-size blocks on the fast kernel, the
    clipped right column (4 wide) and bottom row (8 high) in the rim launch."""
    assert me.rd_kernel_variant(100, 72, 100, 16, 7, lam) == FAST
    _run(engine, 100, 72, 5, 16, 7, lam)


@pytest.mark.parametrize("lam", FAST_LAMBDAS)
def test_fast_row_pitch(engine, lam):
    """96x64 in rows of 128 bytes; the padding must not be read as pixels."""
    assert me.rd_kernel_variant(96, 64, 128, 16, 7, lam) == FAST
    ref, cur = _case(96, 64, 3)
    planes = []
    for a in (ref, cur):
        p = np.full((64, 128), 201, np.uint8)
        p[:, :96] = a
        planes.append(_t(p))
    pred = _pred("random", 96, 64, 3, 16, 7)
    _check(_device(engine, planes[0], planes[1], 16, 7, lam, pred, width=96),
           _want(96, 64, 3, 16, 7, lam, pred))


# ---- the generic kernel
GENERIC_SHAPES = [(90, 50, 16, 7), (40, 24, 8, 7), (70, 40, 32, 4), (23, 17, 5, 3),
                  (130, 70, 64, 2), (48, 32, 16, 128)]


@pytest.mark.parametrize("lam", [0, 16, 1 << 24])
@pytest.mark.parametrize("w,h,B,S", GENERIC_SHAPES)
def test_generic_shapes(engine, w, h, B, S, lam):
    assert me.rd_kernel_variant(w, h, w, B, S, lam) == GENERIC
    _run(engine, w, h, 6, B, S, lam)


@pytest.mark.parametrize("lam", [FAST_LAM + 1, 1 << 24])
@pytest.mark.parametrize("w,h,S", [(96, 64, 7), (100, 72, 7)])
def test_generic_above_the_fast_bound(engine, w, h, S, lam):
    assert me.rd_kernel_variant(w, h, w, 16, S, lam) == GENERIC
    _run(engine, w, h, 3 if w == 96 else 5, 16, S, lam)


# ---- predictors
@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (160, 112, 16, 7), (90, 50, 16, 7),
                                      (40, 24, 8, 7)])
@pytest.mark.parametrize("lam", [1, 16, 4096])
def test_predictors(engine, w, h, B, S, lam):
    ref, cur = _case(w, h, 7)
    none = _device(engine, ref, cur, B, S, lam, None)
    zero = _device(engine, ref, cur, B, S, lam, _pred("zero", w, h, 7, B, S))
    _check(none, _want(w, h, 7, B, S, lam, None))
    _check(zero, none)  # a NULL predictor is the zero predictor
    for kind in ("random", "field"):
        _run(engine, w, h, 7, B, S, lam, kind)
    # predicted by its own best vector, a block keeps it: R = 2, D = the full search's
    if lam == 1:
        f0 = _want(w, h, 7, B, S, 0)
        got = _device(engine, ref, cur, B, S, lam, _pred("field", w, h, 7, B, S))
        np.testing.assert_array_equal(got[0], f0[0])
        assert (got[3] == 2).all()


# ---- ties and saturation
@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (100, 72, 16, 7), (70, 40, 32, 4)])
def test_flat_frame(engine, w, h, B, S):
    flat = np.full((h, w), 93, np.uint8)
    # lambda > 0, zero predictor: every SAD is 0 and the zero vector is the cheapest to code
    mv, j, d, r = _device(engine, flat, flat, B, S, 5)
    assert (mv == 0).all() and (j == 10).all() and (d == 0).all() and (r == 2).all()
    _check((mv, j, d, r), R.search_frame(flat, flat, B, S, 5))
    # lambda = 0: everything ties, the full search's first raster candidate wins
    mv0, c0, _ = O.full_search(flat, flat, B, S, "sad")
    got = _device(engine, flat, flat, B, S, 0)
    np.testing.assert_array_equal(got[0], mv0)
    np.testing.assert_array_equal(got[1], c0)
    assert tuple(got[0][-1]) != (0, 0)


@pytest.mark.parametrize("w,h,lam", [(96, 64, 16), (100, 72, 16), (96, 64, FAST_LAM),
                                      (96, 64, 1 << 24)])
def test_saturation_with_a_far_predictor(engine, w, h, lam):
    """cur = 255 against ref = 0: every candidate's SAD is 65,280 (a full-size
    block), the largest a packed-u16 accumulator holds; a far predictor gives
    the longest codes on top."""
    ref, cur = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    n = me.num_blocks(w, h, 16)
    pred = np.tile(np.array([[32767, -32768]], np.int16), (n, 1))
    got = _device(engine, ref, cur, 16, 7, lam, pred)
    want = R.search_frame(ref, cur, 16, 7, lam, pred)
    _check(got, want)
    # block 0: |4 dx - 32,767| <= 32,767 codes in 31 bits, 4 dy + 32,768 >= 32,768 in 33
    assert got[2][0] == 65280 and got[3][0] == 31 + 33
    np.testing.assert_array_equal(got[1].astype(np.int64),
                                  got[2].astype(np.int64) + lam * got[3].astype(np.int64))


# ---- lambda = 0 is the plain full search on both kernels
@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (160, 112, 16, 7), (100, 72, 16, 7),
                                      (90, 50, 16, 7), (70, 40, 32, 4)])
def test_lambda_zero_is_the_engine_full_search(engine, w, h, B, S):
    ref, cur = _case(w, h, 8)
    mv, cost = engine.full_search(ref, cur, B, S, "sad")
    got = _device(engine, ref, cur, B, S, 0, _pred("random", w, h, 8, B, S))
    np.testing.assert_array_equal(got[0], mv)
    np.testing.assert_array_equal(got[1], cost)
    np.testing.assert_array_equal(got[2], cost)


# ---- batching: three frames, frame strides above a frame, a caller's stream
@pytest.mark.parametrize("w,h,S", [(96, 64, 7), (90, 50, 5)])
def test_batch_on_a_stream(engine, w, h, S):
    import torch
    pairs = [_case(w, h, 10 + f) for f in range(3)]
    rt = torch.full((3, h + 3, w), 17, dtype=torch.uint8, device="cuda")
    ct = torch.full((3, h + 5, w), 29, dtype=torch.uint8, device="cuda")
    for f, (r, c) in enumerate(pairs):
        rt[f, :h] = _t(r)
        ct[f, :h] = _t(c)
    n = me.num_blocks(w, h, 16)
    preds = [_pred("random", w, h, 10 + f, 16, S) for f in range(3)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    got = _device(engine, rt[:, :h], ct[:, :h], 16, S, 16, np.concatenate(preds),
                  stream=ctypes.c_void_p(st.cuda_stream))
    assert len(got[0]) == 3 * n
    for f in range(3):
        _check(got, _want(w, h, 10 + f, 16, S, 16, preds[f]), frame=f)


@pytest.mark.parametrize("w,h", [(96, 64), (90, 50)])
def test_null_dist_and_bits(engine, w, h):
    ref, cur = _case(w, h, 3)
    want = _want(w, h, 3, 16, 7, 16)
    for dist, bits in ((False, False), (True, False), (False, True)):
        got = _device(engine, ref, cur, 16, 7, 16, dist=dist, bits=bits)
        assert (got[2] is None) == (not dist) and (got[3] is None) == (not bits)
        _check(got, want)


# ---- captured call: no context scratch, so no warm-up call before capture
def test_captured_search():
    """The search (fast kernel, then the rim on the generic one) captured on a
    fresh context and replayed once on new contents."""
    import torch
    w, h = 100, 72
    ref0, cur0 = _case(w, h, 20)
    ref1, cur1 = _case(w, h, 21)
    n = me.num_blocks(w, h, 16)
    pred = _pred("random", w, h, 21, 16, 7)
    st = torch.cuda.Stream()
    sh = ctypes.c_void_p(st.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(st):
        rt, ct, pt = _t(ref0), _t(cur0), _t(pred)
        mv = torch.full((n, 2), -777, dtype=torch.int16, device="cuda")
        j = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        d = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        r = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = eng.capture(sh, lambda: eng.rd_search_device(rt, ct, 16, 7, 16, mv, j, d, r, pt,
                                                         stream=sh))
        rt.copy_(_t(ref1))
        ct.copy_(_t(cur1))
        g.launch(sh)
        torch.cuda.synchronize()
        eng.device_check()
        got = (mv.cpu().numpy(), j.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32),
               r.cpu().numpy())
        _check(got, _want(w, h, 21, 16, 7, 16, pred))


# ---- exact minimisers: per block R never rises and D never falls with lambda
@pytest.mark.parametrize("w,h,B,S", [(160, 112, 16, 7), (90, 50, 16, 7)])
def test_rate_distortion_monotone_on_the_device(engine, w, h, B, S):
    ref, cur = _case(w, h, 9)
    pred = _pred("random", w, h, 9, B, S)
    prev = None
    for lam in (0, 4, 64):
        _, _, d, r = _device(engine, ref, cur, B, S, lam, pred)
        if prev is not None:
            assert (r <= prev[1]).all() and (d >= prev[0]).all(), lam
        prev = (d, r)


# ---- Foreman 1 -> 2, 16x16, +-7, zero predictor: the table of DESIGN.md
FOREMAN = [(0, 290804, 3730, 125, 290804), (1, 290893, 3586, 129, 294479),
           (4, 291719, 3238, 156, 304671), (16, 294967, 2882, 187, 341079),
           (64, 321438, 2168, 250, 460190), (256, 472554, 1056, 367, 742890),
           (1 << 20, 565944, 792, 396, 831038136)]


def test_foreman_table(engine):
    ref, cur = O.load_frame("ForemanYF1"), O.load_frame("ForemanYF2")
    table = R.sad_table(ref, cur, 16, 7)
    rt, ct = _t(ref), _t(cur)
    for lam, *want in FOREMAN:
        got = _device(engine, rt, ct, 16, 7, lam)
        _check(got, R.search_frame(ref, cur, 16, 7, lam, table=table))
        assert R.summary(*got) == tuple(want), lam


# ---- host planes: the synchronous entry point equals the device one
@pytest.mark.parametrize("w,h,B,S,width", [(96, 64, 16, 7, None), (90, 50, 16, 7, None),
                                            (70, 40, 32, 4, None), (112, 64, 16, 7, 100)])
@pytest.mark.parametrize("kind", ["none", "random"])
def test_host_entry_point(engine, w, h, B, S, width, kind):
    ref, cur = _case(w, h, 7)
    fw = width or w
    pred = _pred(kind, fw, h, 7, B, S) if kind == "none" else \
        np.random.default_rng(1).integers(-32768, 32768, (me.num_blocks(fw, h, B), 2)).astype(np.int16)
    want = R.search_frame(ref[:, :fw], cur[:, :fw], B, S, 16, pred)
    _check(engine.rd_search(ref, cur, B, S, 16, pred, width=width), want)
    _check(_device(engine, ref, cur, B, S, 16, pred, width=width), want)


# ---- refinement with the rate term
REFINE_SHAPES = [(96, 64, 16), (40, 24, 8), (50, 30, 16)]


@functools.lru_cache(maxsize=None)
def _field(w, h, B):
    ref, cur = _case(w, h, 12)
    mv, _, _ = O.full_search(ref, cur, B, 4, "sad")
    mv.setflags(write=False)
    return mv


def _refine_device(eng, ref, cur, B, cost, lam, mv, pred):
    import torch
    n = len(mv)
    q = torch.full((n, 2), -777, dtype=torch.int16, device="cuda")
    j = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.refine_qpel_rd_device(_t(ref), _t(cur), B, cost, lam, _t(mv), q, j, d,
                              _t(pred) if pred is not None else None)
    torch.cuda.synchronize()
    eng.device_check()
    return q.cpu().numpy(), j.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("w,h,B", REFINE_SHAPES)
def test_refinement_at_lambda_zero_is_refine_qpel(engine, w, h, B, cost):
    ref, cur = _case(w, h, 12)
    mv = _field(w, h, B)
    q, c = engine.refine_qpel(ref, cur, B, mv, cost)
    pred = _pred("random", w, h, 12, B, 4)
    for got in (engine.refine_qpel_rd(ref, cur, B, mv, 0, pred, cost),
                _refine_device(engine, ref, cur, B, cost, 0, mv, pred)):
        np.testing.assert_array_equal(got[0], q)
        np.testing.assert_array_equal(got[1], c)
        np.testing.assert_array_equal(got[2], c)


@pytest.mark.parametrize("lam", [1, 16, 1 << 24])
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("w,h,B", REFINE_SHAPES)
def test_refinement_against_the_restatement(engine, w, h, B, cost, lam):
    ref, cur = _case(w, h, 12)
    mv = _field(w, h, B)
    near = (4 * mv + np.random.default_rng(2).integers(-6, 7, mv.shape)).astype(np.int16)
    for pred in (None, near, _pred("random", w, h, 12, B, 4)):
        want = R.refine(ref, cur, B, mv, lam, pred, cost)
        for got in (_refine_device(engine, ref, cur, B, cost, lam, mv, pred),
                    engine.refine_qpel_rd(ref, cur, B, mv, lam, pred, cost)):
            for g, w_, what in zip(got, want, ("q", "Jq", "D")):
                np.testing.assert_array_equal(g, w_, err_msg=what)


@pytest.mark.parametrize("w,h,B,S", [(96, 64, 16, 7), (100, 72, 16, 7), (40, 24, 8, 7)])
@pytest.mark.parametrize("lam", [0, 16])
def test_full_search_rd_qpel_is_the_two_steps_composed(engine, w, h, B, S, lam):
    ref, cur = _case(w, h, 13)
    pred = _pred("field", w, h, 13, B, S) + np.int16(3)
    mv, _, _, _ = engine.rd_search(ref, cur, B, S, lam, pred)
    q, j, _ = engine.refine_qpel_rd(ref, cur, B, mv, lam, pred, "sad")
    got = engine.full_search_rd_qpel(ref, cur, B, S, lam, pred)
    np.testing.assert_array_equal(got[0], q)
    np.testing.assert_array_equal(got[1], j)
    want = R.refine(ref, cur, B, _want(w, h, 13, B, S, lam, pred)[0], lam, pred, "sad")
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# ---- rejected arguments
@pytest.mark.parametrize("kw,status", [
    (dict(cost="ssd"), _lib.ME_EUNSUPPORTED),
    (dict(cost="ssim"), _lib.ME_EUNSUPPORTED),
    (dict(span=129), _lib.ME_EUNSUPPORTED),
    (dict(lam=(1 << 24) + 1), _lib.ME_EINVAL),
    (dict(span=-1), _lib.ME_EINVAL),
])
def test_rejected_arguments(engine, kw, status):
    import torch
    ref, cur = _case(96, 64, 3)
    a = dict(span=7, lam=16, cost="sad")
    a.update(kw)
    with pytest.raises(me.MEError) as e:
        engine.rd_search(ref, cur, 16, a["span"], a["lam"], cost=a["cost"])
    assert e.value.status == status
    with pytest.raises(me.MEError) as e:
        _device(engine, ref, cur, 16, a["span"], a["lam"], cost=a["cost"])
    assert e.value.status == status
    if "span" not in kw and a["cost"] == "sad":
        with pytest.raises(me.MEError) as e:
            engine.full_search_rd_qpel(ref, cur, 16, 7, a["lam"])
        assert e.value.status == status
        with pytest.raises(me.MEError) as e:
            engine.refine_qpel_rd(ref, cur, 16, np.zeros((24, 2), np.int16), a["lam"])
        assert e.value.status == status


def test_rejected_null_vectors_and_stripe_context(engine):
    import torch
    ref, cur = _case(96, 64, 3)
    rt, ct = _t(ref), _t(cur)
    n = me.num_blocks(96, 64, 16)
    mv = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
    j = torch.zeros((n,), dtype=torch.int32, device="cuda")
    s = _lib.lib().me_rd_search_device(engine._h, rt.data_ptr(), 0, ct.data_ptr(), 0, 96, 64, 96,
                                       16, 7, _lib.ME_COST_SAD, 16, 1, None, None, j.data_ptr(),
                                       None, None, None)
    assert s == _lib.ME_EINVAL
    s = _lib.lib().me_refine_qpel_rd_device(engine._h, rt.data_ptr(), 0, ct.data_ptr(), 0, 96, 64,
                                            96, 16, _lib.ME_COST_SAD, 16, 1, None, mv.data_ptr(),
                                            None, j.data_ptr(), None, None)
    assert s == _lib.ME_EINVAL
    # a context over repeated device ids searches in stripes: not offered
    with me.Engine(devices=[0, 0]) as two:
        with pytest.raises(me.MEError) as e:
            two.rd_search(ref, cur, 16, 7, 16)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.rd_search_device(rt, ct, 16, 7, 16, mv, j)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.refine_qpel_rd(ref, cur, 16, np.zeros((n, 2), np.int16), 16)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.refine_qpel_rd_device(rt, ct, 16, "sad", 16, mv, None, j)
        assert e.value.status == _lib.ME_EUNSUPPORTED
        with pytest.raises(me.MEError) as e:
            two.full_search_rd_qpel(ref, cur, 16, 7, 16)
        assert e.value.status == _lib.ME_EUNSUPPORTED
