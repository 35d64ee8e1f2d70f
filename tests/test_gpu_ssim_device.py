"""SSIM through the device entry points (me_full_search_device, the stripe,
job-list and batch calls, captured graphs) on planes the caller owns.

The host entry points upload into the library's own planes (256-byte aligned,
pitch = width), so there launch_ssim's choices that depend on the caller's
pointers -- 16-byte staging through a buffer resource against the byte loop,
4-byte loads of the current blocks, stripes whose reference holds only the halo
rows, job lists sharing one scratch plane -- are decided by the width alone.
Here a plane is a view into a larger uint8 tensor of random non-zero bytes, at
a chosen byte offset and pitch, with GUARD rows after its last resident row:
whatever a kernel reads next to the frame is memory this test owns and not
zero, and every result is the oracle's on tight host copies -- score bits and
MVs on every block (every shape here has a positive best score on every block,
which the tests assert, so no block is left out of the MV comparison)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import motionestimation_amd as me
from motionestimation_amd import shard, synth

pytestmark = pytest.mark.gpu

NT = 16
GUARD = 16  # rows of the parent tensor after a plane's last resident row


@functools.lru_cache(maxsize=None)
def _pair(w, h, seed):
    ref, cur = synth.frame_pair(w, h, seed, 3, -2)
    ref.setflags(write=False)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def _oracle(w, h, seed, blk, span):
    """(mv, bits) of the whole frame, computed once and shared read-only."""
    mv, bits, _ = O.full_search(*_pair(w, h, seed), blk, span, "ssim", threads=NT)
    assert (bits.view(np.float32) > 0).all(), "a block without a positive score: its MV is undefined"
    mv.setflags(write=False)
    bits.setflags(write=False)
    return mv, bits


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared frames are read-only


def _plane(a, w, pitch, offset=0):
    """(parent, view): the rows `a` as a (rows, w) uint8 view at byte `offset`,
    row pitch `pitch`, of a parent of random non-zero bytes with GUARD rows to
    spare after the view's last row."""
    import torch
    rows = a.shape[0]
    parent = torch.randint(1, 256, (offset + (rows + GUARD) * pitch,), dtype=torch.uint8,
                           device="cuda")
    assert parent.data_ptr() % 256 == 0  # the offset alone decides the view's alignment
    view = parent[offset:].as_strided((rows, w), (pitch, 1))
    view.copy_(_dev(a))
    return parent, view


def _outputs(n):
    import torch
    return (torch.full((n, 2), -7, dtype=torch.int16, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda"))


def _equal(mv_t, co_t, omv, obits, msg):
    np.testing.assert_array_equal(co_t.cpu().numpy().view(np.uint32), obits, err_msg=msg)
    np.testing.assert_array_equal(mv_t.cpu().numpy(), omv, err_msg=msg)


# pitch, ref byte offset, cur byte offset (None: pitch = width)
ALIGNMENTS = [
    (None, 0, 0),   # tight
    (224, 0, 0),    # ref rows 16-byte aligned: buffer-resource staging
    (224, 16, 32),  # ... from offset bases
    (224, 4, 0),    # 16-byte staging off by the pointer, 4-byte current loads on
    (212, 0, 0),    # 16-byte staging off by the pitch, 4-byte current loads on
    (211, 0, 0),    # both off
    (224, 0, 1),    # 4-byte current loads off by the pointer alone
]


@pytest.mark.parametrize("pitch,ref_off,cur_off", ALIGNMENTS)
@pytest.mark.parametrize("w", [208, 200])
def test_ssim_device_pitch_and_pointer_alignment(engine, w, pitch, ref_off, cur_off):
    """16 x 16, S = 20, H = 108 (H % 16 = 12: the partial bottom row's plane;
    W = 200 adds the partial right column) from planes of every alignment class
    launch_ssim distinguishes."""
    import torch
    h, blk, span = 108, 16, 20
    ref, cur = _pair(w, h, 71)
    omv, obits = _oracle(w, h, 71, blk, span)
    pitch = pitch or w
    rp, rt = _plane(ref, w, pitch, ref_off)
    cp, ct = _plane(cur, w, pitch, cur_off)
    mv, co = _outputs(len(obits))
    engine.full_search_device(rt, ct, blk, span, "ssim", mv, co, width=w, height=h, stride=pitch)
    torch.cuda.synchronize()
    _equal(mv, co, omv, obits, f"{w}x{h} pitch {pitch} offsets {ref_off}/{cur_off}")
    engine.device_check()


@pytest.mark.parametrize("blk,span", [(8, 9), (12, 6)])
def test_ssim_device_float_kernels_unaligned(engine, blk, span):
    """The float kernels with the float2 statistics plane from an odd pitch and
    an odd base pointer."""
    import torch
    w, h, pitch = 200, 108, 211
    ref, cur = _pair(w, h, 72)
    omv, obits = _oracle(w, h, 72, blk, span)
    rp, rt = _plane(ref, w, pitch, 1)
    cp, ct = _plane(cur, w, pitch, 1)
    mv, co = _outputs(len(obits))
    engine.full_search_device(rt, ct, blk, span, "ssim", mv, co, width=w, height=h, stride=pitch)
    torch.cuda.synchronize()
    _equal(mv, co, omv, obits, f"B{blk} S{span}")
    assert engine.last_search_path() == "ssim"
    engine.device_check()


def _stripe_jobs(w, h, blk, span, ways, seed):
    """One job per stripe of shard.plan: tensors holding only the rows the
    stripe contract names (include/me.h), GUARD rows of the parent after them."""
    ref, cur = _pair(w, h, seed)
    jobs, keep = [], []
    for st in shard.plan(w, h, blk, span, ways):
        assert st.nblocks
        rp, rt = _plane(ref[st.ref_y0:st.ref_y1], w, w)
        cp, ct = _plane(cur[st.cur_y0:st.cur_y1], w, w)
        mv, co = _outputs(st.nblocks)
        jobs.append((rt, st.ref_y0, ct, st.cur_y0, st.row_begin, st.row_end, mv, co))
        keep += [rp, cp]
    return jobs, keep


@pytest.mark.parametrize("span", [20, 64])
@pytest.mark.parametrize("w", [200, 208])
def test_ssim_halo_only_stripes(engine, w, span):
    """Three stripes of a 108-row frame, each from tensors of its own rows only
    (W = 200: the matrix-core kernel's byte staging, whose rows end with the
    last candidate's patch; W = 208: its buffer resource, clipped at the
    resident bytes).  The concatenated stripes are the oracle's frame."""
    import torch
    h, blk = 108, 16
    omv, obits = _oracle(w, h, 73, blk, span)
    jobs, keep = _stripe_jobs(w, h, blk, span, 3, 73)
    for rt, r0, ct, c0, b0, b1, mv, co in jobs:
        engine.search_stripe_device(rt, r0, ct, c0, w, h, blk, span, "ssim", b0, b1, mv, co,
                                    stride=w)
    torch.cuda.synchronize()
    _equal(torch.cat([j[6] for j in jobs]), torch.cat([j[7] for j in jobs]), omv, obits,
           f"{w}x{h} S{span}")
    engine.device_check()


@pytest.mark.parametrize("w", [200, 208])
def test_ssim_stripe_job_list(engine, w):
    """The same stripes as one me_search_stripes_device call: jobs of different
    rows, hence statistics planes of different sizes, one after the other on
    the context's one scratch."""
    import torch
    h, blk, span = 108, 16, 20
    omv, obits = _oracle(w, h, 73, blk, span)
    jobs, keep = _stripe_jobs(w, h, blk, span, 3, 73)
    nbx = (w + blk - 1) // blk
    for _ in range(2):
        engine.search_stripes_device(w, h, blk, span, "ssim", jobs)
    torch.cuda.synchronize()
    for rt, r0, ct, c0, b0, b1, mv, co in jobs:
        _equal(mv, co, omv[b0 * nbx:b1 * nbx], obits[b0 * nbx:b1 * nbx], f"{w} rows {b0}:{b1}")
    engine.device_check()


def test_ssim_batch_of_frames(engine):
    """me_full_search_batch_device: three different frame pairs, padded pitch
    and a frame stride larger than a frame; records frame-major."""
    import torch
    F, w, h, blk, span, pitch = 3, 200, 108, 16, 20, 224
    ref_b = torch.randint(1, 256, (F, h + 24, pitch), dtype=torch.uint8, device="cuda")
    cur_b = torch.randint(1, 256, (F, h + 24, pitch), dtype=torch.uint8, device="cuda")
    for f in range(F):
        ref, cur = _pair(w, h, 80 + f)
        ref_b[f, :h, :w] = _dev(ref)
        cur_b[f, :h, :w] = _dev(cur)
    n = me.num_blocks(w, h, blk)
    mv, co = _outputs(F * n)
    engine.search_batch_device(ref_b, 0, cur_b, 0, w, h, blk, span, "ssim", 0, (h + blk - 1) // blk,
                               mv, co)
    torch.cuda.synchronize()
    for f in range(F):
        omv, obits = _oracle(w, h, 80 + f, blk, span)
        _equal(mv[f * n:(f + 1) * n], co[f * n:(f + 1) * n], omv, obits, f"frame {f}")
    engine.device_check()


def test_ssim_captured_stripe_and_graph_kernel_path():
    """An interior SSIM stripe captured once and replayed on inputs rewritten
    in place: each replay is the oracle's field for the inputs of that replay.
    The graph's set_kernel_path / last_search_path are its engine's."""
    import torch
    w, h, blk, span = 200, 108, 16, 20
    st = shard.plan(w, h, blk, span, 3)[1]
    b0, b1 = st.row_begin * st.nbx, st.row_end * st.nbx
    pairs = [_pair(w, h, 90), _pair(w, h, 91), _pair(w, h, 92)]
    want = [(_oracle(w, h, 90 + k, blk, span)[0][b0:b1], _oracle(w, h, 90 + k, blk, span)[1][b0:b1])
            for k in range(3)]
    s = torch.cuda.Stream()
    sh = ctypes.c_void_p(s.cuda_stream)
    with me.Engine(devices=[0]) as eng, torch.cuda.stream(s):
        rp, rt = _plane(pairs[0][0][st.ref_y0:st.ref_y1], w, w)
        cp, ct = _plane(pairs[0][1][st.cur_y0:st.cur_y1], w, w)
        mv, co = _outputs(st.nblocks)
        run = eng.prepared_stripe_search(rt, st.ref_y0, ct, st.cur_y0, w, h, blk, span, "ssim",
                                         st.row_begin, st.row_end, mv, co, stream=sh, stride=w)
        # never run: the capture would have to allocate the statistics planes
        with pytest.raises(me.MEError) as ei:
            eng.capture(sh, run)
        assert ei.value.status == me._lib.ME_EINVAL
        run()  # uncaptured first: sizes the scratch
        torch.cuda.synchronize()
        _equal(mv, co, *want[0], "uncaptured")
        assert eng.last_search_path() == "ssim_mfma"
        g = eng.capture(sh, run)
        for k in (1, 2):
            rt.copy_(_dev(pairs[k][0][st.ref_y0:st.ref_y1]))
            ct.copy_(_dev(pairs[k][1][st.cur_y0:st.cur_y1]))
            mv.fill_(-7)
            co.zero_()
            g.launch(sh)
            torch.cuda.synchronize()
            _equal(mv, co, *want[k], f"replay {k}")
        eng.device_check()
        # the graph's path calls reach the context (they once took the graph's
        # handle for it)
        assert g.last_search_path() == eng.last_search_path() == "ssim_mfma"
        with pytest.raises(me.MEError) as ei:
            g.set_kernel_path("no-such-path")
        assert ei.value.status == me._lib.ME_EINVAL
        g.set_kernel_path("valu")
        mvh, bits = eng.full_search(*pairs[0], blk, span, "ssim")
        assert g.last_search_path() == eng.last_search_path() == "ssim"
        np.testing.assert_array_equal(bits, _oracle(w, h, 90, blk, span)[1])
        np.testing.assert_array_equal(mvh, _oracle(w, h, 90, blk, span)[0])
        g.set_kernel_path(None)
        eng.full_search(*pairs[0], blk, span, "ssim")
        assert g.last_search_path() == eng.last_search_path() == "ssim_mfma"
        eng.device_check()


def test_ssim_scratch_reuse_across_searches():
    """One context, searches whose planes differ in size and format back to
    back: compact planes, float2 planes (8 x 8, and 16 x 16 past S = 64), the
    SSD prepass planes in the same scratch, and the first search again."""
    seq = [("ssim", 16, 64, 208, 124), ("ssim", 16, 3, 48, 40), ("ssim", 8, 60, 96, 80),
           ("ssim", 16, 65, 136, 100), ("ssd", 16, 32, 208, 124), ("ssim", 16, 64, 208, 124)]
    with me.Engine(devices=[0]) as eng:
        for cost, blk, span, w, h in seq:
            ref, cur = _pair(w, h, 74)
            mv, bits = eng.full_search(ref, cur, blk, span, cost)
            if cost == "ssim":
                omv, obits = _oracle(w, h, 74, blk, span)
            else:
                omv, obits, _ = O.full_search(ref, cur, blk, span, cost, threads=NT)
            msg = f"{cost} B{blk} S{span} {w}x{h}"
            np.testing.assert_array_equal(bits, obits, err_msg=msg)
            np.testing.assert_array_equal(mv, omv, err_msg=msg)
        eng.device_check()


@pytest.mark.parametrize("span", [3, 33, 64])
def test_ssim_kernel_path_ab(span):
    """16 x 16 on a 120 x 92 frame (partial right column and bottom row): the
    matrix-core kernel on 'auto', the float-chain kernels with a float2 plane
    on 'valu', the oracle's bits and MVs on both.  The path is this context's
    own, the process-wide one stays as it is."""
    w, h, blk = 120, 92, 16
    ref, cur = _pair(w, h, 75)
    omv, obits = _oracle(w, h, 75, blk, span)
    with me.Engine(devices=[0]) as eng:
        for path, want in (("auto", "ssim_mfma"), ("valu", "ssim"), ("auto", "ssim_mfma")):
            eng.set_kernel_path(path)
            mv, bits = eng.full_search(ref, cur, blk, span, "ssim")
            assert eng.last_search_path() == want, (path, eng.last_search_path())
            np.testing.assert_array_equal(bits, obits, err_msg=path)
            np.testing.assert_array_equal(mv, omv, err_msg=path)
        eng.device_check()
