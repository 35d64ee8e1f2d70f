"""The VALU search kernels over their plan and range envelope, bit for bit.

Every row of tests/valu_envelope_cases.py runs through me_full_search_device
on planes carved at the row's pitch and byte offsets from buffers this test
owns, and must equal the oracle (oracle/me_oracle.c, the restatement of the
reference's src/cpu/main.c:18-82) in every MV and every cost; SSD through the
oracle's float-MSE mode, as tests/test_gpu_fuzz.py compares it.
tests/test_valu_envelope_cover.py proves on the CPU which me_fast_kernel
instance and which plan features each row reaches; here the pointers' real
alignment class must be the one that proof planned with, and the kernel family
the search reports the one the row expects.  Rows marked `valu` run on a
context of their own set to ME_PATH_VALU; the process-wide path is left alone.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import motionestimation_amd as me
import valu_envelope_cases as V
from valu_envelope_cases import CASES, SAD

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
GUARD = 4  # rows of the parent buffer after a plane's last row
MV_SENTINEL, COST_SENTINEL = -32768, -559038737  # no search writes either


def _case_data(name):
    """(ref, cur, oracle mv, oracle cost) of a row."""
    c = V.BY_NAME[name]
    ref, cur, _ = V.frames(c)
    omv, oc, _ = O.full_search(ref, cur, c.blk, c.range, "sad" if c.cost == SAD else "mse", threads=NT)
    return ref, cur, omv, oc


def _plane(a, pitch, offset):
    """(parent, view): `a` as a (rows, width) view at byte `offset` and row
    pitch `pitch` of a parent of random non-zero bytes."""
    import torch
    rows, w = a.shape
    parent = torch.randint(1, 256, (offset + (rows + GUARD) * pitch,), dtype=torch.uint8, device="cuda")
    assert parent.data_ptr() % V.BASE_ALIGN == 0  # the offset alone decides the view's alignment
    view = parent[offset:].as_strided((rows, w), (pitch, 1))
    view.copy_(torch.from_numpy(a).cuda())
    return parent, view


@pytest.fixture(scope="module")
def valu_engine():
    with me.Engine(devices=[0]) as eng:
        eng.set_kernel_path("valu")
        yield eng


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_envelope_case_equals_oracle(engine, valu_engine, name):
    import torch
    c = V.BY_NAME[name]
    ref, cur, omv, oc = _case_data(name)
    rp, rt = _plane(ref, c.stride, c.ref_off)
    cp, ct = _plane(cur, c.stride, c.cur_off)
    assert V.align_class(c.stride, rt.data_ptr(), ct.data_ptr()) == c.align, "not the planned alignment class"
    n = c.nbx * c.nby
    assert n == len(oc)
    mv = torch.full((n, 2), MV_SENTINEL, dtype=torch.int16, device="cuda")
    co = torch.full((n,), COST_SENTINEL, dtype=torch.int32, device="cuda")
    eng = valu_engine if c.path == "valu" else engine
    eng.full_search_device(rt, ct, c.blk, c.range, c.cost_name, mv, co, width=c.width,
                           height=c.height, stride=c.stride)
    torch.cuda.synchronize()
    eng.device_check()
    assert eng.last_search_path() == c.expect_path, (eng.last_search_path(), c.expect_path)
    gmv, gco = mv.cpu().numpy(), co.cpu().numpy().view(np.uint32)
    unwritten = np.flatnonzero((gmv == MV_SENTINEL).any(axis=1) | (gco == np.uint32(COST_SENTINEL & 0xFFFFFFFF)))
    assert unwritten.size == 0, f"{name}: records never written: blocks {unwritten[:8]}"
    bad = np.flatnonzero((gmv != omv).any(axis=1) | (gco != oc))
    print(f"{name}: {n} blocks, {bad.size} differ")
    if bad.size:
        i = int(bad[0])
        raise AssertionError(
            f"{name}: {bad.size} of {n} blocks differ from the oracle; first block {i} "
            f"(bx {i % c.nbx}, by {i // c.nbx}): got mv {tuple(gmv[i])} cost {gco[i]}, "
            f"oracle mv {tuple(omv[i])} cost {oc[i]}")
