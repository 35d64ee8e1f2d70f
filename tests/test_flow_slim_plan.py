"""The pruning flow launch's slim bound scratch and its plane loads, on the CPU.

In a launch with box-sum planes the bound phase of me_flow_kernel<16, 13, 144>
loads the plane rows it reads from the job's planes in global memory into
registers; the slot's bound scratch shrinks from FLOW_PRUNE_BYTES (four planes
of 77 x 32 bytes, minlb, the cur blocks' box sums) to FLOW_SLIM_BYTES (list,
verify flags, minlb, box sums), and more slots fit the LDS.  A launch without
planes keeps the layout it had.  bin/flow_slim_dump (tools/flow_slim_dump.cc)
compiles the planner file and me_geom.h alone; checked here:

  * the planner's numbers of both layouts at 1080p +-32,
  * no plane load of any width the flow plan accepts ends past its phase row
    (so none straddles the end of a job's plane bytes),
  * the byte offsets of the kernel's formula (flow_plane_byte, the function the
    kernel calls) against the LDS DMA layout they replace, written out here.

No GPU and no library load.
"""
import json
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(REPO, "bin", "flow_slim_dump")
B, S, QROWS = 16, 32, 77


@pytest.fixture(scope="module")
def dump():
    subprocess.run(["make", "-s", "-C", REPO, "-f", "tools.mk", "bin/flow_slim_dump"], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([DUMP, *map(str, args)], capture_output=True, text=True, timeout=120, check=True)
        return json.loads(r.stdout)
    return run


# ------------------------------------------------------------------ the planner
def test_1080p_slot_counts_of_both_layouts(dump):
    d = dump("plan", 1920, 1080, 1920, 16 * 68, 0)
    assert d["flow"] and d["prune"] == 1 and d["tb"] == 4 and d["pitch"] == 144
    flow_lds = d["lds_budget"] - 1024  # plan_flow's FLOW_LDS
    slot = d["tile_bytes"] + 4 * B * B
    assert slot == 12544 and d["ctl_bytes"] == 256
    # without planes: the parent's layout, unchanged
    assert d["prune_bytes"] == 4 * 77 * 32 + 320 * 4 + 64 == 11200
    assert slot + d["prune_bytes"] == 23744
    assert d["prune_slots"] == 6
    assert d["prune_lds"] == 6 * 23744 + 6 * 4 * 8 + 256 == 142912
    # with planes: list + verify flags + U_b (1,024), minlb (1,280), box sums of cur (64)
    assert d["slim_bytes"] == 1024 + 1280 + 64 == 2368
    want = min(16, (flow_lds - 16 * 4 * 8 - d["ctl_bytes"]) // (slot + d["slim_bytes"]))
    assert d["slim_slots"] == want == 10
    assert d["slim_lds"] == want * (slot + d["slim_bytes"]) + want * 4 * 8 + d["ctl_bytes"]
    assert d["slim_lds"] <= d["lds_budget"] and d["prune_lds"] <= d["lds_budget"]


@pytest.mark.parametrize("slots", [2, 3, 4, 6, 9, 12])
def test_flow_slots_override_caps_both_layouts(dump, slots):
    d = dump("plan", 1920, 1080, 1920, 16 * 68, slots)
    assert d["prune_slots"] == min(6, slots) and d["slim_slots"] == min(10, slots)
    assert d["slim_lds"] == d["slim_slots"] * (12544 + 2368 + 32) + 256
    assert d["prune_lds"] == d["prune_slots"] * (23744 + 32) + 256


def test_small_and_padded_frames_get_the_same_layouts(dump):
    for w, h, stride, rows in ((256, 64, 256, 128), (320, 136, 320, 180), (336, 136, 336, 180), (640, 440, 640, 56),
                               (320, 136, 384, 180)):
        d = dump("plan", w, h, stride, rows, 0)
        assert d["flow"] and d["prune"] == 1 and d["tb"] == 4, (w, h)
        assert (d["prune_slots"], d["slim_slots"]) == (6, 10), (w, h)


# --------------------------------------------------------------- no straddling
def test_no_plane_load_straddles_a_phase_row_at_any_width(dump):
    """16 c + 32 <= flow_plane_pitch(W) for the last tile column c of every
    width from 64 to 8192 that plan_flow accepts, lane by lane through the
    kernel's formula; the planner's check (which gates the layout) agrees."""
    d = dump("fit", 64, 8192)
    assert d["planned"] == len(range(64, 8193, 16))  # every W % 16 == 0
    assert d["slim"] == d["planned"] and d["bad"] == []


# ------------------------------------------------------ plane byte addressing
# name -> (W, H, r0, r1, ref_row0): one job each
ADDR_CASES = {
    "clamped_256x64": (256, 64, 0, 4, 0),          # every window clamped at the top and the bottom
    "bottom_h8_320x136": (320, 136, 0, 9, 0),       # H % 16 = 8: the last block row is not bounded
    "partial_tile_200x96": (200, 96, 0, 6, 0),      # 12 full blocks; the frame's last columns have no q
    "partial_tile_336x136": (336, 136, 0, 9, 0),    # 21 blocks: the last tile has one; padded plane pitch
    "padded_pitch_304x136": (304, 136, 0, 9, 0),    # (304 + 64) / 4 = 92 -> pitch 96
    "stripe_mid_640x440": (640, 440, 7, 19, 80),    # ref_row0 = 7 * 16 - 32 > 0, rows end 19 * 16 + 32
    "stripe_last_640x440": (640, 440, 19, 28, 272),  # down to the frame's last row
    "stripe_no_halo_640x440": (640, 440, 7, 19, 112),  # ref rows start at the stripe: windows start above them
}


def _dma_offsets(w, h, r0, r1, ref0, pitch, bys, ncols):
    """The LDS DMA layout the loads replace (the parent's stage_item_wave): LDS
    plane k, window row r, byte i of the slot <- phase row 4 (prow0 - ref_row0
    + r) + k of the job's planes, byte 16 c + i.  Signed offsets, per
    (by, c, r, k, i)."""
    by = np.array(bys, np.int64)[:, None, None, None, None]
    c = np.arange(ncols, dtype=np.int64)[None, :, None, None, None]
    r = np.arange(QROWS, dtype=np.int64)[None, None, :, None, None]
    k = np.arange(4, dtype=np.int64)[None, None, None, :, None]
    i = np.arange(32, dtype=np.int64)[None, None, None, None, :]
    return (4 * (by * B - S - ref0 + r) + k) * pitch + 16 * c + i


@pytest.mark.parametrize("name", list(ADDR_CASES))
def test_kernel_offsets_equal_the_dma_layout(dump, tmp_path, name):
    w, h, r0, r1, ref0 = ADDR_CASES[name]
    out = tmp_path / "addr.bin"
    d = dump("addr", w, h, r0, r1, ref0, out)
    pitch, nbytes, ncols, bys = d["pitch"], d["bytes"], d["ncols"], d["bys"]
    assert pitch % 16 == 0 and pitch >= (w + 64) // 4 and ncols == (w // B + 3) // 4
    rows_end = min(h, r1 * B + S)
    assert d["rows"] == rows_end - ref0 and nbytes == d["rows"] * 4 * pitch and nbytes < 2 ** 31
    assert bys == [y for y in range(r0, r1) if h - y * B >= B]
    got = np.fromfile(out, np.uint32).astype(np.int64)
    n2 = len(bys) * ncols * QROWS * 64
    step2 = got[:n2].reshape(len(bys), ncols, QROWS, 64)
    fold = got[n2:].reshape(len(bys), ncols, 20, 64)
    dma = _dma_offsets(w, h, r0, r1, ref0, pitch, bys, ncols)  # [by, c, r, k, i]
    lane = np.arange(64)
    b, k, m, y = lane >> 4, (lane >> 2) & 3, lane & 3, lane & 15

    def inside(off, size):  # what the buffer range check passes (the offsets are unsigned)
        return off + size <= nbytes

    # step 2: lane (b, k, m) reads the slot's plane k, row r, bytes 4 b + 4 m .. + 7
    want = dma[:, :, :, k, 4 * b + 4 * m]  # [by, c, r, lane]
    want_in = (want >= 0) & (want + 8 <= nbytes)
    assert np.array_equal(inside(step2, 8), want_in), name
    assert np.array_equal(step2[want_in], want[want_in]), name
    assert np.all(step2 % 4 == 0)
    # a load is wholly inside or wholly outside: never across the end
    assert not np.any((step2 < nbytes) & (step2 + 8 > nbytes)), name
    # the fold column: lane (b, y) reads plane 0, rows y + 4 n (<= 76 where used), bytes 4 b + 16 .. + 19
    for n in range(20):
        rr = y + 4 * n
        use = rr < QROWS
        wf = dma[:, :, np.minimum(rr, QROWS - 1), 0, 4 * b + 16]  # [by, c, lane]
        wf_in = (wf >= 0) & (wf + 4 <= nbytes)
        g = fold[:, :, n, :]
        assert np.array_equal(inside(g, 4)[:, :, use], wf_in[:, :, use]), (name, n)
        sel = wf_in & use[None, None, :]
        assert np.array_equal(g[sel], wf[sel]), (name, n)
    assert not np.any((fold < nbytes) & (fold + 4 > nbytes)), name
    # both states occur where the case says so
    if ref0 > r0 * B - S or rows_end < r1 * B + S:
        assert not want_in.all(), name
    assert want_in.any(), name
