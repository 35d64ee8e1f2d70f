"""The chain kernel's pre-bound, on the CPU: where it reads the cur blocks and
where its marker lies.

The wave that publishes an item forms minlb and the cur blocks' box sums of the
slot's NEXT item behind the publish (csrc/me_kernels.hip, flow_fill).  The
slot's cur area still belongs to the item in front, so the box sums come from
global memory: lane (block, sub-block row, sub-block column) loads four dwords
at flow_qcur_byte (csrc/me_geom.h, the function the kernel calls).  Checked
here through bin/flow_prebound_dump (tools/flow_prebound_dump.cc, me_geom.h
alone): the sums over those bytes are numpy's 4x4 box sums >> 4 of the cur
plane, and the offsets are those of the bytes the slot's cur DMA brings
(stage_item_part: granule d = row (d >> 4) & 15 of block d >> 8), written out
here; the marker word overlaps nothing else of the slim bound scratch, whose
size stays what it was.

No GPU and no library load.
"""
import json
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(REPO, "bin", "flow_prebound_dump")
B, TB = 16, 4


@pytest.fixture(scope="module")
def dump():
    subprocess.run(["make", "-s", "-C", REPO, "-f", "tools.mk", "bin/flow_prebound_dump"], check=True, timeout=300)

    def run(tmp, w, h, stride, r0, r1, cur_row0):
        out = os.path.join(str(tmp), "qcur.bin")
        r = subprocess.run([DUMP, *map(str, (w, h, stride, r0, r1, cur_row0, out))], capture_output=True, text=True,
                           timeout=120, check=True)
        return json.loads(r.stdout), np.fromfile(out, np.uint32)
    return run


# name -> (W, H, stride, r0, r1, cur_row0): one job each
CASES = {
    "whole_frame_320x136": (320, 136, 320, 0, 9, 0),       # top and bottom full rows; the h = 8 row is left out
    "whole_frame_1080p": (1920, 1080, 1920, 0, 68, 0),
    "stripe_mid_640x440": (640, 440, 640, 7, 19, 112),     # cur rows from the stripe's first block row
    "stripe_last_640x440": (640, 440, 640, 19, 28, 304),   # down to the frame's last full row
    "stripe_padded_stride": (320, 136, 384, 3, 8, 48),     # cur_row0 != 0 and a stride above the width
    "one_block_last_tile_336": (336, 136, 336, 0, 9, 0),   # 21 blocks: the last tile has one
    "one_block_last_tile_stripe": (336, 136, 352, 4, 8, 64),
    "top_row_only": (256, 64, 256, 0, 1, 0),
    "bottom_row_only": (256, 64, 256, 3, 4, 48),
}


@pytest.mark.parametrize("name", list(CASES))
def test_offsets_give_the_cur_blocks_box_sums(dump, tmp_path, name):
    w, h, stride, r0, r1, cur_row0 = CASES[name]
    d, got = dump(tmp_path, w, h, stride, r0, r1, cur_row0)
    nbx = w // B
    ncols, bys = d["ncols"], d["bys"]
    assert ncols == (nbx + TB - 1) // TB and bys == [y for y in range(r0, r1) if h - y * B >= B] and bys
    off = got.astype(np.int64).reshape(len(bys), ncols, 64, 4)
    # the job's cur plane as the caller holds it: frame rows cur_row0 .. of the stripe, rows of `stride` bytes
    rows = min(h, r1 * B) - cur_row0
    rng = np.random.default_rng(sum(map(ord, name)))
    frame = rng.integers(0, 256, (h, w), dtype=np.uint8)
    plane = rng.integers(0, 256, (rows, stride), dtype=np.uint8)  # (the padding holds noise)
    plane[:, :w] = frame[cur_row0:cur_row0 + rows]
    flat = plane.reshape(-1)
    lane = np.arange(64)
    b, sy, sx = lane >> 4, (lane >> 2) & 3, lane & 3
    for iy, by in enumerate(bys):
        for c in range(ncols):
            nb = min(TB, nbx - TB * c)
            o = off[iy, c]                      # [lane, r]
            live = b < nb
            assert np.all(o[~live] == 0xFFFFFFFF), (name, by, c)
            ol = o[live]
            assert np.all(ol % 4 == 0) and ol.min() >= 0 and ol.max() + 4 <= flat.size, (name, by, c)
            # the bytes the slot's cur DMA brings: LDS dword (b * 16 + row) * 4 + sx <- row `row` of block b
            row = 4 * sy[live, None] + np.arange(4)[None, :]
            dma = ((by * B - cur_row0) + row) * stride + (TB * c + b[live, None]) * B + 4 * sx[live, None]
            assert np.array_equal(ol, dma), (name, by, c)
            # box sums >> 4 over them against numpy's of the frame
            s = np.zeros(ol.shape[0], np.int64)
            for r in range(4):
                for k in range(4):
                    s += flat[ol[:, r] + k]
            x0 = (TB * c + b[live]) * B + 4 * sx[live]
            y0 = by * B + 4 * sy[live]
            want = np.array([frame[y:y + 4, x:x + 4].astype(np.int64).sum() for y, x in zip(y0, x0)])
            assert np.array_equal(s >> 4, want >> 4), (name, by, c)
    if "one_block" in name:
        assert min(TB, nbx - TB * (ncols - 1)) == 1
    if name.startswith("stripe"):
        assert cur_row0 > 0


def test_marker_overlaps_nothing_and_the_scratch_keeps_its_size(dump, tmp_path):
    d, _ = dump(tmp_path, 256, 64, 256, 0, 1, 0)
    areas = {"list": (0, d["list_bytes"]), "dead": (d["dead"], d["dead_bytes"]), "ub": (d["ub"], d["ub_bytes"]),
             "minlb": (d["minlb"], d["minlb_bytes"]), "qcur": (d["qcur"], d["qcur_bytes"])}
    m0, m1 = d["mark"], d["mark"] + d["mark_bytes"]
    assert 976 <= m0 and m1 <= 1024 and m0 % 4 == 0
    for name, (a, n) in areas.items():
        assert m1 <= a or a + n <= m0, (name, a, n, m0)
    # the areas themselves stay where they were
    assert areas == {"list": (0, 640), "dead": (640, 320), "ub": (960, 16), "minlb": (1024, 1280),
                     "qcur": (2304, 64)}
    assert d["slim_bytes"] == 2368
    # NONE, BUSY(item) and DONE(item) never coincide, and item 0's are not NONE
    assert d["none"] == 0 and d["busy7"] == 16 and d["done7"] == 17
    assert len({d["none"], d["busy7"], d["done7"]}) == 3
