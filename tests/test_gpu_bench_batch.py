"""GPU: exactly the launches bench.py times, against the oracle and the reference.

bench.py's headline step is F = 16 1080p frame pairs (bench.batch_frames: the
synthetic pair rolled 37 f columns) in ONE me_full_search_batch_device call
(one flow-kernel launch, src/cpu/main.c:151-157 replaced).  Here the same call
on the same frames must equal
  * the oracle restatement run live, frame by frame (SAD), and
  * the committed per-frame pins (tests/golden/bench_pins.json: SAD from the
    oracle, SSD from the unmodified reference's ref_dump).
The SSD leg (ssd_mfma: one band-walk matrix-core launch for the 16 frames,
plus the lean kernel's launch for their partial bottom block rows) and the 4K
stripe leg's batch are pinned the same way.
"""
import hashlib
import os

import numpy as np
import pytest

import bench
import oracle_lib as O
from motionestimation_amd import synth

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
F = 16


def _batch(cfg):
    return bench.batch_frames(*synth.named_pair(cfg), F)


def _search(engine, frames, blk, span, cost):
    import torch
    h, w = frames[0][0].shape
    nb = ((w + blk - 1) // blk) * ((h + blk - 1) // blk)
    ref_t = torch.from_numpy(np.stack([r for r, _ in frames])).cuda()
    cur_t = torch.from_numpy(np.stack([c for _, c in frames])).cuda()
    mv = torch.full((F * nb, 2), -7, dtype=torch.int16, device="cuda")
    co = torch.zeros(F * nb, dtype=torch.int32, device="cuda")
    run = engine.prepared_batch_search(ref_t, 0, cur_t, 0, w, h, blk, span, cost, 0,
                                       (h + blk - 1) // blk, mv, co)
    for _ in range(3):  # as the timed loop: the same buffers rewritten
        run()
    torch.cuda.synchronize()
    engine.device_check()
    return bench.batch_fields(mv, co, F)


def _hash(mv, co, w, h, blk, cost):
    return hashlib.sha256(bench.record_stream(mv, co, w, h, blk, cost)).hexdigest()


def test_headline_batch_1080p_sad_equals_oracle_every_frame(engine):
    frames = _batch("1080p")
    fields = _search(engine, frames, 16, 32, "sad")
    pins = bench.load_pins("1080p", 16, 32, "sad")
    assert len(pins) == F
    for f, ((r, c), (mv, co)) in enumerate(zip(frames, fields)):
        omv, oco, _ = O.full_search(r, c, 16, 32, "sad", threads=NT)
        np.testing.assert_array_equal(mv, omv, err_msg=f"frame {f} mv")
        np.testing.assert_array_equal(co, oco, err_msg=f"frame {f} sad")
        assert _hash(mv, co, 1920, 1080, 16, "sad") == pins[f], f"frame {f} pin"


def test_plain_run_is_the_headline_leg_and_dumps_the_pinned_fields(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: one JSON line
    with the headline figures and no other leg; --dump-outputs writes the last
    timed step's fields, which are the pinned ones of the 16-frame batch."""
    import json
    import subprocess
    import sys
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(O.REPO, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--ramp-ms", "5", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "candidates/s" and d["dtype"] == "u8"
    assert d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    cands = d["config"]["candidates_per_frame"] * F
    assert d["value"] == pytest.approx(cands / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["parity"] is True and list(d["parity_legs"]) == ["timed_step"]
    assert d["cpu_baseline"] is None
    for leg in ("single_frame", "ssd_mfma", "ssd_single_frame", "ssim", "stripe_4k", "host_stream"):
        assert leg not in d, leg
    assert sorted(p.name for p in out.iterdir()) == ["cost.npy", "mv.npy"]
    mv, co = np.load(out / "mv.npy"), np.load(out / "cost.npy")
    nb = d["config"]["blocks_per_frame"]
    assert mv.dtype == co.dtype == np.float32 and mv.shape == (F, nb, 2) and co.shape == (F, nb)
    pins = bench.load_pins("1080p", 16, 32, "sad")
    assert len(pins) == F
    for f in range(F):
        assert _hash(mv[f].astype(np.int16), co[f].astype(np.uint32), 1920, 1080, 16,
                     "sad") == pins[f], f"frame {f} pin"


@pytest.mark.parametrize("path,kernel", [("auto", "mfma_bandwalk"), ("lean", "mfma_bandwalk"),
                                         ("prepass", "mfma_prepass")])
def test_ssd_leg_batch_1080p_equals_reference_every_frame(engine, path, kernel):
    """The benched SSD launch (16 1080p frames) runs the band-walk kernel on
    the automatic path (its strips fill the CUs) and equals the reference."""
    import motionestimation_amd as me
    me.set_kernel_path(path)
    try:
        fields = _search(engine, _batch("1080p"), 16, 32, "ssd")
        assert me.last_search_path() == kernel, (path, me.last_search_path())
    finally:
        me.set_kernel_path("auto")
    pins = bench.load_pins("1080p", 16, 32, "ssd")
    assert len(pins) == F
    bad = [f for f, (mv, co) in enumerate(fields) if _hash(mv, co, 1920, 1080, 16, "ssd") != pins[f]]
    assert not bad, f"frames {bad} differ from the reference's fields"


@pytest.mark.slow
@pytest.mark.parametrize("cost,path", [("sad", "auto"), ("ssd", "auto"), ("ssd", "lean")])
def test_stripe_4k_batch_equals_pins(engine, cost, path):
    import motionestimation_amd as me
    pins = bench.load_pins("4k", 16, 64, cost)
    if not pins:
        pytest.skip("no 4K pins committed")
    me.set_kernel_path(path)
    try:
        fields = _search(engine, _batch("4k"), 16, 64, cost)
    finally:
        me.set_kernel_path("auto")
    bad = [f for f, (mv, co) in enumerate(fields[:len(pins)])
           if _hash(mv, co, 3840, 2160, 16, cost) != pins[f]]
    assert not bad, f"4K {cost} frames {bad} differ from their pins"
