#!/usr/bin/env python
"""The table of calls the C ABI refuses: tests/golden/api_args.json.

Run once on a GPU, against the library of the commit BEFORE the argument rules
moved to csrc/me_api_rules.cpp (ME_HIP_LIB names that build):

    ME_HIP_LIB=libme_hip_parent.so python tests/golden/make_api_args.py

For every case it records the entry point, the arguments, which pointers are
null, the status returned and the me_last_error text.  A case the library
accepts is dropped, not kept.  Every case below is written to be refused, so
the recording launches no kernel; every non-null pointer is a real buffer
(BUF bytes, far more than the 48x32 block-16 shape needs), the 2 GiB cases
included: they pass a large frame stride with small buffers.

tests/test_api_rules.py replays the table through oracle/api_rules_dump (the
rules alone, no GPU) and tests/test_gpu_api_rules.py through the built library.
Cases marked "loose" carry one of the frame-batch messages, whose two wordings
were merged: only their status is compared.

A record is one line of flat keys: the integers by argument name (fs_*: frame
strides; elem / elem_val / elem_arr: a vector component poked into vector
array elem_arr, mode_idx / mode_val a mode byte, pix_idx / pix_val a pixel),
"null": the null pointers' names, space separated ("f.x": member x of the
field struct, "job.x": of the last job), "ndev": the context's device count.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "api_args.json")
W, H, B = 48, 32, 16
FB = W * H           # bytes of a frame
BUF = 1 << 16
INTS = ("width height stride blk range cost n_frames refine r0 r1 ref_row0 cur_row0 num_blks "
        "n_jobs").split()
SIZES = ("fs_ref", "fs_cur", "fs_ref1")
DEFAULT = dict(width=W, height=H, stride=W, blk=B, range=4, cost=1, n_frames=1, refine=1, r0=0, r1=2,
               ref_row0=0, cur_row0=0, num_blks=6, n_jobs=2, fs_ref=FB, fs_cur=FB, fs_ref1=FB,
               **{"lambda": 4})
PART_MEMBERS = ("mv_2nx2n mv_2nxn mv_nx2n mv_nxn cost_2nx2n cost_2nxn cost_nx2n cost_nxn mode "
                "mode_cost").split()
RD_MEMBERS = "dist_2nx2n dist_2nxn dist_nx2n dist_nxn bits_2nx2n bits_2nxn bits_nx2n bits_nxn".split()


class PartFields(ctypes.Structure):
    _fields_ = [(m, ctypes.c_void_p) for m in PART_MEMBERS]


class PartRdFields(ctypes.Structure):
    _fields_ = [("f", PartFields)] + [(m, ctypes.c_void_p) for m in RD_MEMBERS]


class StripeJob(ctypes.Structure):
    _fields_ = [("ref", ctypes.c_void_p), ("ref_row0", ctypes.c_int), ("cur", ctypes.c_void_p),
                ("cur_row0", ctypes.c_int), ("r0", ctypes.c_int), ("r1", ctypes.c_int),
                ("mv", ctypes.c_void_p), ("cost", ctypes.c_void_p)]


# Entry point -> (arguments in C order after the context, required pointers,
# accepted costs, largest range, largest lambda).  "fields" is a me_part_fields
# (me_part_rd_fields for the partition_rd entry points), "stream" the NULL stream.
_S = "ref cur width height stride blk range cost"
_FR = "ref fs_ref cur fs_cur width height stride blk"
SPECS = {
    "me_full_search": (_S + " mv cost_out", "ref cur mv", (0, 1, 2), 1024, None),
    "me_full_search_device": (_S + " mv cost_out stream", "ref cur mv", (0, 1, 2), 1024, None),
    "me_full_search_stripe_device": ("ref ref_row0 cur cur_row0 width height stride blk range cost r0 r1 "
                                     "mv cost_out stream", "ref cur mv", (0, 1, 2), 1024, None),
    "me_full_search_batch_device": ("ref fs_ref ref_row0 cur fs_cur cur_row0 width height stride blk range "
                                    "cost r0 r1 n_frames mv cost_out stream", "ref cur mv", (0, 1, 2),
                                    1024, None),
    "me_search_stripes_device": ("width height stride blk range cost jobs n_jobs stream",
                                 "jobs job.ref job.cur job.mv", (0, 1, 2), 1024, None),
    "me_find_best_blocks": ("ref cur width height blk range blks num_blks", "ref cur blks", None, 1024,
                            None),
    "me_motion_compensate": ("ref width height blk mv out", "ref mv out", None, None, None),
    "me_compensate_planes": ("ref cur width height blk mv out psnr", "ref cur mv out", None, None, None),
    "me_motion_compensate_qpel": ("ref width height blk mv out", "ref mv out", None, None, None),
    "me_compensate_planes_qpel": ("ref cur width height blk mv out psnr", "ref cur mv out", None, None,
                                  None),
    "me_refine_qpel_device": (_FR + " cost n_frames mv mv_q cost_out stream", "ref cur mv mv_q",
                              (0, 1, 3), None, None),
    "me_refine_qpel": ("ref cur width height stride blk cost mv mv_q cost_out", "ref cur mv mv_q",
                       (0, 1, 3), None, None),
    "me_full_search_qpel": (_S + " mv_q cost_out", "ref cur mv_q", (0, 1, 3), 1024, None),
    "me_bipred_device": ("ref fs_ref ref1 fs_ref1 cur fs_cur width height stride blk cost refine n_frames "
                         "mv q1 out0 out1 mode cost_out cost3 stream", "ref ref1 cur mv q1 out0 out1 mode",
                         (0, 1, 3), None, None),
    "me_bipred": ("ref ref1 cur width height stride blk cost refine mv q1 out0 out1 mode cost_out cost3",
                  "ref ref1 cur mv q1 out0 out1 mode", (0, 1, 3), None, None),
    "me_full_search_bipred": ("ref ref1 cur width height stride blk range cost out0 out1 mode cost_out",
                              "ref ref1 cur out0 out1 mode", (0, 1, 3), 1024, None),
    "me_motion_compensate_bipred": ("ref ref1 width height blk mv q1 mode out", "ref ref1 mv q1 mode out",
                                    None, None, None),
    "me_compensate_planes_bipred": ("ref ref1 cur width height blk mv q1 mode out psnr",
                                    "ref ref1 cur mv q1 mode out", None, None, None),
    "me_partition_search_device": (_FR + " range cost lambda n_frames fields stream",
                                   "ref cur fields f.mv_2nx2n f.mv_2nxn f.mv_nx2n f.mv_nxn f.mode", (1,),
                                   128, 1 << 24),
    "me_partition_search": (_S + " lambda fields",
                            "ref cur fields f.mv_2nx2n f.mv_2nxn f.mv_nx2n f.mv_nxn f.mode", (1,), 128,
                            1 << 24),
    "me_partition_leaf_field_device": ("width height blk n_frames fields leaf stream",
                                       "fields leaf f.mv_2nx2n f.mv_2nxn f.mv_nx2n f.mv_nxn f.mode", None,
                                       None, None),
    "me_rd_search_device": (_FR + " range cost lambda n_frames pred mv cost_out dist bits stream",
                            "ref cur mv cost_out", (1,), 128, 1 << 24),
    "me_rd_search": (_S + " lambda pred mv cost_out dist bits", "ref cur mv cost_out", (1,), 128, 1 << 24),
    "me_refine_qpel_rd_device": (_FR + " cost lambda n_frames pred mv mv_q cost_out dist stream",
                                 "ref cur mv mv_q", (0, 1, 3), None, 1 << 24),
    "me_refine_qpel_rd": ("ref cur width height stride blk cost lambda pred mv mv_q cost_out dist",
                          "ref cur mv mv_q", (0, 1, 3), None, 1 << 24),
    "me_full_search_rd_qpel": (_S + " lambda pred mv_q cost_out", "ref cur mv_q", (1, 3), 128, 1 << 24),
    "me_partition_rd_search_device": (_FR + " range cost lambda n_frames pred fields stream",
                                      "ref cur fields f.mv_2nx2n f.mv_2nxn f.mv_nx2n f.mv_nxn f.mode",
                                      (1,), 128, 1 << 23),
    "me_partition_rd_search": (_S + " lambda pred fields",
                               "ref cur fields f.mv_2nx2n f.mv_2nxn f.mv_nx2n f.mv_nxn f.mode", (1,), 128,
                               1 << 23),
}
# Host entry points that check their vectors' components: (limit, vector arrays).
VECTORS = {"me_refine_qpel": (8000, 1), "me_refine_qpel_rd": (8000, 1), "me_bipred": (32766, 2)}
MODES = ("me_motion_compensate_bipred", "me_compensate_planes_bipred")


def args_of(fn):
    return SPECS[fn][0].split()


def violations(fn):
    """Name -> overrides: every rule of fn broken alone."""
    names, required, costs, max_range, max_lambda = SPECS[fn]
    names = names.split()
    v = {f"null_{p}": {"null": p} for p in required.split()}
    v.update({"width0": {"width": 0}, "height0": {"height": 0}, "blk0": {"blk": 0},
              "blk65": {"blk": 65}})
    if "stride" in names:
        v["stride47"] = {"stride": 47}
    if max_range:
        v.update({"range-1": {"range": -1}, "range_max+1": {"range": max_range + 1}})
    if max_lambda:
        v["lambda_max+1"] = {"lambda": max_lambda + 1}
    if costs:
        v.update({f"cost{k}": {"cost": k} for k in range(-1, 5) if k not in costs})
    if "n_frames" in names:
        v.update({"n_frames0": {"n_frames": 0}, "n_frames-1": {"n_frames": -1},
                  "n_frames4097": {"n_frames": 4097}})
    for fs in SIZES:
        if fs in names:
            v[f"{fs}_below_frame"] = {"n_frames": 2, fs: FB - 1}
            v[f"{fs}_stack_2GiB"] = {"n_frames": 2, fs: (1 << 31) - FB}
    if "r0" in names or "jobs" in names:
        v.update({"r0-1": {"r0": -1}, "r1_3": {"r1": 3}, "r0_above_r1": {"r0": 2, "r1": 1},
                  "ref_row0-1": {"ref_row0": -1}, "ref_row0_1": {"ref_row0": 1},
                  "cur_row0-1": {"cur_row0": -1}, "cur_row0_1": {"cur_row0": 1}})
    if "jobs" in names:
        v["n_jobs-1"] = {"n_jobs": -1}
    if "num_blks" in names:
        v.update({"num_blks5": {"num_blks": 5}, "pixel256": {"pix_idx": 7, "pix_val": 256},
                  "pixel-1": {"pix_idx": W * H - 1, "pix_val": -1}})
    if fn in VECTORS:
        lim, arrays = VECTORS[fn]
        for a in range(arrays):
            v[f"vec{a}_above"] = {"elem": 5, "elem_val": lim + 1, "elem_arr": a}
            v[f"vec{a}_below"] = {"elem": 2 * 6 - 1, "elem_val": -lim - 1, "elem_arr": a}
    if fn in MODES:
        v["mode3"] = {"mode_idx": 4, "mode_val": 3}
    return v


def _group(name):
    """The rule family a violation belongs to."""
    for g in ("null", "blk", "stride", "range", "lambda", "cost", "n_frames", "fs", "n_jobs"):
        if name.startswith(g):
            return g
    if name.startswith(("width", "height")):
        return "size"
    return "rows" if name.startswith(("r0", "r1", "ref_row0", "cur_row0")) else "elem"


# Two rules broken at once pin which is reported first: per entry point, the
# first pair of each of these family pairs (SSIM cost with a null output,
# n_frames 0 with stride < width, lambda too large with SSD cost, ...).
PAIRS = [{"cost", "null"}, {"n_frames", "stride"}, {"lambda", "cost"}, {"fs", "lambda"}, {"range", "cost"},
         {"blk", "rows"}, {"n_frames", "cost"}, {"fs", "cost"}, {"lambda", "null"}, {"rows", "cost"},
         {"blk", "range"}, {"elem", "cost"}]


def cases():
    out = []
    for fn in SPECS:
        v = violations(fn)
        for name, over in v.items():
            out.append(dict(name=f"{fn}:{name}", fn=fn, **over))
        if fn.startswith(("me_motion", "me_compensate")) and fn not in MODES:
            continue
        seen = []
        for (na, a), (nb, b) in itertools.combinations(v.items(), 2):
            groups = {_group(na), _group(nb)}
            if set(a) & set(b) or groups not in PAIRS or groups in seen:
                continue
            if any(n.startswith(("null_ref", "null_cur", "null_f.", "blk65", "n_frames-1", "range-1",
                                 "cost-1")) for n in (na, nb)):
                continue  # (the plainer member of each family stands for it)
            seen.append(groups)
            out.append(dict(name=f"{fn}:{na}+{nb}", fn=fn, **a, **b))
    return out


class Call:
    """The ctypes arguments of a case, with the buffers they point into kept alive.
    alloc(name, device, fresh) -> (object to keep, address) of a zeroed BUF-byte
    buffer; fresh: one of its own (the case writes into it)."""

    def __init__(self, case, alloc):
        fn = case["fn"]
        device = fn.endswith("_device")
        null = set(case.get("null", "").split())
        self.keep, self.argv = [], []
        fresh = any(k in case for k in ("elem", "mode_idx", "pix_idx"))

        def buf(name, dev=device):
            if name in null:
                return None
            obj, addr = alloc(name, dev, fresh and not dev)
            self.keep.append(obj)
            return addr

        for a in args_of(fn):
            if a in INTS:
                self.argv.append(ctypes.c_int(case.get(a, DEFAULT[a])))
            elif a in SIZES:
                self.argv.append(ctypes.c_size_t(case.get(a, DEFAULT[a])))
            elif a == "lambda":
                self.argv.append(ctypes.c_uint32(case.get(a, DEFAULT[a])))
            elif a == "stream":
                self.argv.append(ctypes.c_void_p(None))
            elif a == "psnr":
                self.keep.append(ctypes.c_double(0))
                self.argv.append(ctypes.byref(self.keep[-1]))
            elif a == "fields":
                rd = "partition_rd" in fn
                f = PartRdFields() if rd else PartFields()
                for m in PART_MEMBERS:
                    setattr(f.f if rd else f, m, buf("f." + m))
                for m in RD_MEMBERS if rd else ():
                    setattr(f, m, buf("f." + m))
                self.keep.append(f)
                self.argv.append(None if a in null else ctypes.byref(f))
            elif a == "jobs":
                n = max(case.get("n_jobs", DEFAULT["n_jobs"]), 1)
                jobs = (StripeJob * n)()
                for i in range(n):
                    last = i == n - 1  # the case's violation is the last job's
                    g = (lambda k: case.get(k, DEFAULT[k])) if last else DEFAULT.get
                    jobs[i] = StripeJob(buf("job.ref") if last else buf("ok.ref"), g("ref_row0"),
                                        buf("job.cur") if last else buf("ok.cur"), g("cur_row0"), g("r0"),
                                        g("r1"), buf("job.mv") if last else buf("ok.mv"), buf("ok.cost"))
                self.keep.append(jobs)
                self.argv.append(None if a in null else ctypes.cast(jobs, ctypes.c_void_p))
            else:  # a plane or a record array
                addr = buf(a)
                if addr is not None and not device:
                    self.poke(case, a, addr)
                self.argv.append(ctypes.c_void_p(addr))

    @staticmethod
    def poke(case, a, addr):
        arr = {"mv": 0, "q1": 1}.get(a)
        if "elem" in case and arr == case["elem_arr"]:
            ctypes.cast(addr, ctypes.POINTER(ctypes.c_int16))[case["elem"]] = case["elem_val"]
        if "mode_idx" in case and a == "mode":
            ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint8))[case["mode_idx"]] = case["mode_val"]
        if "pix_idx" in case and a == "cur" and case["fn"] == "me_find_best_blocks":
            ctypes.cast(addr, ctypes.POINTER(ctypes.c_int))[case["pix_idx"]] = case["pix_val"]


def allocator():
    """alloc() for Call: numpy host buffers, torch device buffers, one per name."""
    import numpy as np
    import torch
    cache = {}

    def alloc(name, device, fresh):
        if fresh or (name, device) not in cache:
            if device:
                t = torch.zeros(BUF, dtype=torch.uint8, device="cuda")
                made = t, t.data_ptr()
            else:
                a = np.zeros(BUF, dtype=np.uint8)
                made = a, a.ctypes.data
            if fresh:
                return made
            cache[name, device] = made
        return cache[name, device]
    return alloc


def run(lib, ctx, case, alloc):
    """(status, message) of the case's call on context ctx."""
    call = Call(case, alloc)
    status = getattr(lib, case["fn"])(ctypes.c_void_p(ctx), *call.argv)
    return status, (lib.me_last_error(ctypes.c_void_p(ctx)) or b"").decode()


def open_lib():
    """A handle of its own on the built library (the package's handle declares
    argument types; these calls pass ctypes objects as they are)."""
    import torch  # (before the library: both bring a HIP runtime, torch's goes first as in the package)
    torch.cuda.init()
    sys.path.insert(0, REPO)
    from motionestimation_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.me_last_error.restype = ctypes.c_char_p
    lib.me_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int]
    lib.me_destroy.argtypes = [ctypes.c_void_p]
    return lib


def load_table():
    """The records, with what the file leaves out: fn (the name's prefix), ndev 1, loose 0."""
    with open(TABLE) as f:
        return [dict(dict(fn=r["name"].split(":")[0], ndev=1, loose=0), **r) for r in json.load(f)["records"]]


def write_table(records):
    about = ("Calls the C ABI refuses, recorded from the library before its argument rules moved to "
             "csrc/me_api_rules.cpp (tests/golden/make_api_args.py says how). One record per line; the "
             "entry point is the name up to the colon.")
    lean = [{k: v for k, v in r.items() if k != "fn" and (k, v) not in (("ndev", 1), ("loose", 0))}
            for r in records]
    with open(TABLE, "w") as f:
        f.write(json.dumps({"about": about})[:-1] + ',\n"records": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in lean))
        f.write("\n]}\n")


def main() -> None:
    lib, alloc = open_lib(), allocator()
    ctx = ctypes.c_void_p()
    assert lib.me_create(ctypes.byref(ctx), None, 0) == 0, "me_create"
    records, dropped = [], []
    for case in cases():
        status, message = run(lib, ctx.value, case, alloc)
        if status == 0:
            dropped.append(case["name"])
            continue
        loose = message.startswith(("frame stride", "batch of"))
        records.append(dict(case, ndev=1, status=status, message=message, loose=int(loose)))
    lib.me_destroy(ctx)
    write_table(records)
    print(f"{len(records)} refused calls recorded, {len(dropped)} accepted and dropped: {dropped}")


if __name__ == "__main__":
    main()
