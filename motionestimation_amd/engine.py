"""Host-side engine over libme_hip.so.

``Engine.full_search`` is the frame-level drop-in for the reference's dispatch
region (src/cpu/main.c:144-158): one call searches every block of the frame on
the GPU and returns the MV field plus per-block cost.  ``full_search_device``
works on HBM-resident torch tensors and enqueues on a stream (what bench.py
times); ``search_stripe_device`` is the per-rank unit of the row-stripe shard.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import ME_COST_SAD, ME_COST_SATD, ME_COST_SSD, ME_COST_SSIM, MEError, check

# "satd": the quarter-pel refinements, the bi-prediction and their composites
# (include/me.h "SATD cost"); every integer search rejects it
_COST = {"ssd": ME_COST_SSD, "mse": ME_COST_SSD, "sad": ME_COST_SAD, "ssim": ME_COST_SSIM,
         "satd": ME_COST_SATD,
         ME_COST_SSD: ME_COST_SSD, ME_COST_SAD: ME_COST_SAD, ME_COST_SSIM: ME_COST_SSIM,
         ME_COST_SATD: ME_COST_SATD}


def cost_code(cost) -> int:
    try:
        return _COST[cost]
    except KeyError:
        raise MEError(_lib.ME_EINVAL, f"unknown cost {cost!r}") from None


def num_blocks(width: int, height: int, blk: int) -> int:
    return int(_lib.lib().me_num_blocks(width, height, blk))


def candidate_count(width: int, height: int, blk: int, span: int) -> int:
    return int(_lib.lib().me_candidate_count(width, height, blk, span))


def plan_stripes(width: int, height: int, blk: int, span: int, shards: int) -> list:
    """Block-row boundaries [b0=0, ..., b_n=nby] balancing the kernels' cost
    model (me_plan_stripes, include/me.h): a block row costs
    nbx * (3 (2S+1) + ny), so a clipped edge row is discounted by a quarter of
    its candidate deficit, not all of it."""
    out = (ctypes.c_int * (shards + 1))()
    check(_lib.lib().me_plan_stripes(width, height, blk, span, shards, out))
    return list(out)


def partition_counts(width: int, height: int, blk: int) -> tuple:
    """Cells of the partition search's four grids (me_partition_counts):
    (2Nx2N, 2NxN, Nx2N, NxN)."""
    out = (ctypes.c_int * 4)()
    check(_lib.lib().me_partition_counts(width, height, blk, out))
    return tuple(out)


def partition_kernel_variant(width: int, height: int, stride: int, blk: int, span: int) -> int:
    """The kernel that takes the frame's full-size macroblocks
    (me_partition_kernel_variant): ME_PART_KERNEL_FAST, ME_PART_KERNEL_GENERIC,
    or -1 for arguments the search rejects."""
    return int(_lib.lib().me_partition_kernel_variant(width, height, stride, blk, span))


def mv_bits(v: int) -> int:
    """Code length of a vector component difference (me_mv_bits): the signed
    exp-Golomb length 2 floor(log2(2 |v| + 1)) + 1."""
    return int(_lib.lib().me_mv_bits(v))


def rd_kernel_variant(width: int, height: int, stride: int, blk: int, span: int, lam: int) -> int:
    """The kernel that takes the frame's full-size blocks in a rate-constrained
    search (me_rd_kernel_variant): ME_RD_KERNEL_FAST, ME_RD_KERNEL_GENERIC, or
    -1 for arguments the search rejects."""
    if not 0 <= lam < 1 << 32:
        return -1
    return int(_lib.lib().me_rd_kernel_variant(width, height, stride, blk, span, lam))


class PartFields(ctypes.Structure):
    """include/me.h me_part_fields."""
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("mv_2nx2n", "mv_2nxn", "mv_nx2n", "mv_nxn", "cost_2nx2n", "cost_2nxn",
                 "cost_nx2n", "cost_nxn", "mode", "mode_cost")]


class PartitionFields:
    """The records of a partition search: mv (four int16 [cells, 2] fields in
    the order 2Nx2N, 2NxN, Nx2N, NxN), cost (four uint32 [cells], or None),
    mode (uint8 per macroblock) and mode_cost (uint32 per macroblock, or None).
    numpy arrays from the host entry points, torch tensors ([F * cells, ...],
    frame-major) for the device ones."""

    def __init__(self, mv, cost, mode, mode_cost):
        self.mv, self.cost, self.mode, self.mode_cost = list(mv), cost, mode, mode_cost

    def struct(self) -> PartFields:
        ptr = (lambda a: a.ctypes.data) if isinstance(self.mode, np.ndarray) else \
            (lambda a: a.data_ptr())
        opt = lambda a: ptr(a) if a is not None else None
        cost = self.cost if self.cost is not None else [None] * 4
        return PartFields(*[ptr(a) for a in self.mv], *[opt(a) for a in cost], ptr(self.mode),
                          opt(self.mode_cost))

    @classmethod
    def host(cls, width: int, height: int, blk: int) -> "PartitionFields":
        n = partition_counts(width, height, blk)
        return cls([np.zeros((k, 2), np.int16) for k in n], [np.zeros(k, np.uint32) for k in n],
                   np.zeros(n[0], np.uint8), np.zeros(n[0], np.uint32))

    @classmethod
    def device(cls, width: int, height: int, blk: int, frames: int = 1, device="cuda"):
        import torch
        n = partition_counts(width, height, blk)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        return cls([z((frames * k, 2), torch.int16) for k in n],
                   [z((frames * k,), torch.int32) for k in n],
                   z((frames * n[0],), torch.uint8), z((frames * n[0],), torch.int32))

    def numpy(self) -> "PartitionFields":
        """Host copy of device fields (costs as uint32)."""
        u = lambda t: t.cpu().numpy().view(np.uint32)
        return PartitionFields([t.cpu().numpy() for t in self.mv],
                               [u(t) for t in self.cost] if self.cost is not None else None,
                               self.mode.cpu().numpy(),
                               u(self.mode_cost) if self.mode_cost is not None else None)


class PartRdFields(ctypes.Structure):
    """include/me.h me_part_rd_fields."""
    _fields_ = [("f", PartFields)] + [(n, ctypes.c_void_p) for n in
                                      ("dist_2nx2n", "dist_2nxn", "dist_nx2n", "dist_nxn",
                                       "bits_2nx2n", "bits_2nxn", "bits_nx2n", "bits_nxn")]


class PartitionRdFields(PartitionFields):
    """The records of a rate-constrained partition search: PartitionFields
    (cost = J per cell) plus dist (four uint32 [cells], the SADs, or None) and
    bits (four uint8 [cells], the rates, or None).  struct() is the
    me_part_fields inside, so the leaf-field calls take these fields as they
    are; rd_struct() is the whole me_part_rd_fields."""

    def __init__(self, mv, cost, mode, mode_cost, dist, bits):
        super().__init__(mv, cost, mode, mode_cost)
        self.dist, self.bits = dist, bits

    def rd_struct(self) -> PartRdFields:
        ptr = (lambda a: a.ctypes.data) if isinstance(self.mode, np.ndarray) else \
            (lambda a: a.data_ptr())
        opt = lambda a: ptr(a) if a is not None else None
        dist = self.dist if self.dist is not None else [None] * 4
        bits = self.bits if self.bits is not None else [None] * 4
        return PartRdFields(self.struct(), *[opt(a) for a in dist], *[opt(a) for a in bits])

    @classmethod
    def host(cls, width: int, height: int, blk: int) -> "PartitionRdFields":
        n = partition_counts(width, height, blk)
        return cls([np.zeros((k, 2), np.int16) for k in n], [np.zeros(k, np.uint32) for k in n],
                   np.zeros(n[0], np.uint8), np.zeros(n[0], np.uint32),
                   [np.zeros(k, np.uint32) for k in n], [np.zeros(k, np.uint8) for k in n])

    @classmethod
    def device(cls, width: int, height: int, blk: int, frames: int = 1, device="cuda"):
        import torch
        n = partition_counts(width, height, blk)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        return cls([z((frames * k, 2), torch.int16) for k in n],
                   [z((frames * k,), torch.int32) for k in n],
                   z((frames * n[0],), torch.uint8), z((frames * n[0],), torch.int32),
                   [z((frames * k,), torch.int32) for k in n],
                   [z((frames * k,), torch.uint8) for k in n])

    def numpy(self) -> "PartitionRdFields":
        """Host copy of device fields (costs and distortions as uint32)."""
        u = lambda t: t.cpu().numpy().view(np.uint32)
        return PartitionRdFields([t.cpu().numpy() for t in self.mv],
                                 [u(t) for t in self.cost] if self.cost is not None else None,
                                 self.mode.cpu().numpy(),
                                 u(self.mode_cost) if self.mode_cost is not None else None,
                                 [u(t) for t in self.dist] if self.dist is not None else None,
                                 [t.cpu().numpy() for t in self.bits]
                                 if self.bits is not None else None)


def partition_rd_kernel_variant(width: int, height: int, stride: int, blk: int, span: int,
                                lam: int) -> int:
    """The kernel that takes the frame's full-size macroblocks in a
    rate-constrained partition search (me_partition_rd_kernel_variant):
    ME_PART_KERNEL_FAST, ME_PART_KERNEL_GENERIC, or -1 for arguments the search
    rejects."""
    if not 0 <= lam < 1 << 32:
        return -1
    return int(_lib.lib().me_partition_rd_kernel_variant(width, height, stride, blk, span, lam))


def partition_leaf_field(width: int, height: int, blk: int, fields: PartitionFields):
    """The leaf field (int16 [nhx * nhy, 2], block size blk / 2) of one frame's
    host fields, on the host (me_partition_leaf_field: no context, no GPU)."""
    n = partition_counts(width, height, blk)
    f = PartitionFields([np.ascontiguousarray(a, np.int16) for a in fields.mv], None,
                        np.ascontiguousarray(fields.mode, np.uint8), None)
    for a, k in zip(f.mv, n):
        if a.size != 2 * k:
            raise MEError(_lib.ME_EINVAL, f"field of {a.size // 2} records for {k} cells")
    if f.mode.size != n[0]:
        raise MEError(_lib.ME_EINVAL, f"{f.mode.size} modes for {n[0]} macroblocks")
    leaf = np.zeros((n[3], 2), np.int16)
    st = f.struct()
    check(_lib.lib().me_partition_leaf_field(width, height, blk, ctypes.byref(st), _ptr(leaf)))
    return leaf


_PATH_CODES = {"auto": 0, "valu": 1, "tiles": 2, "lean": 3, "prepass": 4}


def set_kernel_path(path: str) -> None:
    """'auto': 16x16 and 8x8 SSD on the matrix cores (i8 MFMA; 16x16 with
    S <= 64 on the band-walk kernel when a launch's strips fill the CUs, else
    the prepass + block-major pair), the rest on the VALU kernels; 'valu':
    VALU kernels only (SSIM too: its float-chain kernels, where the other
    paths run 16x16 SSIM with S <= 64 on the matrix cores); 'tiles': as 'auto'
    with 16x16 SSD on the 4x4-block-tile MFMA kernel; 'lean': 16x16 SSD (S <= 64) on the band-walk kernel for every
    launch (no prepass planes, no scratch); 'prepass': 16x16 SSD on the S2
    prepass + block-major pair.  Process-wide; results are identical."""
    if path not in _PATH_CODES:
        raise MEError(_lib.ME_EINVAL, f"unknown kernel path {path!r}")
    _lib.lib().me_set_kernel_path(_PATH_CODES[path])


SEARCH_PATHS = {0: "none", 1: "valu", 2: "mfma_prepass", 3: "mfma_bandwalk", 4: "mfma_lean",
                5: "mfma_tiles", 6: "mfma_8x8", _lib.ME_SEARCH_PATH_SSIM: "ssim",
                _lib.ME_SEARCH_PATH_SSIM_MFMA: "ssim_mfma"}


def last_search_path() -> str:
    """The kernel family of the most recent search launched in this process
    (me_last_search_path): 'valu', 'mfma_prepass', 'mfma_bandwalk', ..."""
    return SEARCH_PATHS.get(_lib.lib().me_last_search_path(), "unknown")


def version() -> str:
    return _lib.lib().me_version().decode()


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


class Engine:
    """One context: device buffers, a HIP stream per device, RCCL comms when
    created over several distinct devices.  Use from one thread at a time."""

    def __init__(self, devices=None):
        L = _lib.lib()
        h = ctypes.c_void_p()
        if devices:
            ids = (ctypes.c_int * len(devices))(*devices)
            st = L.me_create(ctypes.byref(h), ids, len(devices))
        else:
            st = L.me_create(ctypes.byref(h), None, 0)
        check(st)
        self._h = h
        self.devices = list(devices) if devices else None
        self.comm_ranks = 0  # me_comm_init: size of this context's RCCL group

    def set_kernel_path(self, path) -> None:
        """This context's kernel path (me_ctx_set_kernel_path): one of
        set_kernel_path()'s names, or None to follow the process-wide path."""
        if path is not None and path not in _PATH_CODES:
            raise MEError(_lib.ME_EINVAL, f"unknown kernel path {path!r}")
        code = _lib.ME_PATH_PROCESS if path is None else _PATH_CODES[path]
        check(_lib.lib().me_ctx_set_kernel_path(self._h, code), self._h)

    def last_search_path(self, device_index: int = 0) -> str:
        """The kernel family of this context's latest search on its device
        `device_index` (me_ctx_last_search_path)."""
        return SEARCH_PATHS.get(_lib.lib().me_ctx_last_search_path(self._h, device_index), "unknown")

    def close(self) -> None:
        if getattr(self, "_h", None):
            for g in getattr(self, "_graphs", ()):
                g.close()
            _lib.lib().me_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------- host API
    def full_search(self, ref, cur, blk: int, span: int, cost="ssd", stride=None):
        """Search (H, W) uint8 planes.  Returns (mv int16 [nblocks, 2] as
        (mvx, mvy), cost uint32 [nblocks]) in the reference's raster order."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, w = ref.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        mv = np.zeros((max(n, 1), 2), np.int16)
        cst = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().me_full_search(self._h, _ptr(ref), _ptr(cur), w, h, stride or w, blk,
                                        span, cost_code(cost), _ptr(mv), _ptr(cst)), self._h)
        return mv[:n], cst[:n]

    def compensate_planes(self, ref, cur, blk: int, mv):
        """5-plane output [ref, cur, mc, |ref-cur|, |mc-cur|] (5H, W) and PSNR."""
        ref = np.ascontiguousarray(ref, np.uint8)
        cur = np.ascontiguousarray(cur, np.uint8)
        mv = np.ascontiguousarray(mv, np.int16)
        h, w = ref.shape
        out = np.zeros((5 * h, w), np.uint8)
        psnr = ctypes.c_double()
        check(_lib.lib().me_compensate_planes(self._h, _ptr(ref), _ptr(cur), w, h, blk,
                                              _ptr(mv), _ptr(out), ctypes.byref(psnr)), self._h)
        return out, psnr.value

    def motion_compensate(self, ref, blk: int, mv):
        ref = np.ascontiguousarray(ref, np.uint8)
        mv = np.ascontiguousarray(mv, np.int16)
        h, w = ref.shape
        mc = np.zeros_like(ref)
        check(_lib.lib().me_motion_compensate(self._h, _ptr(ref), w, h, blk, _ptr(mv),
                                              _ptr(mc)), self._h)
        return mc

    # ---- quarter-pel (include/me.h "quarter-pel refinement") ----
    def refine_qpel(self, ref, cur, blk: int, mv, cost="ssd", stride=None):
        """Refine the integer field mv [nblocks, 2] to quarter-pel on cost
        "ssd", "sad" or "satd".  Returns (mv_q int16 [nblocks, 2], four units
        per pixel, cost uint32 [nblocks])."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, w = ref.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        mv = np.ascontiguousarray(mv, np.int16)
        if mv.size != 2 * n:
            raise MEError(_lib.ME_EINVAL, f"mv of {mv.size // 2} records for {n} blocks")
        q = np.zeros((max(n, 1), 2), np.int16)
        cst = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().me_refine_qpel(self._h, _ptr(ref), _ptr(cur), w, h, stride or w, blk,
                                        cost_code(cost), _ptr(mv), _ptr(q), _ptr(cst)), self._h)
        return q[:n], cst[:n]

    def full_search_qpel(self, ref, cur, blk: int, span: int, cost="ssd", stride=None):
        """full_search and refine_qpel back to back on the device ("satd": the
        search at SAD, the refinement at SATD).  Returns
        (mv_q int16 [nblocks, 2] in quarter-pel units, cost uint32 [nblocks])."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, w = ref.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        q = np.zeros((max(n, 1), 2), np.int16)
        cst = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().me_full_search_qpel(self._h, _ptr(ref), _ptr(cur), w, h, stride or w, blk,
                                             span, cost_code(cost), _ptr(q), _ptr(cst)), self._h)
        return q[:n], cst[:n]

    def compensate_planes_qpel(self, ref, cur, blk: int, mv_q):
        """compensate_planes with quarter-pel vectors (edge-replicated samples)."""
        ref = np.ascontiguousarray(ref, np.uint8)
        cur = np.ascontiguousarray(cur, np.uint8)
        mv_q = np.ascontiguousarray(mv_q, np.int16)
        h, w = ref.shape
        out = np.zeros((5 * h, w), np.uint8)
        psnr = ctypes.c_double()
        check(_lib.lib().me_compensate_planes_qpel(self._h, _ptr(ref), _ptr(cur), w, h, blk,
                                                   _ptr(mv_q), _ptr(out), ctypes.byref(psnr)),
              self._h)
        return out, psnr.value

    def motion_compensate_qpel(self, ref, blk: int, mv_q):
        ref = np.ascontiguousarray(ref, np.uint8)
        mv_q = np.ascontiguousarray(mv_q, np.int16)
        h, w = ref.shape
        mc = np.zeros_like(ref)
        check(_lib.lib().me_motion_compensate_qpel(self._h, _ptr(ref), w, h, blk, _ptr(mv_q),
                                                   _ptr(mc)), self._h)
        return mc

    # ---- bi-prediction (include/me.h "bi-predictive mode decision") ----
    @staticmethod
    def _planes3(ref0, ref1, cur):
        ref0 = np.ascontiguousarray(ref0, dtype=np.uint8)
        ref1 = np.ascontiguousarray(ref1, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref0.ndim != 2 or ref0.shape != cur.shape or ref1.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL,
                          f"plane shapes {ref0.shape} / {ref1.shape} vs {cur.shape}")
        return ref0, ref1, cur

    @staticmethod
    def _field(mv, n, what):
        mv = np.ascontiguousarray(mv, np.int16)
        if mv.size != 2 * n:
            raise MEError(_lib.ME_EINVAL, f"{what} of {mv.size // 2} records for {n} blocks")
        return mv

    def bipred(self, ref0, ref1, cur, blk: int, mv_q0, mv_q1, cost="ssd", refine=True,
               stride=None):
        """Per block: the costs of ref0 at mv_q0, ref1 at mv_q1 and their
        rounded average (jointly refined by a quarter step with refine), and
        the cheapest mode.  Returns (mv0 int16 [nblocks, 2], mv1 int16
        [nblocks, 2], mode uint8 [nblocks] (ME_PRED_L0 / L1 / BI), cost uint32
        [nblocks], cost3 uint32 [nblocks, 3] = (c0, c1, cb))."""
        ref0, ref1, cur = self._planes3(ref0, ref1, cur)
        h, w = cur.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        q0, q1 = self._field(mv_q0, n, "mv_q0"), self._field(mv_q1, n, "mv_q1")
        m = max(n, 1)
        o0, o1 = np.zeros((m, 2), np.int16), np.zeros((m, 2), np.int16)
        mode, cst, c3 = np.zeros(m, np.uint8), np.zeros(m, np.uint32), np.zeros((m, 3), np.uint32)
        check(_lib.lib().me_bipred(self._h, _ptr(ref0), _ptr(ref1), _ptr(cur), w, h, stride or w,
                                   blk, cost_code(cost), int(bool(refine)), _ptr(q0), _ptr(q1),
                                   _ptr(o0), _ptr(o1), _ptr(mode), _ptr(cst), _ptr(c3)), self._h)
        return o0[:n], o1[:n], mode[:n], cst[:n], c3[:n]

    def full_search_bipred(self, ref0, ref1, cur, blk: int, span: int, cost="ssd", stride=None):
        """Both searches, both quarter-pel refinements and bipred(refine=True)
        back to back on the device.  Returns (mv0, mv1, mode, cost)."""
        ref0, ref1, cur = self._planes3(ref0, ref1, cur)
        h, w = cur.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        m = max(n, 1)
        o0, o1 = np.zeros((m, 2), np.int16), np.zeros((m, 2), np.int16)
        mode, cst = np.zeros(m, np.uint8), np.zeros(m, np.uint32)
        check(_lib.lib().me_full_search_bipred(self._h, _ptr(ref0), _ptr(ref1), _ptr(cur), w, h,
                                               stride or w, blk, span, cost_code(cost), _ptr(o0),
                                               _ptr(o1), _ptr(mode), _ptr(cst)), self._h)
        return o0[:n], o1[:n], mode[:n], cst[:n]

    def compensate_planes_bipred(self, ref0, ref1, cur, blk: int, mv0, mv1, mode):
        """compensate_planes_qpel with two references and a mode per block:
        [ref0, cur, mc, |ref0-cur|, |mc-cur|] (5H, W) and PSNR."""
        ref0, ref1, cur = self._planes3(ref0, ref1, cur)
        mv0, mv1 = np.ascontiguousarray(mv0, np.int16), np.ascontiguousarray(mv1, np.int16)
        mode = np.ascontiguousarray(mode, np.uint8)
        h, w = cur.shape
        out = np.zeros((5 * h, w), np.uint8)
        psnr = ctypes.c_double()
        check(_lib.lib().me_compensate_planes_bipred(
            self._h, _ptr(ref0), _ptr(ref1), _ptr(cur), w, h, blk, _ptr(mv0), _ptr(mv1),
            _ptr(mode), _ptr(out), ctypes.byref(psnr)), self._h)
        return out, psnr.value

    def motion_compensate_bipred(self, ref0, ref1, blk: int, mv0, mv1, mode):
        ref0, ref1, _ = self._planes3(ref0, ref1, ref0)
        mv0, mv1 = np.ascontiguousarray(mv0, np.int16), np.ascontiguousarray(mv1, np.int16)
        mode = np.ascontiguousarray(mode, np.uint8)
        h, w = ref0.shape
        mc = np.zeros_like(ref0)
        check(_lib.lib().me_motion_compensate_bipred(
            self._h, _ptr(ref0), _ptr(ref1), w, h, blk, _ptr(mv0), _ptr(mv1), _ptr(mode),
            _ptr(mc)), self._h)
        return mc

    # ---- partition search (include/me.h "partition search") ----
    def partition_search(self, ref, cur, blk: int, span: int, lam: int = 0, cost="sad",
                         width=None) -> "PartitionFields":
        """Best vector of every macroblock, of its halves and of its quarters,
        and the cheapest of the four shapes at Lagrangian weight lam
        (me_partition_search) on (H, pitch) uint8 planes; width (default: the
        pitch) names the frame's columns.  Returns PartitionFields of numpy
        arrays."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, pitch = ref.shape
        w = width or pitch
        out = PartitionFields.host(w, h, blk)
        st = out.struct()
        check(_lib.lib().me_partition_search(self._h, _ptr(ref), _ptr(cur), w, h, pitch, blk, span,
                                             cost_code(cost), lam, ctypes.byref(st)), self._h)
        return out

    # ---- rate-constrained search (include/me.h "rate-constrained motion search") ----
    def _pred(self, pred, n):
        if pred is None:
            return None
        pred = np.ascontiguousarray(pred, np.int16)
        if pred.size != 2 * n:
            raise MEError(_lib.ME_EINVAL, f"predictor of {pred.size // 2} records for {n} blocks")
        return pred

    def rd_search(self, ref, cur, blk: int, span: int, lam: int = 0, pred=None, cost="sad",
                  width=None):
        """The minimiser of SAD + lam * bits(4 mv - pred) per block
        (me_rd_search) on (H, pitch) uint8 planes; pred int16 [nblocks, 2] in
        quarter-pel units or None (all zero); width (default: the pitch) names
        the frame's columns.  Returns (mv int16 [nblocks, 2], J uint32, SAD
        uint32, bits uint8)."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, pitch = ref.shape
        w = width or pitch
        n = num_blocks(w, h, blk) if blk > 0 else 0
        pred = self._pred(pred, n)
        mv = np.zeros((max(n, 1), 2), np.int16)
        j, d = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        r = np.zeros(max(n, 1), np.uint8)
        check(_lib.lib().me_rd_search(self._h, _ptr(ref), _ptr(cur), w, h, pitch, blk, span,
                                      cost_code(cost), lam, _ptr(pred) if pred is not None else None,
                                      _ptr(mv), _ptr(j), _ptr(d), _ptr(r)), self._h)
        return mv[:n], j[:n], d[:n], r[:n]

    def partition_rd_search(self, ref, cur, blk: int, span: int, lam: int = 0, pred=None,
                            cost="sad", width=None) -> "PartitionRdFields":
        """partition_search on J = SAD + lam * bits(4 mv - pred) per partition,
        the mode priced by its code length (me_partition_rd_search); pred int16
        [macroblocks, 2] in quarter-pel units or None (all zero).  Returns
        PartitionRdFields of numpy arrays."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, pitch = ref.shape
        w = width or pitch
        out = PartitionRdFields.host(w, h, blk)
        pred = self._pred(pred, out.mode.size)
        st = out.rd_struct()
        check(_lib.lib().me_partition_rd_search(
            self._h, _ptr(ref), _ptr(cur), w, h, pitch, blk, span, cost_code(cost), lam,
            _ptr(pred) if pred is not None else None, ctypes.byref(st)), self._h)
        return out

    # ---- partition-wise quarter-pel refinement (include/me.h) ----
    def partition_refine_qpel(self, ref, cur, blk: int, fields, lam: int = 0, pred=None,
                              cost="sad", width=None) -> "PartitionRdFields":
        """The four integer grids of fields (a PartitionFields of numpy arrays;
        only mv is read) refined to quarter-pel partition by partition on
        cost + lam * bits(q - pred), and the mode decided again on the refined J
        (me_partition_refine_qpel); pred int16 [macroblocks, 2] in quarter-pel
        units or None (all zero).  Returns PartitionRdFields of numpy arrays
        with mv in quarter-pel units."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, pitch = ref.shape
        w = width or pitch
        out = PartitionRdFields.host(w, h, blk)
        mv = [np.ascontiguousarray(a, np.int16) for a in fields.mv]
        for a, o in zip(mv, out.mv):
            if a.size != o.size:
                raise MEError(_lib.ME_EINVAL, f"field of {a.size // 2} records for {o.size // 2} cells")
        pred = self._pred(pred, out.mode.size)
        st_in = PartitionFields(mv, None, out.mode, None).struct()
        st = out.rd_struct()
        check(_lib.lib().me_partition_refine_qpel(
            self._h, _ptr(ref), _ptr(cur), w, h, pitch, blk, cost_code(cost), lam,
            _ptr(pred) if pred is not None else None, ctypes.byref(st_in), ctypes.byref(st)),
            self._h)
        return out

    def partition_search_qpel(self, ref, cur, blk: int, span: int, lam: int = 0, pred=None,
                              cost="sad", width=None, leaf=True):
        """partition_rd_search at SAD, partition_refine_qpel at cost ("sad" or
        "satd") and, if leaf, the leaf field, back to back on the device
        (me_partition_search_qpel).  Returns (PartitionRdFields, leaf int16
        [nhx * nhy, 2] in quarter-pel units at block size blk / 2, or None)."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, pitch = ref.shape
        w = width or pitch
        out = PartitionRdFields.host(w, h, blk)
        pred = self._pred(pred, out.mode.size)
        leaf_mv = np.zeros((out.mv[3].shape[0], 2), np.int16) if leaf else None
        st = out.rd_struct()
        check(_lib.lib().me_partition_search_qpel(
            self._h, _ptr(ref), _ptr(cur), w, h, pitch, blk, span, cost_code(cost), lam,
            _ptr(pred) if pred is not None else None, ctypes.byref(st),
            _ptr(leaf_mv) if leaf else None), self._h)
        return out, leaf_mv

    def refine_qpel_rd(self, ref, cur, blk: int, mv, lam: int = 0, pred=None, cost="ssd",
                       stride=None):
        """refine_qpel on cost + lam * bits(q - pred) (me_refine_qpel_rd).
        Returns (mv_q int16 [nblocks, 2], Jq uint32, distortion uint32)."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, w = ref.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        mv = np.ascontiguousarray(mv, np.int16)
        if mv.size != 2 * n:
            raise MEError(_lib.ME_EINVAL, f"mv of {mv.size // 2} records for {n} blocks")
        pred = self._pred(pred, n)
        q = np.zeros((max(n, 1), 2), np.int16)
        j, d = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().me_refine_qpel_rd(self._h, _ptr(ref), _ptr(cur), w, h, stride or w, blk,
                                           cost_code(cost), lam,
                                           _ptr(pred) if pred is not None else None, _ptr(mv),
                                           _ptr(q), _ptr(j), _ptr(d)), self._h)
        return q[:n], j[:n], d[:n]

    def full_search_rd_qpel(self, ref, cur, blk: int, span: int, lam: int = 0, pred=None,
                            cost="sad", stride=None):
        """rd_search and refine_qpel_rd back to back on the device with one
        predictor and lam (me_full_search_rd_qpel).  Returns (mv_q int16
        [nblocks, 2] in quarter-pel units, Jq uint32 [nblocks])."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        if ref.ndim != 2 or ref.shape != cur.shape:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {ref.shape} vs {cur.shape}")
        h, w = ref.shape
        n = num_blocks(w, h, blk) if blk > 0 else 0
        pred = self._pred(pred, n)
        q = np.zeros((max(n, 1), 2), np.int16)
        j = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().me_full_search_rd_qpel(self._h, _ptr(ref), _ptr(cur), w, h, stride or w,
                                                blk, span, cost_code(cost), lam,
                                                _ptr(pred) if pred is not None else None, _ptr(q),
                                                _ptr(j)), self._h)
        return q[:n], j[:n]

    def search_pairs(self, frames, pairs, blk: int, span: int, cost="ssd"):
        """Search many (ref, cur) frame pairs in one pipelined call.

        frames: sequence of (H, W) uint8 planes (or one (N, H, W) array); pairs:
        [(ref_index, cur_index), ...].  Returns (mv int16 [npairs, nblocks, 2],
        cost uint32 [npairs, nblocks]).  Frames allocated with
        :func:`pinned_frames` are DMAed without staging."""
        # contiguous u8 frames pass through uncopied (pinned ones stay pinned)
        planes = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        if not planes:
            raise MEError(_lib.ME_EINVAL, "no frames")
        h, w = planes[0].shape
        for f in planes:
            if f.shape != (h, w):
                raise MEError(_lib.ME_EINVAL, f"frame shape {f.shape} != {(h, w)}")
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        npairs = pr.shape[0]
        n = num_blocks(w, h, blk) if blk > 0 else 0
        mv = np.zeros((max(npairs, 1), max(n, 1), 2), np.int16)
        cst = np.zeros((max(npairs, 1), max(n, 1)), np.uint32)
        ptrs = (ctypes.c_void_p * len(planes))(*[f.ctypes.data for f in planes])
        check(_lib.lib().me_search_pairs(self._h, ptrs, len(planes), w, h, w, blk, span,
                                         cost_code(cost), _ptr(pr), npairs, _ptr(mv),
                                         _ptr(cst)), self._h)
        return mv[:npairs, :n], cst[:npairs, :n]

    # ----------------------------------------------------------- device API
    def full_search_device(self, ref_t, cur_t, blk: int, span: int, cost, mv_t, cost_t=None,
                           stream=None, width=None, height=None, stride=None):
        """Enqueue a search on HBM-resident uint8 torch tensors (H, W); mv_t is an
        int16 tensor [nblocks, 2], cost_t uint32/int32 [nblocks] or None."""
        h, w = (height, width) if height else tuple(ref_t.shape[-2:])
        st = stream if stream is not None else _current_stream()
        check(_lib.lib().me_full_search_device(
            self._h, ref_t.data_ptr(), cur_t.data_ptr(), w, h, stride or w, blk, span,
            cost_code(cost), mv_t.data_ptr(), cost_t.data_ptr() if cost_t is not None else None,
            st), self._h)

    def search_stripe_device(self, ref_t, ref_row0: int, cur_t, cur_row0: int, width: int,
                             height: int, blk: int, span: int, cost, row_begin: int,
                             row_end: int, mv_t, cost_t=None, stream=None, stride=None):
        """One row stripe (block rows [row_begin, row_end)) on resident planes that
        start at frame rows ref_row0 / cur_row0."""
        st = stream if stream is not None else _current_stream()
        check(_lib.lib().me_full_search_stripe_device(
            self._h, ref_t.data_ptr(), ref_row0, cur_t.data_ptr(), cur_row0, width, height,
            stride or width, blk, span, cost_code(cost), row_begin, row_end, mv_t.data_ptr(),
            cost_t.data_ptr() if cost_t is not None else None, st), self._h)


    def search_stripes_device(self, width: int, height: int, blk: int, span: int, cost, jobs,
                              stream=None, stride=None):
        """Several stripes in one call (me_search_stripes_device).  jobs: list of
        (ref_t, ref_row0, cur_t, cur_row0, row_begin, row_end, mv_t, cost_t) --
        the arguments of one search_stripe_device each (tensors (rows, pitch))."""
        self.prepared_stripes_search(width, height, blk, span, cost, jobs, stream, stride)()

    def prepared_stripes_search(self, width, height, blk, span, cost, jobs, stream=None,
                                stride=None):
        """Zero-argument callable enqueueing search_stripes_device(...) with these buffers."""
        arr = (StripeJob * len(jobs))()
        for a, (rt, r0, ct, c0, b0, b1, mv, co) in zip(arr, jobs):
            a.d_ref, a.ref_row0, a.d_cur, a.cur_row0 = rt.data_ptr(), r0, ct.data_ptr(), c0
            a.block_row_begin, a.block_row_end = b0, b1
            a.d_mv_xy, a.d_block_cost = mv.data_ptr(), co.data_ptr() if co is not None else None
        pitch = stride or jobs[0][0].stride(0) * jobs[0][0].element_size()
        fn, h = _lib.lib().me_search_stripes_device, self._h
        args = (h, width, height, pitch, blk, span, cost_code(cost), arr, len(jobs),
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, h)
        run.jobs = arr  # keep the descriptor array alive with the callable
        return run

    def search_batch_device(self, ref_t, ref_row0: int, cur_t, cur_row0: int, width: int,
                            height: int, blk: int, span: int, cost, row_begin: int, row_end: int,
                            mv_t, cost_t=None, stream=None, stride=None):
        """A batch of stripes in one launch (me_full_search_batch_device):
        ref_t / cur_t are uint8 tensors [F, rows, pitch] (frame f = ref_t[f]),
        mv_t int16 [F * nblk, 2] and cost_t [F * nblk], frame-major."""
        st = stream if stream is not None else _current_stream()
        check(_lib.lib().me_full_search_batch_device(*self._batch_args(
            ref_t, ref_row0, cur_t, cur_row0, width, height, blk, span, cost, row_begin, row_end,
            mv_t, cost_t, st, stride)), self._h)

    def _batch_args(self, ref_t, ref_row0, cur_t, cur_row0, width, height, blk, span, cost,
                    row_begin, row_end, mv_t, cost_t, stream, stride):
        if ref_t.dim() != 3 or cur_t.dim() != 3 or ref_t.shape[0] != cur_t.shape[0]:
            raise MEError(_lib.ME_EINVAL, f"batch shapes {tuple(ref_t.shape)} / {tuple(cur_t.shape)}")
        es = ref_t.element_size()
        return (self._h, ref_t.data_ptr(), ref_t.stride(0) * es, ref_row0, cur_t.data_ptr(),
                cur_t.stride(0) * es, cur_row0, width, height, stride or ref_t.stride(1) * es,
                blk, span, cost_code(cost), row_begin, row_end, ref_t.shape[0],
                mv_t.data_ptr(), cost_t.data_ptr() if cost_t is not None else None, stream)

    def prepared_batch_search(self, ref_t, ref_row0, cur_t, cur_row0, width, height, blk, span,
                              cost, row_begin, row_end, mv_t, cost_t, stream=None, stride=None):
        """Zero-argument callable enqueueing search_batch_device(...) with these buffers."""
        fn, h = _lib.lib().me_full_search_batch_device, self._h
        args = self._batch_args(ref_t, ref_row0, cur_t, cur_row0, width, height, blk, span, cost,
                                row_begin, row_end, mv_t, cost_t,
                                stream if stream is not None else _current_stream(), stride)

        def run():
            s = fn(*args)
            if s:
                check(s, h)
        return run

    def refine_qpel_device(self, ref_t, cur_t, blk: int, cost, mv_t, q_t=None, cost_t=None,
                           stream=None, width=None, height=None):
        """Enqueue the quarter-pel refinement of resident frames
        (me_refine_qpel_device): ref_t / cur_t are uint8 tensors (H, pitch) or a
        batch [F, H, pitch], mv_t the integer field int16 [F * nblocks, 2], q_t
        the result (None: in place, into mv_t), cost_t uint32/int32
        [F * nblocks] or None.  width / height default to the tensors' last
        two dimensions; the row pitch and the frame stride are the tensors'."""
        self.prepared_refine_qpel(ref_t, cur_t, blk, cost, mv_t, q_t, cost_t, stream, width,
                                  height)()

    def prepared_refine_qpel(self, ref_t, cur_t, blk, cost, mv_t, q_t=None, cost_t=None,
                             stream=None, width=None, height=None):
        """Zero-argument callable enqueueing refine_qpel_device(...) with these buffers."""
        if ref_t.dim() not in (2, 3) or ref_t.dim() != cur_t.dim() or \
                (ref_t.dim() == 3 and ref_t.shape[0] != cur_t.shape[0]):
            raise MEError(_lib.ME_EINVAL, f"plane shapes {tuple(ref_t.shape)} / {tuple(cur_t.shape)}")
        es = ref_t.element_size()
        frames = ref_t.shape[0] if ref_t.dim() == 3 else 1
        rfs = ref_t.stride(0) * es if ref_t.dim() == 3 else 0
        cfs = cur_t.stride(0) * es if cur_t.dim() == 3 else 0
        h = height if height else ref_t.shape[-2]
        w = width if width else ref_t.shape[-1]
        fn, ctx = _lib.lib().me_refine_qpel_device, self._h
        args = (ctx, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, ref_t.stride(-2) * es, blk,
                cost_code(cost), frames, mv_t.data_ptr(),
                (q_t if q_t is not None else mv_t).data_ptr(),
                cost_t.data_ptr() if cost_t is not None else None,
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        return run

    def bipred_device(self, ref0_t, ref1_t, cur_t, blk: int, cost, q0_t, q1_t, mode_t,
                      out0_t=None, out1_t=None, cost_t=None, cost3_t=None, refine=True,
                      stream=None, width=None, height=None):
        """Enqueue the bi-prediction of resident frames (me_bipred_device):
        ref0_t / ref1_t / cur_t are uint8 tensors (H, pitch) of one row pitch or
        batches [F, H, pitch], q0_t / q1_t the quarter-pel fields int16
        [F * nblocks, 2], out0_t / out1_t the results (None: in place), mode_t
        uint8 [F * nblocks], cost_t uint32/int32 [F * nblocks] or None, cost3_t
        [F * nblocks, 3] or None."""
        self.prepared_bipred(ref0_t, ref1_t, cur_t, blk, cost, q0_t, q1_t, mode_t, out0_t, out1_t,
                             cost_t, cost3_t, refine, stream, width, height)()

    def prepared_bipred(self, ref0_t, ref1_t, cur_t, blk, cost, q0_t, q1_t, mode_t, out0_t=None,
                        out1_t=None, cost_t=None, cost3_t=None, refine=True, stream=None,
                        width=None, height=None):
        """Zero-argument callable enqueueing bipred_device(...) with these buffers."""
        dims = {ref0_t.dim(), ref1_t.dim(), cur_t.dim()}
        es = cur_t.element_size()
        if dims not in ({2}, {3}) or len({t.shape[0] for t in (ref0_t, ref1_t, cur_t)}) != 1 or \
                len({t.stride(-2) for t in (ref0_t, ref1_t, cur_t)}) != 1:
            raise MEError(_lib.ME_EINVAL, f"plane shapes {tuple(ref0_t.shape)} / "
                          f"{tuple(ref1_t.shape)} / {tuple(cur_t.shape)} or row pitches differ")
        batch = cur_t.dim() == 3
        frames = cur_t.shape[0] if batch else 1
        fs = [t.stride(0) * es if batch else 0 for t in (ref0_t, ref1_t, cur_t)]
        h = height if height else cur_t.shape[-2]
        w = width if width else cur_t.shape[-1]
        opt = lambda t: t.data_ptr() if t is not None else None
        fn, ctx = _lib.lib().me_bipred_device, self._h
        args = (ctx, ref0_t.data_ptr(), fs[0], ref1_t.data_ptr(), fs[1], cur_t.data_ptr(), fs[2],
                w, h, cur_t.stride(-2) * es, blk, cost_code(cost), int(bool(refine)), frames,
                q0_t.data_ptr(), q1_t.data_ptr(),
                (out0_t if out0_t is not None else q0_t).data_ptr(),
                (out1_t if out1_t is not None else q1_t).data_ptr(), mode_t.data_ptr(),
                opt(cost_t), opt(cost3_t), stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        return run

    def partition_search_device(self, ref_t, cur_t, blk: int, span: int, lam: int, fields,
                                cost="sad", stream=None, width=None, height=None):
        """Enqueue the partition search of resident frames
        (me_partition_search_device): ref_t / cur_t are uint8 tensors (H, pitch)
        or batches [F, H, pitch], fields a PartitionFields of torch tensors
        (PartitionFields.device).  width / height default to the tensors' last
        two dimensions; the row pitch and the frame strides are the tensors'."""
        self.prepared_partition_search(ref_t, cur_t, blk, span, lam, fields, cost, stream, width,
                                       height)()

    def prepared_partition_search(self, ref_t, cur_t, blk, span, lam, fields, cost="sad",
                                  stream=None, width=None, height=None):
        """Zero-argument callable enqueueing partition_search_device(...) with these buffers."""
        if ref_t.dim() not in (2, 3) or ref_t.dim() != cur_t.dim() or \
                ref_t.stride(-2) != cur_t.stride(-2) or \
                (ref_t.dim() == 3 and ref_t.shape[0] != cur_t.shape[0]):
            raise MEError(_lib.ME_EINVAL, f"plane shapes {tuple(ref_t.shape)} / "
                          f"{tuple(cur_t.shape)} or row pitches differ")
        es = ref_t.element_size()
        frames = ref_t.shape[0] if ref_t.dim() == 3 else 1
        rfs = ref_t.stride(0) * es if ref_t.dim() == 3 else 0
        cfs = cur_t.stride(0) * es if cur_t.dim() == 3 else 0
        h = height if height else ref_t.shape[-2]
        w = width if width else ref_t.shape[-1]
        st = fields.struct()
        fn, ctx = _lib.lib().me_partition_search_device, self._h
        args = (ctx, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, ref_t.stride(-2) * es, blk,
                span, cost_code(cost), lam, frames, ctypes.byref(st),
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        run.fields = st  # keep the pointer struct alive with the callable
        return run

    def rd_search_device(self, ref_t, cur_t, blk: int, span: int, lam: int, mv_t, cost_t,
                         dist_t=None, bits_t=None, pred_t=None, cost="sad", stream=None,
                         width=None, height=None):
        """Enqueue the rate-constrained search of resident frames
        (me_rd_search_device): ref_t / cur_t are uint8 tensors (H, pitch) or
        batches [F, H, pitch], pred_t the quarter-pel predictors int16
        [F * nblocks, 2] or None (all zero), mv_t int16 [F * nblocks, 2], cost_t
        (J) and dist_t (SAD, or None) uint32/int32 [F * nblocks], bits_t uint8
        [F * nblocks] or None.  width / height default to the tensors' last two
        dimensions; the row pitch and the frame strides are the tensors'."""
        self.prepared_rd_search(ref_t, cur_t, blk, span, lam, mv_t, cost_t, dist_t, bits_t, pred_t,
                                cost, stream, width, height)()

    def _plane_args(self, ref_t, cur_t, width, height):
        if ref_t.dim() not in (2, 3) or ref_t.dim() != cur_t.dim() or \
                ref_t.stride(-2) != cur_t.stride(-2) or \
                (ref_t.dim() == 3 and ref_t.shape[0] != cur_t.shape[0]):
            raise MEError(_lib.ME_EINVAL, f"plane shapes {tuple(ref_t.shape)} / "
                          f"{tuple(cur_t.shape)} or row pitches differ")
        es = ref_t.element_size()
        frames = ref_t.shape[0] if ref_t.dim() == 3 else 1
        rfs = ref_t.stride(0) * es if ref_t.dim() == 3 else 0
        cfs = cur_t.stride(0) * es if cur_t.dim() == 3 else 0
        h = height if height else ref_t.shape[-2]
        w = width if width else ref_t.shape[-1]
        return frames, rfs, cfs, w, h, ref_t.stride(-2) * es

    def prepared_rd_search(self, ref_t, cur_t, blk, span, lam, mv_t, cost_t, dist_t=None,
                           bits_t=None, pred_t=None, cost="sad", stream=None, width=None,
                           height=None):
        """Zero-argument callable enqueueing rd_search_device(...) with these buffers."""
        frames, rfs, cfs, w, h, pitch = self._plane_args(ref_t, cur_t, width, height)
        opt = lambda t: t.data_ptr() if t is not None else None
        fn, ctx = _lib.lib().me_rd_search_device, self._h
        args = (ctx, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, pitch, blk, span,
                cost_code(cost), lam, frames, opt(pred_t), opt(mv_t), opt(cost_t), opt(dist_t),
                opt(bits_t), stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        return run

    def partition_rd_search_device(self, ref_t, cur_t, blk: int, span: int, lam: int, fields,
                                   pred_t=None, cost="sad", stream=None, width=None, height=None):
        """Enqueue the rate-constrained partition search of resident frames
        (me_partition_rd_search_device): partition_search_device's arguments
        with fields a PartitionRdFields of torch tensors
        (PartitionRdFields.device) and pred_t the macroblocks' quarter-pel
        predictors int16 [F * macroblocks, 2] or None (all zero)."""
        self.prepared_partition_rd_search(ref_t, cur_t, blk, span, lam, fields, pred_t, cost,
                                          stream, width, height)()

    def prepared_partition_rd_search(self, ref_t, cur_t, blk, span, lam, fields, pred_t=None,
                                     cost="sad", stream=None, width=None, height=None):
        """Zero-argument callable enqueueing partition_rd_search_device(...) with these buffers."""
        frames, rfs, cfs, w, h, pitch = self._plane_args(ref_t, cur_t, width, height)
        st = fields.rd_struct()
        fn, ctx = _lib.lib().me_partition_rd_search_device, self._h
        args = (ctx, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, pitch, blk, span,
                cost_code(cost), lam, frames, pred_t.data_ptr() if pred_t is not None else None,
                ctypes.byref(st), stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        run.fields = st  # keep the pointer struct alive with the callable
        return run

    def partition_refine_qpel_device(self, ref_t, cur_t, blk: int, cost, lam: int, fields_in,
                                     fields_out, pred_t=None, stream=None, width=None,
                                     height=None):
        """Enqueue the partition-wise quarter-pel refinement of resident frames
        (me_partition_refine_qpel_device): fields_in a PartitionFields of torch
        tensors whose four integer mv grids are read, fields_out a
        PartitionRdFields of torch tensors (it may share fields_in's mv tensors:
        in place), pred_t int16 [F * macroblocks, 2] or None (all zero)."""
        self.prepared_partition_refine_qpel(ref_t, cur_t, blk, cost, lam, fields_in, fields_out,
                                            pred_t, stream, width, height)()

    def prepared_partition_refine_qpel(self, ref_t, cur_t, blk, cost, lam, fields_in, fields_out,
                                       pred_t=None, stream=None, width=None, height=None):
        """Zero-argument callable enqueueing partition_refine_qpel_device(...) with these buffers."""
        frames, rfs, cfs, w, h, pitch = self._plane_args(ref_t, cur_t, width, height)
        st_in, st = fields_in.struct(), fields_out.rd_struct()
        fn, ctx = _lib.lib().me_partition_refine_qpel_device, self._h
        args = (ctx, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, pitch, blk,
                cost_code(cost), lam, frames, pred_t.data_ptr() if pred_t is not None else None,
                ctypes.byref(st_in), ctypes.byref(st),
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, ctx)
        run.fields = (st_in, st)  # keep the pointer structs alive with the callable
        return run

    def refine_qpel_rd_device(self, ref_t, cur_t, blk: int, cost, lam: int, mv_t, q_t=None,
                              cost_t=None, dist_t=None, pred_t=None, stream=None, width=None,
                              height=None):
        """Enqueue the rate-constrained quarter-pel refinement of resident
        frames (me_refine_qpel_rd_device): refine_qpel_device's arguments plus
        lam, pred_t (int16 [F * nblocks, 2] or None: all zero) and dist_t (the
        distortion at the result, or None); cost_t receives Jq."""
        frames, rfs, cfs, w, h, pitch = self._plane_args(ref_t, cur_t, width, height)
        opt = lambda t: t.data_ptr() if t is not None else None
        check(_lib.lib().me_refine_qpel_rd_device(
            self._h, ref_t.data_ptr(), rfs, cur_t.data_ptr(), cfs, w, h, pitch, blk,
            cost_code(cost), lam, frames, opt(pred_t), mv_t.data_ptr(),
            (q_t if q_t is not None else mv_t).data_ptr(), opt(cost_t), opt(dist_t),
            stream if stream is not None else _current_stream()), self._h)

    def partition_leaf_field_device(self, width: int, height: int, blk: int, fields, leaf_t,
                                    frames: int = 1, stream=None):
        """Enqueue the leaf field of `frames` searched frames
        (me_partition_leaf_field_device): leaf_t int16 [frames * nhx * nhy, 2],
        an ordinary integer field of block size blk / 2."""
        st = fields.struct()
        check(_lib.lib().me_partition_leaf_field_device(
            self._h, width, height, blk, frames, ctypes.byref(st), leaf_t.data_ptr(),
            stream if stream is not None else _current_stream()), self._h)

    # ---- multi-process stripes: the one exchange step in native code ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """RCCL unique id (rank 0), to be sent to every rank out of band."""
        buf = ctypes.create_string_buffer(_lib.ME_COMM_ID_BYTES)
        check(_lib.lib().me_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, n_ranks: int, rank: int) -> None:
        """Join an n_ranks RCCL group on this context's first device (collective)."""
        if len(uid) != _lib.ME_COMM_ID_BYTES:
            raise ValueError(f"comm id of {len(uid)} bytes, expected {_lib.ME_COMM_ID_BYTES}")
        check(_lib.lib().me_comm_init(self._h, uid, n_ranks, rank), self._h)
        self.comm_ranks = n_ranks

    def gather_device(self, send_t, recv_t=None, stream=None) -> None:
        """Gather send_t (same byte count on every rank) into rank 0's recv_t
        (n_ranks x the bytes, rank order), enqueued on `stream` (default: torch's
        current stream)."""
        st = stream if stream is not None else _current_stream()
        check(_lib.lib().me_gather_device(
            self._h, send_t.data_ptr(), send_t.numel() * send_t.element_size(),
            recv_t.data_ptr() if recv_t is not None else None, st), self._h)


    def comm_check(self, timeout_ms: int = _lib.ME_COMM_TIMEOUT_MS, stream=None) -> None:
        """Bounded wait for the work on `stream` (default: torch's current
        stream) with RCCL failure detection (me_comm_check): raises MEError
        (ME_ECOMM) on an RCCL error or when timeout_ms passed; the communicator
        is then aborted."""
        st = stream if stream is not None else _current_stream()
        check(_lib.lib().me_comm_check(self._h, st, int(timeout_ms)), self._h)

    def device_check(self) -> None:
        """Raise MEError (ME_EDEVICE) if a search kernel reported a broken
        in-kernel invariant since the last check (call after synchronising)."""
        check(_lib.lib().me_device_check(self._h), self._h)

    # ---- captured steps: one graph launch per frame ----
    def capture(self, stream, enqueue) -> "Graph":
        """Record what enqueue() puts on `stream` (device entry points of this
        context, e.g. a stripe search and its gather) as one graph.  Run the
        searches once uncaptured first (they size the context's scratch)."""
        L = _lib.lib()
        check(L.me_capture_begin(self._h, stream), self._h)
        g = ctypes.c_void_p()
        try:
            enqueue()
        except BaseException:
            # end the capture (the stream must leave capture mode) and drop the
            # graph it made; the enqueue's exception is the one that propagates
            if L.me_capture_end(self._h, stream, ctypes.byref(g)) == _lib.ME_OK and g:
                L.me_graph_destroy(g)
            raise
        st = L.me_capture_end(self._h, stream, ctypes.byref(g))
        check(st, self._h)
        gr = Graph(self, g)
        if not hasattr(self, "_graphs"):
            self._graphs = []
        self._graphs.append(gr)  # destroyed before the context (include/me.h)
        return gr

    # ---- prepared calls: arguments marshalled once per buffer set ----
    # A sharded step on a small stripe is bound by host time (an 8-way 1080p
    # stripe searches in 15-18 us), so the per-frame calls skip the wrapper's
    # argument handling.  The caller keeps the tensors alive.
    def prepared_stripe_search(self, ref_t, ref_row0, cur_t, cur_row0, width, height, blk,
                               span, cost, row_begin, row_end, mv_t, cost_t, stream=None,
                               stride=None):
        """Zero-argument callable enqueueing search_stripe_device(...) with these
        fixed buffers on `stream` (default: torch's current stream now)."""
        fn, h = _lib.lib().me_full_search_stripe_device, self._h
        args = (h, ref_t.data_ptr(), ref_row0, cur_t.data_ptr(), cur_row0, width, height,
                stride or width, blk, span, cost_code(cost), row_begin, row_end,
                mv_t.data_ptr(), cost_t.data_ptr() if cost_t is not None else None,
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, h)
        return run

    def prepared_gather(self, send_t, recv_t=None, stream=None):
        """Zero-argument callable enqueueing gather_device(send_t, recv_t)."""
        fn, h = _lib.lib().me_gather_device, self._h
        args = (h, send_t.data_ptr(), send_t.numel() * send_t.element_size(),
                recv_t.data_ptr() if recv_t is not None else None,
                stream if stream is not None else _current_stream())

        def run():
            s = fn(*args)
            if s:
                check(s, h)
        return run


class StripeJob(ctypes.Structure):
    """include/me.h me_stripe_job."""
    _fields_ = [("d_ref", ctypes.c_void_p), ("ref_row0", ctypes.c_int),
                ("d_cur", ctypes.c_void_p), ("cur_row0", ctypes.c_int),
                ("block_row_begin", ctypes.c_int), ("block_row_end", ctypes.c_int),
                ("d_mv_xy", ctypes.c_void_p), ("d_block_cost", ctypes.c_void_p)]


class Graph:
    """A captured step (me_capture_begin/end); launch() replays it on a stream."""

    def __init__(self, eng: Engine, handle):
        self._eng, self._h = eng, handle
        self._launch = _lib.lib().me_graph_launch

    def launch(self, stream) -> None:
        s = self._launch(self._h, stream)
        if s:
            check(s, self._eng._h)

    def prepared(self, stream):
        """Zero-argument callable launching the graph on `stream`."""
        fn, h, ctx = self._launch, self._h, self._eng._h

        def run():
            s = fn(h, stream)
            if s:
                check(s, ctx)
        return run

    def set_kernel_path(self, path) -> None:
        """This context's kernel path (me_ctx_set_kernel_path): one of
        set_kernel_path()'s names, or None to follow the process-wide path."""
        if path is not None and path not in _PATH_CODES:
            raise MEError(_lib.ME_EINVAL, f"unknown kernel path {path!r}")
        self._eng.set_kernel_path(path)  # the handle here is the graph's, not the context's

    def last_search_path(self, device_index: int = 0) -> str:
        """The kernel family of this context's latest search on its device
        `device_index` (me_ctx_last_search_path)."""
        return self._eng.last_search_path(device_index)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().me_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Pinned:
    """Owner of one me_host_alloc block (freed when the last view dies)."""

    def __init__(self, nbytes: int):
        self.ptr = _lib.lib().me_host_alloc(nbytes)
        if not self.ptr:
            raise MEError(_lib.ME_ENOMEM, f"me_host_alloc({nbytes})")

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                _lib.lib().me_host_free(self.ptr)
            except Exception:  # interpreter shutdown: module globals already torn down
                pass
            self.ptr = None


def pinned_frames(n: int, height: int, width: int) -> np.ndarray:
    """(n, height, width) uint8 array in pinned host memory (me_host_alloc):
    frames written here are uploaded by DMA without a staging copy."""
    owner = _Pinned(max(1, n * height * width))
    buf = (ctypes.c_uint8 * (n * height * width)).from_address(owner.ptr)
    buf._owner = owner  # keep the allocation alive with every view
    return np.frombuffer(buf, dtype=np.uint8).reshape(n, height, width)


def _current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
