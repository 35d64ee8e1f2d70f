"""Sheared-periodic ("lattice") frames that tie candidates everywhere, and the
census that proves it (numpy only: no GPU, no library load).

Every search entry point promises the first minimum in raster order (dy outer,
dx inner, strict <).  A flat frame ties every candidate, so the winner is the
window's top-left corner under ANY key order; a 0/255 board keeps the winner at
cost 0 in the first dy chunk and the first dx group.  Neither can tell a kernel
that orders its keys by (dy, dx) from one that orders them by (dx, dy).

A reference that is periodic on a sheared lattice can:

    ref[y, x] = base[y % Py, (x + shear * (y // Py)) % Px]

so ref[y, x] == ref[y + vy, x + vx] for every lattice vector v = i (Px, 0) +
j (-shear, Py).  Candidates d and d + v then read identical reference patches:
their SAD, SSD, SSIM score and box-sum bound are bit-identical WHATEVER the
current frame holds.  The tie survives noise blended into the current frame,
so it sits at any cost level and with any live-list length of the pruning flow
kernel.  A current frame is the lattice evaluated at displaced coordinates
(cur[y, x] = ref[y + sy, x + sx], exact at the frame edges too), per column
strip its own displacement, blended with a / 256 of uniform noise of its own.

Special lattices (beside the regular ones between (23, 19, 9) and (47, 29, 30)):
  (23, 5, 1)   v = (-1, 5), (-2, 10): partners inside one lane-task on rows
               that different parts of a row split own;
  (29, 5, 9)   v = (-9, 5): same dy chunk, another dx group, dx_first > dx_other;
  (3, 19, 1)   v = (3, 0): partners inside one lane-task on one row;
  (67, 1, 64)  v = (-64, 1): the wrap pair (+32, d) against (-32, d + 1);
  defect       rows of the REFERENCE overwritten with noise break the copies at
               dy < 0 of the blocks below them, so (0, 0), a seed of the flow
               kernel's bound, is the raster-first minimiser with partners at
               dy > 0 (in a pure lattice -v is in an unclamped window whenever
               +v is, so a partner always precedes (0, 0)).

census() brute-forces the SAD map of every full-size block (the window is
me_full_search's, rd_ref._window) and returns per block the minimum, the number
of minimisers, and the raster-first, the (dx, dy)-first and the raster-last
one.  pair_classes() classifies the tied pairs (first, other) of the unclamped
16x16 +-32 blocks by the flow kernel's geometry (csrc/me_flow_kernel.inc, the
unsplit task and flow_split_task; csrc/me_geom.h flow_split_*):

    column cx = dx + 32, row-of-window cy = dy + 32
    chunk  cy // 13, row cy % 13
    group  cx // 4 for cx < 64; the fold column cx = 64 (dx = +32) of row j
           belongs to the lane-task of group j of its chunk (lane gi < 13 owns
           the fold candidate of row gi), and in a split task to part 0
    lane-task = (chunk, block, group); under the row split with R rows per lane
           part i owns rows [min(i R, 13 - R), + R)

  same_row      same lane-task, same row
  split_R       same lane-task, no part of the R-row split holds both (R = 1,
                2, 3, 4, 7)
  groups        same chunk, different groups, dx_first > dx_other
  chunks        different chunks
  fold          one of the two is in the fold column;  wrap: (+32, d) against
                (-32 + k, d + 1), k <= 3
  seed_later    other == (0, 0);  seed_earlier: first == (0, 0)

live_estimate() is the numpy bound of test_gpu_sad_prune.py (box_q) per item of
4 blocks: the lane-tasks with 16 minlb - 240 <= U_b, U_b = min(SAD(0, 0), SAD
at the smallest bound, ties by the kernel's entry order).  It serves only to
grade the noise weights; it is never asserted against the GPU.

Figures of the table below (tests/test_tie_cases.py prints and asserts them;
thresholds: tied >= 60 % of the full blocks, first != (dx, dy)-first and first
!= last in >= 50 % of the tied ones):

  case          full blocks  tied            first != (dx, dy)-first  first != last
  lat_320x136   3200         3058 (95.6 %)   1946 (63.6 % of tied)    3058 (100 %)
  lat_256x64    2048         2033 (99.3 %)   1461 (71.9 %)            2033 (100 %)
  lat_1024x512  2048         2047 (100.0 %)  1982 (96.8 %)            2047 (100 %)
  lat_small      168          167 (99.4 %)    125 (74.9 %)             167 (100 %)

  tied pairs (first, other) of the unclamped blocks, by class:
                same_row  split_1  _2   _3   _4   _7   groups  chunks  fold  wrap  seed_later  seed_earlier
  lat_320x136   64        224      160  96   96   64   672     14060   4462  64    76          64
  lat_1024x512  224       224      224  224  224  0    0       8232    840   0     166         0
  (lat_256x64 has no unclamped block; lat_small serves the kernels without a flow geometry.)

  live_estimate's wave-tasks of lat_320x136 by the rows per lane of the row split, R = 1: 29, 2: 59, 3: 57,
  4: 70, 7: 251; the tuning build's histogram (me_debug_prune_split_hist) counted the same on an MI355X.

  blocks of lat_small that keep a tie of J under midpoint_pred, lambda = 0 / 5 / 1000:
  16x16 +-16: 165 / 151 / 148 of 208;  16x16 +-32: 206 / 173 / 173 of 208;  8x8 +-16 (frame 0): 375 of 375 each.

Oracle budget: a case costs at most 5e7 16x16 candidate equivalents
(valu_envelope_cases.oracle_cost's measure).
"""
from __future__ import annotations

import functools
import os
from collections import Counter, namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import rd_ref
import valu_envelope_cases as V

B, S, K, G = 16, 32, 13, 16
INVALID = 0xFFFF  # above the largest 16x16 SAD, 65,280
SPLIT_ROWS = (1, 2, 3, 4, 7)
ORACLE_BUDGET = V.ORACLE_BUDGET
THREADS = min(8, os.cpu_count() or 1)


# ------------------------------------------------------------------ content
def _tile(Py, Px, seed, raw=False):
    """A random Py x Px tile, smoothed periodically ([1 2 1] / 4 along an axis:
    twice from 8 samples on, once from 4, not below: a tiny tile keeps its
    contrast); raw: not smoothed at all."""
    t = np.random.default_rng(seed).integers(0, 256, (Py, Px)).astype(np.int64)
    for ax, n in ((0, Py), (1, Px)):
        for _ in range(0 if raw else 2 if n >= 8 else 1 if n >= 4 else 0):
            t = (np.roll(t, 1, ax) + 2 * t + np.roll(t, -1, ax) + 2) >> 2
    return t.astype(np.uint8)


def lattice_ref(h, w, Px, Py, shear, seed, oy=0, ox=0, raw=False):
    """base[y % Py, (x + shear * (y // Py)) % Px] at y = oy .. oy + h - 1, x =
    ox .. ox + w - 1 (any integers: the lattice has no edge)."""
    base = _tile(Py, Px, seed, raw)
    yy = np.arange(h)[:, None] + oy
    xx = np.arange(w)[None, :] + ox
    return np.ascontiguousarray(base[yy % Py, (xx + shear * (yy // Py)) % Px])


# One frame: the lattice (Px, Py, shear), per column strip of equal width its
# displacement (sx, sy) (cur[y, x] = ref[y + sy, x + sx]) and its noise weight
# a of 256 (one int: every strip's), and the reference rows [y0, y1) that hold
# noise instead of the lattice; raw: the tile is not smoothed (unrelated patches
# are far apart in SAD, so a tie of J survives a large lambda).
Fr = namedtuple("Fr", "lat shifts ampl defect raw", defaults=((), False))
Case = namedtuple("Case", "name width height seed frames")


def build_frame(w, h, fr, seed):
    rng = np.random.default_rng(seed)
    Px, Py, shear = fr.lat
    ref = lattice_ref(h, w, Px, Py, shear, seed, raw=fr.raw)
    n = len(fr.shifts)
    assert w % n == 0
    ampl = fr.ampl if isinstance(fr.ampl, tuple) else (fr.ampl,) * n
    cur = np.empty((h, w), np.uint8)
    for i, ((sx, sy), a) in enumerate(zip(fr.shifts, ampl)):
        x0, sw = i * (w // n), w // n
        c = lattice_ref(h, sw, Px, Py, shear, seed, sy, x0 + sx, fr.raw).astype(np.int32)
        cur[:, x0:x0 + sw] = ((256 - a) * c + a * rng.integers(0, 256, (h, sw))) >> 8
    for y0, y1 in fr.defect:
        ref[y0:y1] = rng.integers(0, 256, (y1 - y0, w), dtype=np.uint8)
    return ref, cur


def sweep_shifts():
    """test_gpu_flow_split's dy_sweep: 40 (dx, dy), dy + 32 on every row 0 .. 12
    of a chunk in three chunks (0 and 64 among them), dx = +32 / -32 / other
    per row, and (0, 0)."""
    from test_gpu_flow_split import _sweep_shifts  # (numpy and ctypes declarations only: no library is loaded)
    return _sweep_shifts()


REGULAR = [(23, 19, 9), (47, 29, 30), (31, 23, 12), (37, 17, 20)]
HALVES = ((3, -3), (-6, 4))


def _lat_320x136():
    sw = sweep_shifts()
    grade = [0, 6, 10, 12, 14, 16, 18, 20, 22, 24]
    fr = [Fr(REGULAR[f % 4], tuple(sw[4 * f:4 * f + 4]), grade[f]) for f in range(10)]
    fr += [
        Fr((23, 5, 1), HALVES, (4, 12)),
        Fr((29, 5, 9), HALVES, (8, 16)),
        Fr((3, 19, 1), ((3, -3),), 10),
        Fr((67, 1, 64), ((32, -32),), 8),
        Fr((47, 29, 30), ((0, 0),), 12, ((44, 48), (60, 64))),
        Fr((23, 19, 9), ((0, 0),), 16),
        Fr((23, 19, 9), HALVES, (26, 28)),
        Fr((47, 29, 30), HALVES, (20, 28)),
        Fr((31, 23, 12), HALVES, (32, 64)),
        Fr((37, 17, 20), HALVES, (40, 256)),
    ]
    return Case("lat_320x136", 320, 136, 3201, tuple(fr))


def _lat_256x64():
    sw = sweep_shifts()
    lats = [(23, 19, 9), (31, 23, 12), (29, 5, 9), (23, 5, 1), (19, 13, 7), (27, 11, 5)]
    grade = [0, 4, 8, 10, 12, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24]
    fr = [Fr(lats[f % 6], (sw[(2 * f) % 40], sw[(2 * f + 1) % 40]), (grade[f // 2], grade[f // 2] + 2 * (f % 2)))
          for f in range(30)]
    fr += [Fr((23, 19, 9), HALVES, (40, 256)), Fr((31, 23, 12), ((0, 0),), 0)]
    return Case("lat_256x64", 256, 64, 2564, tuple(fr))


def _lat_1024x512():
    sw = sweep_shifts()
    shifts = tuple(sw[i] for i in (0, 7, 13, 18, 22, 29, 33, 39))
    return Case("lat_1024x512", 1024, 512, 1024, (Fr((37, 17, 20), shifts, (0, 8, 14, 18, 22, 26, 32, 64)),))


def _lat_small():
    return Case("lat_small", 200, 120, 200, (Fr((3, 3, 1), ((2, -1),), 6, raw=True),
                                               Fr((23, 19, 9), HALVES, (0, 10), raw=True)))


CASES = {c.name: c for c in (_lat_320x136(), _lat_256x64(), _lat_1024x512(), _lat_small())}
FLOW_CASES = ("lat_320x136", "lat_256x64", "lat_1024x512")  # >= 512 tiles of 4 blocks, width % 64 == 0


@functools.lru_cache(maxsize=None)
def frames(name):
    """(ref [F, h, w], cur [F, h, w]) of a named case, read-only."""
    c = CASES[name]
    pairs = [build_frame(c.width, c.height, fr, c.seed + 17 * f) for f, fr in enumerate(c.frames)]
    ref, cur = np.stack([r for r, _ in pairs]), np.stack([k for _, k in pairs])
    ref.setflags(write=False)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def case_census(name):
    """census() of the whole case at 16x16 +-32, computed once."""
    return census(*frames(name))


def oracle_cost(case, blk=B, span=S):
    """16x16 candidate equivalents of the whole case (valu_envelope_cases.oracle_cost's measure)."""
    return len(case.frames) * V.candidate_count(case.width, case.height, blk, span) * blk * blk / 256.0


# ------------------------------------------------------------------- census
Census = namedtuple("Census", "cost cmin nmin first dxfirst last unclamped")


def sad_maps(ref, cur, blk=B, span=S):
    """uint16 [F, 2S+1, 2S+1, nby, nbx] over (dy, dx) and the FULL-size blocks:
    the SAD, INVALID where the block has no such candidate."""
    ref, cur = np.asarray(ref, np.uint8), np.asarray(cur, np.uint8)
    if ref.ndim == 2:
        ref, cur = ref[None], cur[None]
    F, H, W = ref.shape
    assert blk * blk * 255 < INVALID
    nby, nbx = H // blk, W // blk
    n = 2 * span + 1
    refp = np.zeros((F, H + 2 * span, W + 2 * span), np.uint8)
    refp[:, span:span + H, span:span + W] = ref
    curc = np.ascontiguousarray(cur[:, :nby * blk, :nbx * blk])
    wx = np.array([rd_ref._window(bx * blk, blk, W, span) for bx in range(nbx)])
    wy = np.array([rd_ref._window(by * blk, blk, H, span) for by in range(nby)])
    out = np.full((F, n, n, nby, nbx), INVALID, np.uint16)

    def row(dy):
        vy = (wy[:, 0] <= dy) & (dy <= wy[:, 1])
        if not vy.any():
            return
        for dx in range(-span, span + 1):
            v = vy[:, None] & ((wx[:, 0] <= dx) & (dx <= wx[:, 1]))[None, :]
            if not v.any():
                continue
            r = refp[:, span + dy:span + dy + nby * blk, span + dx:span + dx + nbx * blk]
            d = np.maximum(curc, r) - np.minimum(curc, r)
            s = d.reshape(F, nby, blk, nbx, blk).sum(axis=4, dtype=np.uint16).sum(axis=2, dtype=np.uint16)
            out[:, dy + span, dx + span] = np.where(v[None], s, INVALID)

    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(row, range(-span, span + 1)))
    return out


def _first(mask, order):
    """First True of mask [F, ny, nx, nby, nbx] per block in the given order of
    (dy, dx): 'raster' (dy outer), 'dxdy' (dx outer) or 'last' (raster-last);
    int [F, nby, nbx, 2] as (dx, dy) indices."""
    F, ny, nx, nby, nbx = mask.shape
    if order == "dxdy":
        k = mask.transpose(0, 2, 1, 3, 4).reshape(F, nx * ny, nby, nbx).argmax(axis=1)
        ix, iy = k // ny, k % ny
    else:
        m = mask.reshape(F, ny * nx, nby, nbx)
        k = m.argmax(axis=1) if order == "raster" else ny * nx - 1 - m[:, ::-1].argmax(axis=1)
        iy, ix = k // nx, k % nx
    return np.stack([ix, iy], axis=-1)


def census(ref, cur, blk=B, span=S, order="raster"):
    """The minimisers of every full-size block.  first / dxfirst / last:
    int [F, nby, nbx, 2] displacements (dx, dy); unclamped: bool [nby, nbx]."""
    ref = np.asarray(ref)
    H, W = ref.shape[-2:]
    cost = sad_maps(ref, cur, blk, span)
    cmin = cost.min(axis=(1, 2))
    mask = cost == cmin[:, None, None]
    nby, nbx = H // blk, W // blk
    ucy = np.array([rd_ref._window(by * blk, blk, H, span) == (-span, span) for by in range(nby)])
    ucx = np.array([rd_ref._window(bx * blk, blk, W, span) == (-span, span) for bx in range(nbx)])
    return Census(cost, cmin.astype(np.uint32), mask.sum(axis=(1, 2)), _first(mask, order) - span,
                  _first(mask, "dxdy") - span, _first(mask, "last") - span, ucy[:, None] & ucx[None, :])


def minimisers(cen, f, by, bx):
    """The block's minimisers (dx, dy) in raster order."""
    span = (cen.cost.shape[1] - 1) // 2
    iy, ix = np.nonzero(cen.cost[f, :, :, by, bx] == cen.cmin[f, by, bx])
    return [(int(x) - span, int(y) - span) for y, x in zip(iy, ix)]


def tie_stats(cen):
    """(full blocks, tied, tied with first != (dx, dy)-first, tied with first != last)."""
    tied = cen.nmin > 1
    a = (cen.first != cen.dxfirst).any(axis=-1) & tied
    b = (cen.first != cen.last).any(axis=-1) & tied
    return int(tied.size), int(tied.sum()), int(a.sum()), int(b.sum())


# ------------------------------------------------- the flow kernel's geometry
def split_rows(n):
    """me_geom.h flow_split_rows: rows per lane of a wave-task of n list entries."""
    return 1 if n <= 4 else 2 if n <= 9 else 3 if n <= 12 else 4 if n <= 16 else 7 if n <= 32 else K


def split_parts(R):
    return (K + R - 1) // R


def split_row0(R, i):
    return min(i * R, K - R)


def split_lane(R, lane, n):
    """me_geom.h flow_split_lane: (entry, first row, live, fold)."""
    P = split_parts(R)
    e, part = divmod(lane, P)
    return [min(e, n - 1), split_row0(R, part), int(e < n), int(e < n and part == 0)]


def lane_task(d):
    """(chunk, group, row, in the fold column) of candidate d = (dx, dy)."""
    cx, cy = d[0] + S, d[1] + S
    chunk, row = divmod(cy, K)
    return (chunk, row, row, True) if cx == 2 * S else (chunk, cx // 4, row, False)


def parts_of(row, fold, R):
    """The parts of the R-row split whose lanes evaluate the candidate."""
    if fold:
        return {0}
    return {i for i in range(split_parts(R)) if split_row0(R, i) <= row < split_row0(R, i) + R}


def pair_labels(first, other):
    """Classes of the tied pair (first, other) of an unclamped 16x16 +-32 block."""
    c1, g1, r1, f1 = lane_task(first)
    c2, g2, r2, f2 = lane_task(other)
    out = set()
    if (c1, g1) == (c2, g2):
        if r1 == r2:
            out.add("same_row")
        for R in SPLIT_ROWS:
            if not parts_of(r1, f1, R) & parts_of(r2, f2, R):
                out.add(f"split_{R}")
    elif c1 == c2:
        if first[0] > other[0]:
            out.add("groups")
    else:
        out.add("chunks")
    if f1 or f2:
        out.add("fold")
    if f1 and other[1] == first[1] + 1 and other[0] <= -S + 3:
        out.add("wrap")
    if tuple(other) == (0, 0):
        out.add("seed_later")
    if tuple(first) == (0, 0):
        out.add("seed_earlier")
    return out


PAIR_CLASSES = (["same_row"] + [f"split_{R}" for R in SPLIT_ROWS] +
                ["groups", "chunks", "fold", "wrap", "seed_later", "seed_earlier"])


def pair_classes(cen):
    """Counter of pair_labels over the tied pairs (raster-first, other) of the
    unclamped blocks of a 16x16 +-32 census."""
    assert cen.cost.shape[1] == 2 * S + 1
    n = Counter()
    for f, by, bx in zip(*np.nonzero((cen.nmin > 1) & cen.unclamped[None])):
        m = minimisers(cen, f, by, bx)
        assert m[0] == tuple(cen.first[f, by, bx])
        for other in m[1:]:
            n.update(pair_labels(m[0], other))
    return n


# --------------------------------------------------------- live-list estimate
def live_estimate(ref, cur, cost):
    """Live lane-tasks per h = 16 item (4 blocks of a block row) of one frame:
    int [nby, ceil(nbx / 4)].  cost: sad_maps of the frame, [65, 65, nby, nbx]."""
    from test_gpu_sad_prune import box_q
    H, W = ref.shape
    nby, nbx = H // B, W // B
    qref, qcur = box_q(ref), box_q(cur)
    big = 1 << 30
    live = np.zeros((nby, (nbx + 3) // 4), np.int64)
    dys, dxs = np.mgrid[0:2 * S + 1, 0:2 * S + 1]
    chunk, row = dys // K, dys % K
    fold = dxs == 2 * S
    group = np.where(fold, row, dxs // 4)
    task = chunk * G + group
    order = (row * 8 + np.where(fold, 4, dxs % 4)) * 128 + chunk * G + group  # the bound's entry order at equal q-sums
    for by in range(nby):
        for bx in range(nbx):
            c = cost[:, :, by, bx].astype(np.int64)
            valid = c != INVALID
            y0, x0 = by * B - S, bx * B - S
            lb = np.zeros((2 * S + 1, 2 * S + 1), np.int64)
            iy, ix = np.nonzero(valid)
            for sy in range(4):
                for sx in range(4):
                    q = qcur[by * B + 4 * sy, bx * B + 4 * sx]
                    lb[iy, ix] += np.abs(qref[y0 + iy + 4 * sy, x0 + ix + 4 * sx] - q)
            lb = np.where(valid, lb, big)
            minlb = np.full(5 * G, big, np.int64)
            np.minimum.at(minlb, task.ravel(), lb.ravel())
            k = np.lexsort((order.ravel(), lb.ravel()))[0]  # the smallest bound, ties by the entry order
            ub = int(c.ravel()[k])
            if valid[S, S]:
                ub = min(ub, int(c[S, S]))
            live[by, bx // 4] += int(((minlb < big) & (16 * minlb - 240 <= ub)).sum())
    return live


def last_task_rows(live):
    """R of the last wave-task of a list of `live` entries (13: it runs whole)."""
    return split_rows(live - 64 * ((live - 1) // 64)) if live > 0 else 0


# ------------------------------------------- rate-constrained ties (J = SAD + lam R)
# (block size, range, frames of lat_small) of the partition and rate-constrained
# searches: the fast kernels' 16x16 at +-16 and +-32, the generic ones' 8x8.  At
# 8x8 only the (3, 3, 1) frame keeps a tie of J at lambda = 1000: a 64-pixel
# SAD gap does not outweigh the 12 bits the half-way candidate of a 23-pixel
# period saves, and a 3-pixel period has no integer half-way candidate.
RD_SHAPES = [(16, 16, (0, 1)), (16, 32, (0, 1)), (8, 16, (0,))]
RD_LAMBDAS = (0, 5, 1000)


def midpoint_pred(cen, f, width, height, blk):
    """Quarter-pel predictors int16 [nblocks, 2] of frame f: per tied full block
    p = 2 (d1 + d2), half way between the raster-first minimiser d1 and the tied
    partner d2 with the cheapest vector difference.  4 d1 - p = -(4 d2 - p) and
    bits(v) == bits(-v), so J(d1) == J(d2) at any lambda.  Other blocks: 0."""
    nbx_all, nby_all = -(-width // blk), -(-height // blk)
    pred = np.zeros((nby_all, nbx_all, 2), np.int16)
    for by, bx in zip(*np.nonzero(cen.nmin[f] > 1)):
        m = minimisers(cen, f, by, bx)
        d1 = np.array(m[0])
        rest = np.array(m[1:])
        d2 = rest[(rd_ref.bits(2 * (rest - d1))).sum(axis=1).argmin()]
        pred[by, bx] = 2 * (d1 + d2)
    return pred.reshape(-1, 2)


def j_ties(table, lam, pred):
    """Blocks (bool [nblocks]) whose minimum of J over their candidates is reached twice or more
    (table: rd_ref.sad_table)."""
    sad, valid = table
    n, _, nby, nbx = sad.shape
    span = (n - 1) // 2
    p = rd_ref._pred(pred, nbx * nby).reshape(nby, nbx, 2)
    d = np.arange(-span, span + 1, dtype=np.int64)
    ry = rd_ref.bits(4 * d[:, None, None] - p[None, :, :, 1])  # [dy, nby, nbx]
    rx = rd_ref.bits(4 * d[:, None, None] - p[None, :, :, 0])  # [dx, nby, nbx]
    r = ry[:, None] + rx[None, :]
    j = np.where(valid, sad + int(lam) * r, np.iinfo(np.int64).max)
    return ((j == j.min(axis=(0, 1))).sum(axis=(0, 1)) > 1).ravel()
