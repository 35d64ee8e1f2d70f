"""The case table of the VALU search kernels' envelope tests (numpy only).

include/me.h promises any block size 1..64 and any range 0..1024 on every
cost, bit for bit.  CASES below is what tests/test_gpu_valu_envelope.py runs
through me_full_search_device against the oracle, and what
tests/test_valu_envelope_cover.py proves, on the CPU, to reach every compiled
me_fast_kernel instance of launch_fast and every plan feature of plan_fast
(csrc/me_valu_plan.cpp, as oracle/plan_dump reports it for 256 CUs).

A case is a thin frame: one axis is 3 B + 2 S plus 0..B-1, so some block has an
unclipped window along it, the other about four blocks; both orientations
occur.  A thin 16x16 SAD frame is "small" to plan_fast up to S of about 130
(K = 5, refused from S of about 50 on, where the K = 5 tile leaves the LDS
budget), so the K = 13 / 11 / 8 instances of that family are reached at S >=
130 and, for the compiled pitch 272, on a 416 x 240 frame at S = 68.  The
planes are carved from larger buffers at the case's pitch and byte offsets;
`align` is the class (me_geom.h align_class) the case was planned with, K and
cpp the plan's chunk height and chunks per LDS pass (None: plan_fast refuses
the shape and the generic kernel, or a matrix-core kernel, runs).

Content kinds (deterministic from the case's seed):
  far_shift   box-filtered noise; every block of cur is the ref block displaced
              by one of the window's extremes (+-S, 0), (0, +-S), (S, S),
              (-S, -S) with +-2 jitter, clamped to the block's valid window,
              plus +-2 noise: winners in the fold column, the last group's
              padded columns, the first and last dy chunks and passes.
  two_copies  noise; chosen full blocks of cur occur exactly twice in ref, at
              cost 0, at (dx1, dy1) and (dx2, dy2) with (dy1, dx1) < (dy2, dx2):
                chunks     dy1 < dy2, dx1 > dx2, the window's opposite corners
                           (different dy chunks, and passes where the plan has
                           several)
                groups     equal dy, different 4-wide dx groups
                ingroup    equal dy, dx2 = dx1 + 1 inside one group
                fold_lo    (S - 1, d) against (+S, d)
                fold_wrap  (+S, d) against (-S, d + 1)
                fold_lane  (4 ((d + S) mod K) - S + i, d) against (+S, d): both
                           candidates of one lane of a fold plan (lane gi owns
                           group gi and the fold candidate of dy index gi)
              (overlapping copies, dx2 = dx1 + 1, use blocks with constant rows).
              The raster-first winner is (dx1, dy1); a kernel ordering ties by
              (dx, dy), or the fold column before its row's groups, or losing a
              tie across a chunk or a pass, picks the other copy.
  antidiag    ref[y, x] = f((x + y) mod 7), cur = ref: every candidate with
              dx + dy = 0 (mod 7) ties at cost 0.
  sat:ref0 / sat:ref255 / sat:random
              flat 0 against flat 255, the reverse, and random 0/255 planes:
              all-maximum costs (SAD B*B*255 = 0xFF00 at 16x16, next to the
              lane keys' invalid mark 0xFFFF) on blocks with masked candidates.

Oracle budget: a case costs me_candidate_count * B^2 / 256 <= 5e7 16x16
candidate equivalents (oracle_cost).  The slowest case, sad16_s1024_h (1.7e7),
took 0.57 s on 8 threads of the CPU reference (oracle/me_oracle.c) on the
development machine; the whole table 5.6 s, plus 0.7 s to draw its frames.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SSD, SAD = 0, 1
ALIGN_4, ALIGN_REF16, ALIGN_CUR16 = 1, 2, 4
ORACLE_BUDGET = 5e7
BASE_ALIGN = 256  # alignment of the buffers the planes are carved from

_F = "name width height stride ref_off cur_off blk range cost path content seed align K cpp"


class Case(namedtuple("Case", _F)):
    __slots__ = ()

    @property
    def kind(self):
        return self.content.split(":")[0]

    @property
    def cost_name(self):
        return "sad" if self.cost == SAD else "ssd"

    @property
    def expect_path(self):
        """The kernel family me_ctx_last_search_path must report."""
        if self.cost == SSD and self.blk == 8 and self.path == "auto" and self.range >= 1:
            return "mfma_8x8"
        return "valu"

    @property
    def nbx(self):
        return (self.width + self.blk - 1) // self.blk

    @property
    def nby(self):
        return (self.height + self.blk - 1) // self.blk


def align_class(stride, ref_addr, cur_addr):
    """me_geom.h align_class."""
    return ((ALIGN_4 if stride % 4 == 0 and ref_addr % 4 == 0 and cur_addr % 4 == 0 else 0)
            | (ALIGN_REF16 if stride % 16 == 0 and ref_addr % 16 == 0 else 0)
            | (ALIGN_CUR16 if cur_addr % 16 == 0 else 0))


def _axis(n, blk, rng):
    """(first pixel, size, lowest and highest valid displacement) of every block along one axis."""
    t = np.arange(0, n, blk)
    size = np.minimum(blk, n - t)
    return t, size, np.maximum(-rng, -t), np.minimum(rng, n - size - t)


def candidate_count(width, height, blk, rng):
    """me_candidate_count in closed form."""
    _, _, xlo, xhi = _axis(width, blk, rng)
    _, _, ylo, yhi = _axis(height, blk, rng)
    return int((xhi - xlo + 1).sum()) * int((yhi - ylo + 1).sum())


def oracle_cost(c):
    return candidate_count(c.width, c.height, c.blk, c.range) * c.blk * c.blk / 256.0


# ------------------------------------------------------------------ content
def _box3(a):
    p = np.pad(a.astype(np.int32), 1, mode="edge")
    h, w = a.shape
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((s + 4) // 9).astype(np.uint8)


_EXTREMES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1))


def _far_shift(c, rng):
    W, H, B, S = c.width, c.height, c.blk, c.range
    ref = _box3(rng.integers(0, 256, (H, W), dtype=np.uint8))
    cur = rng.integers(0, 256, (H, W), dtype=np.uint8)
    xs, ws, xlo, xhi = _axis(W, B, S)
    ys, hs, ylo, yhi = _axis(H, B, S)
    for by in range(len(ys)):
        for bx in range(len(xs)):
            ex, ey = _EXTREMES[(bx + 3 * by + c.seed) % 6]
            jx, jy = (int(v) * ((bx + by) % 2) for v in rng.integers(-2, 3, 2))  # every other block exact
            dx = int(np.clip(ex * S + jx, xlo[bx], xhi[bx]))
            dy = int(np.clip(ey * S + jy, ylo[by], yhi[by]))
            x, y, w, h = int(xs[bx]), int(ys[by]), int(ws[bx]), int(hs[by])
            src = ref[y + dy:y + dy + h, x + dx:x + dx + w].astype(np.int16)
            cur[y:y + h, x:x + w] = np.clip(src + rng.integers(-2, 3, (h, w)), 0, 255)
    return ref, cur


PAIR_KINDS = ("chunks", "groups", "ingroup", "fold_lo", "fold_wrap", "fold_lane")
Planted = namedtuple("Planted", "block bx by kind first second")


def _pair(kind, S, B, K, a, xlo, xhi, ylo, yhi, rng):
    """The two displacements of a pair of `kind` for a block with valid window
    [xlo, xhi] x [ylo, yhi], or None where the window has no room for it."""
    def dy_any(lo, hi):
        return int(rng.integers(lo, hi + 1)) if hi >= lo else None

    if kind == "chunks":
        if yhi - ylo < B and xhi - xlo < B or yhi == ylo or xhi == xlo:
            return None
        return (xhi, ylo), (xlo, yhi)
    if kind == "groups":
        d = dy_any(ylo, yhi)
        if d is None or xhi - xlo < B + 4:
            return None
        x1 = int(rng.integers(xlo, xhi - B - 3))
        x2 = int(rng.integers(x1 + max(B, 4), xhi + 1))
        return (x1, d), (x2, d)
    if kind == "ingroup":
        d = dy_any(ylo, yhi)
        # dx = 4 g + i - S - a: i of the first copy in 0..2
        xs = [x for x in range(xlo, xhi) if (x + S + a) % 4 < 3]
        if d is None or not xs:
            return None
        x1 = xs[int(rng.integers(0, len(xs)))]
        return (x1, d), (x1 + 1, d)
    if kind == "fold_lo":
        d = dy_any(ylo, yhi)
        if d is None or xhi != S or xlo > S - 1 or S < 1:
            return None
        return (S - 1, d), (S, d)
    if kind == "fold_wrap":
        d = dy_any(ylo, yhi - 1)
        if d is None or xhi != S or xlo != -S or 2 * S < B:
            return None
        return (S, d), (-S, d + 1)
    if kind == "fold_lane":
        # the lane that owns the fold candidate (+S, d), group gi = (d + S) mod K
        # (me_fast_kernel: jt = gi), against a candidate of that group
        d = dy_any(ylo, yhi)
        if d is None or K is None or a != 0 or xhi != S:
            return None
        x1 = 4 * ((d + S) % K) - S + int(rng.integers(0, 4))
        if x1 < xlo or S - x1 < B:
            return None
        return (x1, d), (S, d)
    raise ValueError(kind)


def _two_copies(c, rng):
    W, H, B, S = c.width, c.height, c.blk, c.range
    ref = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cur = rng.integers(0, 256, (H, W), dtype=np.uint8)
    used = np.zeros((H, W), bool)
    xs, ws, xlo, xhi = _axis(W, B, S)
    ys, hs, ylo, yhi = _axis(H, B, S)
    planted = []
    count = dict.fromkeys(PAIR_KINDS, 0)
    # Blocks with an unclipped window along x, then along y, first: only they
    # have room for the fold kinds and for dy chunks 2 S apart, and ref is
    # still free around them.
    order = sorted((not (xlo[bx] == -S and xhi[bx] == S), not (ylo[by] == -S and yhi[by] == S), by, bx)
                   for by in range(len(ys)) for bx in range(len(xs)) if ws[bx] == B and hs[by] == B)
    for _, _, by, bx in order:
        x, y = int(xs[bx]), int(ys[by])
        a = (x - S) % 4
        # the kind planted least often so far that fits (ties: the fold kinds first)
        for kind in sorted(PAIR_KINDS, key=lambda k: (count[k], -PAIR_KINDS.index(k))):
            pr = _pair(kind, S, B, c.K, a, int(xlo[bx]), int(xhi[bx]), int(ylo[by]), int(yhi[by]), rng)
            if pr is None:
                continue
            (x1, y1), (x2, y2) = pr
            overlap = abs(x1 - x2) < B and abs(y1 - y2) < B
            if overlap and not (y1 == y2 and abs(x1 - x2) == 1):
                continue
            # the union of the two copies must be untouched ref
            r0, r1 = y + min(y1, y2), y + max(y1, y2) + B
            c0, c1 = x + min(x1, x2), x + max(x1, x2) + B
            if overlap:
                if used[r0:r1, c0:c1].any():
                    continue
                rows = rng.integers(0, 256, (B, 1), dtype=np.uint8)
                blk = np.repeat(rows, B, axis=1)
                ref[r0:r1, c0:c1] = np.repeat(rows, B + 1, axis=1)
                used[r0:r1, c0:c1] = True
            else:
                if (used[y + y1:y + y1 + B, x + x1:x + x1 + B].any()
                        or used[y + y2:y + y2 + B, x + x2:x + x2 + B].any()):
                    continue
                blk = cur[y:y + B, x:x + B].copy()
                for (dx, dy) in pr:
                    ref[y + dy:y + dy + B, x + dx:x + dx + B] = blk
                    used[y + dy:y + dy + B, x + dx:x + dx + B] = True
            cur[y:y + B, x:x + B] = blk
            planted.append(Planted(by * len(xs) + bx, bx, by, kind, (x1, y1), (x2, y2)))
            count[kind] += 1
            break
    return ref, cur, planted


def _antidiag(c, rng):
    f = rng.permutation(256)[:7].astype(np.uint8)
    y, x = np.mgrid[0:c.height, 0:c.width]
    ref = f[(x + y) % 7]
    return ref, ref.copy()


def _sat(c, rng):
    shape = (c.height, c.width)
    which = c.content.split(":")[1]
    if which == "ref0":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    if which == "ref255":
        return np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)
    return ((rng.integers(0, 2, shape) * 255).astype(np.uint8),
            (rng.integers(0, 2, shape) * 255).astype(np.uint8))


def frames(c):
    """(ref, cur, planted): tight (H, W) uint8 planes of the case; planted is
    the list of Planted pairs of a two_copies case, else empty."""
    rng = np.random.default_rng(c.seed)
    if c.kind == "two_copies":
        ref, cur, planted = _two_copies(c, rng)
    else:
        ref, cur = {"far_shift": _far_shift, "antidiag": _antidiag, "sat": _sat}[c.kind](c, rng)
        planted = []
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur), planted


def column_first_search(ref, cur, blk, rng):
    """Full SAD search that keeps the first minimum in column-major order (dx
    outer, dy inner): what a kernel ordering ties by (dx, dy) would return."""
    H, W = ref.shape
    xs, ws, xlo, xhi = _axis(W, blk, rng)
    ys, hs, ylo, yhi = _axis(H, blk, rng)
    mv = np.zeros((len(ys) * len(xs), 2), np.int16)
    r = ref.astype(np.int32)
    for by in range(len(ys)):
        for bx in range(len(xs)):
            x, y, w, h = int(xs[bx]), int(ys[by]), int(ws[bx]), int(hs[by])
            cb = cur[y:y + h, x:x + w].astype(np.int32)
            win = r[y + ylo[by]:y + yhi[by] + h, x + xlo[bx]:x + xhi[bx] + w]
            ny, nx = yhi[by] - ylo[by] + 1, xhi[bx] - xlo[bx] + 1
            sad = np.zeros((ny, nx), np.int32)  # [dy index, dx index]
            for oy in range(h):
                for ox in range(w):
                    sad += np.abs(win[oy:oy + ny, ox:ox + nx] - cb[oy, ox])
            i = int(np.argmin(sad.T))  # first minimum, dx-major
            mv[by * len(xs) + bx] = (i // sad.shape[0] + xlo[bx], i % sad.shape[0] + ylo[by])
    return mv


# -------------------------------------------------------------------- table
def _c(name, width, height, stride, ref_off, cur_off, blk, rng, cost, path, content, seed, K, cpp):
    return Case(name, width, height, stride, ref_off, cur_off, blk, rng, cost, path, content, seed,
                align_class(stride, BASE_ALIGN + ref_off, BASE_ALIGN + cur_off), K, cpp)


# name, width, height, stride, ref and cur byte offsets, B, S, cost, path,
# content, seed, K, cpp  # oracle_cost in 1e6
CASES = [
    # -- a greedy cover of the plan features (tests/test_valu_envelope_cover.py) over thin frames
    _c("sad16_s1_50x64_far_shift", 50, 64, 53, 1, 3, 16, 1, SAD, "auto", "far_shift", 101, 5, 1),  # 0.0M
    _c("sad16_s1_50x64_antidiag", 50, 64, 53, 1, 3, 16, 1, SAD, "auto", "antidiag", 102, 5, 1),  # 0.0M
    _c("sad16_s1_50x64_sat_random", 50, 64, 53, 1, 3, 16, 1, SAD, "auto", "sat:random", 103, 5, 1),  # 0.0M
    _c("sad16_s1_58x56_two_copies", 58, 56, 61, 1, 3, 16, 1, SAD, "auto", "two_copies", 104, 5, 1),  # 0.0M
    _c("sad16_s61_16x170_far_shift", 16, 170, 32, 0, 0, 16, 61, SAD, "auto", "far_shift", 105, None, None),  # 0.0M
    _c("sad16_s68_416x240_far_shift", 416, 240, 432, 0, 0, 16, 68, SAD, "auto", "far_shift", 106, 13, 1),  # 5.4M
    _c("sad16_s68_416x240_two_copies", 416, 240, 432, 0, 0, 16, 68, SAD, "auto", "two_copies", 107, 13, 1),  # 5.4M
    _c("sad16_s70_416x240_sat_ref0", 416, 240, 432, 0, 0, 16, 70, SAD, "auto", "sat:ref0", 108, 13, 1),  # 5.7M
    _c("sad16_s140_336x51_two_copies", 336, 51, 352, 0, 0, 16, 140, SAD, "auto", "two_copies", 109, 13, 1),  # 0.7M
    _c("sad16_s140_336x51_antidiag", 336, 51, 352, 0, 0, 16, 140, SAD, "auto", "antidiag", 110, 13, 1),  # 0.7M
    _c("sad16_s143_334x51_far_shift", 334, 51, 336, 32, 4, 16, 143, SAD, "auto", "far_shift", 111, 13, 1),  # 0.7M
    _c("sad16_s152_352x51_far_shift", 352, 51, 356, 4, 8, 16, 152, SAD, "auto", "far_shift", 112, 8, 5),  # 0.8M
    _c("sad16_s152_352x51_two_copies", 352, 51, 356, 4, 8, 16, 152, SAD, "auto", "two_copies", 113, 8, 5),  # 0.8M
    _c("sad16_s152_352x51_sat_ref255", 352, 51, 356, 4, 8, 16, 152, SAD, "auto", "sat:ref255", 114, 8, 5),  # 0.8M
    _c("sad16_s163_64x374_far_shift", 64, 374, 68, 4, 8, 16, 163, SAD, "auto", "far_shift", 115, 11, 3),  # 1.2M
    _c("sad16_s163_64x374_antidiag", 64, 374, 68, 4, 8, 16, 163, SAD, "auto", "antidiag", 116, 11, 3),  # 1.2M
    _c("sad16_s164_64x376_two_copies", 64, 376, 64, 32, 4, 16, 164, SAD, "auto", "two_copies", 117, 11, 3),  # 1.2M
    _c("sad16_s224_496x51_antidiag", 496, 51, 512, 0, 0, 16, 224, SAD, "auto", "antidiag", 118, 8, 2),  # 1.7M
    _c("sad8_s3_8x30_far_shift", 8, 30, 32, 0, 0, 8, 3, SAD, "auto", "far_shift", 119, 8, 1),  # 0.0M
    _c("sad8_s3_30x32_far_shift", 30, 32, 48, 0, 0, 8, 3, SAD, "auto", "far_shift", 120, 8, 1),  # 0.0M
    _c("sad8_s3_30x32_sat_random", 30, 32, 48, 0, 0, 8, 3, SAD, "auto", "sat:random", 121, 8, 1),  # 0.0M
    _c("sad8_s16_56x27_far_shift", 56, 27, 80, 0, 0, 8, 16, SAD, "auto", "far_shift", 122, 11, 3),  # 0.0M
    _c("sad8_s16_56x27_antidiag", 56, 27, 80, 0, 0, 8, 16, SAD, "auto", "antidiag", 123, 11, 3),  # 0.0M
    _c("sad8_s17_58x27_two_copies", 58, 27, 61, 1, 3, 8, 17, SAD, "auto", "two_copies", 124, 13, 3),  # 0.0M
    _c("sad8_s17_58x27_antidiag", 58, 27, 61, 1, 3, 8, 17, SAD, "auto", "antidiag", 125, 13, 3),  # 0.0M
    _c("sad8_s20_64x27_two_copies", 64, 27, 64, 32, 4, 8, 20, SAD, "auto", "two_copies", 126, 8, 6),  # 0.0M
    _c("sad8_s20_64x27_sat_ref255", 64, 27, 64, 32, 4, 8, 20, SAD, "auto", "sat:ref255", 127, 8, 6),  # 0.0M
    _c("sad8_s24_72x27_sat_ref0", 72, 27, 76, 4, 8, 8, 24, SAD, "auto", "sat:ref0", 128, 26, 2),  # 0.0M
    _c("sad8_s24_72x27_far_shift", 72, 27, 76, 4, 8, 8, 24, SAD, "auto", "far_shift", 129, 26, 2),  # 0.0M
    _c("sad8_s24_72x27_two_copies", 72, 27, 76, 4, 8, 8, 24, SAD, "auto", "two_copies", 130, 26, 2),  # 0.0M
    _c("sad8_s24_72x27_antidiag", 72, 27, 76, 4, 8, 8, 24, SAD, "auto", "antidiag", 131, 26, 2),  # 0.0M
    _c("sad8_s32_91x28_far_shift", 91, 28, 95, 1, 3, 8, 32, SAD, "auto", "far_shift", 132, 13, 5),  # 0.0M
    _c("sad8_s35_27x94_two_copies", 27, 94, 32, 32, 4, 8, 35, SAD, "auto", "two_copies", 133, 11, 4),  # 0.0M
    _c("sad8_s112_32x248_antidiag", 32, 248, 48, 0, 0, 8, 112, SAD, "auto", "antidiag", 134, 8, 9),  # 0.1M
    _c("sad8_s116_264x27_two_copies", 264, 27, 272, 32, 4, 8, 116, SAD, "auto", "two_copies", 135, 13, 2),  # 0.1M
    _c("sad8_s129_282x27_far_shift", 282, 27, 292, 4, 8, 8, 129, SAD, "auto", "far_shift", 136, 13, 3),  # 0.1M
    _c("sad8_s141_27x306_two_copies", 27, 306, 48, 0, 0, 8, 141, SAD, "auto", "two_copies", 137, 26, 1),  # 0.2M
    _c("sad8_s142_27x308_far_shift", 27, 308, 31, 1, 3, 8, 142, SAD, "auto", "far_shift", 138, 26, 1),  # 0.2M
    _c("ssd16_s1_16x50_far_shift", 16, 50, 32, 0, 0, 16, 1, SSD, "valu", "far_shift", 139, 8, 1),  # 0.0M
    _c("ssd16_s1_50x64_far_shift", 50, 64, 53, 1, 3, 16, 1, SSD, "valu", "far_shift", 140, 8, 1),  # 0.0M
    _c("ssd16_s1_50x64_antidiag", 50, 64, 53, 1, 3, 16, 1, SSD, "valu", "antidiag", 141, 8, 1),  # 0.0M
    _c("ssd16_s1_50x64_sat_ref0", 50, 64, 53, 1, 3, 16, 1, SSD, "valu", "sat:ref0", 142, 8, 1),  # 0.0M
    _c("ssd16_s9_80x66_antidiag", 80, 66, 96, 0, 0, 16, 9, SSD, "valu", "antidiag", 143, 11, 2),  # 0.0M
    _c("ssd16_s11_70x51_far_shift", 70, 51, 96, 0, 0, 16, 11, SSD, "valu", "far_shift", 144, 13, 2),  # 0.0M
    _c("ssd16_s11_70x51_two_copies", 70, 51, 96, 0, 0, 16, 11, SSD, "valu", "two_copies", 145, 13, 2),  # 0.0M
    _c("ssd16_s14_51x76_two_copies", 51, 76, 80, 0, 0, 16, 14, SSD, "valu", "two_copies", 146, 8, 4),  # 0.0M
    _c("ssd16_s17_51x82_two_copies", 51, 82, 56, 4, 8, 16, 17, SSD, "valu", "two_copies", 147, 11, 2),  # 0.0M
    _c("ssd16_s20_51x88_far_shift", 51, 88, 55, 1, 3, 16, 20, SSD, "valu", "far_shift", 148, 11, 2),  # 0.0M
    _c("ssd16_s32_80x112_antidiag", 80, 112, 96, 0, 0, 16, 32, SSD, "valu", "antidiag", 149, 13, 3),  # 0.1M
    _c("ssd8_s1_8x26_far_shift", 8, 26, 12, 4, 8, 8, 1, SSD, "valu", "far_shift", 150, 8, 1),  # 0.0M
    _c("ssd8_s1_26x32_far_shift", 26, 32, 48, 0, 0, 8, 1, SSD, "valu", "far_shift", 151, 8, 1),  # 0.0M
    _c("ssd8_s1_26x32_antidiag", 26, 32, 48, 0, 0, 8, 1, SSD, "valu", "antidiag", 152, 8, 1),  # 0.0M
    _c("ssd8_s1_26x32_sat_ref0", 26, 32, 48, 0, 0, 8, 1, SSD, "valu", "sat:ref0", 153, 8, 1),  # 0.0M
    _c("ssd8_s8_48x27_far_shift", 48, 27, 51, 1, 3, 8, 8, SSD, "valu", "far_shift", 154, 11, 2),  # 0.0M
    _c("ssd8_s11_46x27_two_copies", 46, 27, 64, 0, 0, 8, 11, SSD, "valu", "two_copies", 155, 13, 2),  # 0.0M
    _c("ssd8_s11_46x27_antidiag", 46, 27, 64, 0, 0, 8, 11, SSD, "valu", "antidiag", 156, 13, 2),  # 0.0M
    _c("ssd8_s14_27x52_two_copies", 27, 52, 36, 4, 8, 8, 14, SSD, "valu", "two_copies", 157, 8, 4),  # 0.0M
    _c("ssd8_s17_27x58_two_copies", 27, 58, 31, 1, 3, 8, 17, SSD, "valu", "two_copies", 158, 11, 2),  # 0.0M
    _c("ssd8_s17_58x27_far_shift", 58, 27, 61, 1, 3, 8, 17, SSD, "valu", "far_shift", 159, 13, 1),  # 0.0M
    _c("ssd8_s208_32x440_antidiag", 32, 440, 48, 0, 0, 8, 208, SSD, "valu", "antidiag", 160, 11, 3),  # 0.4M
    # -- instances no test launched before: <SAD,16,11>, <SAD,16,8>, <SAD,16,13> multi-pass
    # at a runtime pitch, <SAD,8,26,336> with the fold
    _c("sad16_s130_k11", 313, 72, 313, 0, 0, 16, 130, SAD, "auto", "two_copies", 161, 11, 3),  # 1.2M
    _c("sad16_s132_k8", 317, 72, 317, 0, 0, 16, 132, SAD, "auto", "far_shift", 162, 8, 3),  # 1.2M
    _c("sad16_s135_multipass", 323, 72, 323, 0, 0, 16, 135, SAD, "auto", "two_copies", 163, 13, 1),  # 1.3M
    _c("sad8_s148_k26p336_fold", 320, 32, 320, 0, 0, 8, 148, SAD, "auto", "two_copies", 164, 26, 2),  # 0.2M
    # -- the planner's refusals (generic kernel): S = 0, S = 256
    _c("sad16_s0", 70, 45, 96, 0, 0, 16, 0, SAD, "auto", "far_shift", 165, None, None),  # 0.0M
    _c("ssd8_s0_valu", 45, 35, 49, 1, 3, 8, 0, SSD, "valu", "sat:random", 166, None, None),  # 0.0M
    _c("ssd16_s0_auto", 70, 45, 76, 4, 8, 16, 0, SSD, "auto", "far_shift", 167, None, None),  # 0.0M
    _c("sad16_s256", 565, 56, 592, 0, 0, 16, 256, SAD, "auto", "two_copies", 168, None, None),  # 2.4M
    _c("sad8_s256", 36, 539, 40, 4, 8, 8, 256, SAD, "auto", "far_shift", 169, None, None),  # 1.0M
    _c("ssd16_s256_valu", 60, 567, 64, 32, 4, 16, 256, SSD, "valu", "two_copies", 170, None, None),  # 2.6M
    _c("ssd8_s256_valu", 541, 28, 545, 1, 3, 8, 256, SSD, "valu", "antidiag", 171, None, None),  # 0.6M
    # -- 16x16 SSD past the matrix-core kernels' S = 192 on the automatic path (VALU dot4)
    _c("ssd16_s193_auto", 439, 72, 464, 0, 0, 16, 193, SSD, "auto", "far_shift", 172, 13, 1),  # 2.4M
    _c("ssd16_s224_auto", 496, 56, 496, 32, 4, 16, 224, SSD, "auto", "two_copies", 173, 8, 3),  # 1.8M
    _c("ssd16_s255_auto", 567, 67, 572, 4, 8, 16, 255, SSD, "auto", "antidiag", 174, 13, 1),  # 3.8M
    # -- the 8x8 matrix-core kernel past S = 128 (H % 8 == 0: a partial bottom row would end
    # the search on the VALU kernels, which would then be the family reported)
    _c("ssd8_s129_mfma", 32, 288, 48, 0, 0, 8, 129, SSD, "auto", "far_shift", 175, None, None),  # 0.2M
    _c("ssd8_s200_mfma", 427, 32, 436, 4, 8, 8, 200, SSD, "auto", "two_copies", 176, None, None),  # 0.4M
    _c("ssd8_s256_mfma", 37, 536, 44, 4, 8, 8, 256, SSD, "auto", "antidiag", 177, None, None),  # 1.0M
    _c("ssd8_s600_mfma", 1229, 32, 1248, 0, 0, 8, 600, SSD, "auto", "two_copies", 178, None, None),  # 3.5M
    _c("ssd8_s1024_mfma", 2080, 24, 2080, 32, 4, 8, 1024, SSD, "auto", "far_shift", 179, None, None),  # 5.1M
    # -- SAD past the item kernel's S = 255 (generic kernel), up to ME_MAX_RANGE
    _c("sad16_s257", 52, 565, 56, 4, 8, 16, 257, SAD, "auto", "far_shift", 180, None, None),  # 2.2M
    _c("sad16_s600_h", 1255, 56, 1259, 1, 3, 16, 600, SAD, "auto", "two_copies", 181, None, None),  # 12.3M
    _c("sad16_s1024_h", 2100, 40, 2128, 0, 0, 16, 1024, SAD, "auto", "far_shift", 182, None, None),  # 16.9M
    _c("sad8_s257", 543, 28, 560, 0, 0, 8, 257, SAD, "auto", "sat:ref0", 183, None, None),  # 0.6M
    _c("sad8_s600_v", 28, 1227, 32, 32, 4, 8, 600, SAD, "auto", "far_shift", 184, None, None),  # 3.1M
    _c("sad8_s1024_h", 2075, 20, 2084, 4, 8, 8, 1024, SAD, "auto", "two_copies", 185, None, None),  # 4.3M
    # -- block sizes 33..64 with partial edge blocks (generic kernel; SSD: the float-MSE replay)
    _c("sad33_s9", 122, 77, 125, 1, 3, 33, 9, SAD, "auto", "far_shift", 186, None, None),  # 0.0M
    _c("ssd33_s9", 122, 77, 144, 0, 0, 33, 9, SSD, "auto", "two_copies", 187, None, None),  # 0.0M
    _c("sad48_s20", 189, 112, 193, 1, 3, 48, 20, SAD, "auto", "far_shift", 188, None, None),  # 0.1M
    _c("ssd48_s20", 189, 112, 208, 0, 0, 48, 20, SSD, "auto", "two_copies", 189, None, None),  # 0.1M
    _c("sad63_s31", 256, 147, 259, 1, 3, 63, 31, SAD, "auto", "far_shift", 190, None, None),  # 0.4M
    _c("ssd63_s31", 256, 147, 272, 0, 0, 63, 31, SSD, "auto", "two_copies", 191, None, None),  # 0.4M
    _c("sad64_s24", 245, 149, 249, 1, 3, 64, 24, SAD, "auto", "far_shift", 192, None, None),  # 0.2M
    _c("ssd64_s24", 245, 149, 272, 0, 0, 64, 24, SSD, "auto", "two_copies", 193, None, None),  # 0.2M
    _c("sad64_s20_sat", 145, 94, 152, 4, 8, 64, 20, SAD, "auto", "sat:ref255", 194, None, None),  # 0.1M
    _c("ssd64_s12_sat", 145, 94, 160, 32, 4, 64, 12, SSD, "auto", "sat:ref0", 195, None, None),  # 0.0M
    _c("ssd48_s10_antidiag", 107, 68, 128, 0, 0, 48, 10, SSD, "auto", "antidiag", 196, None, None),  # 0.0M
    # -- each side of the generic kernel's window staging boundary,
    # (B + 2 S)^2 + B^2 <= GENERIC_LDS_BUDGET: S = 87 | 88 at B = 64, S = 115 | 116 at B = 16
    # (16x16 SAD: the partial right column and bottom row the item kernel leaves)
    _c("sad64_s87_staged", 371, 366, 400, 0, 0, 64, 87, SAD, "auto", "far_shift", 197, None, None),  # 10.6M
    _c("sad64_s88_global", 373, 368, 380, 4, 8, 64, 88, SAD, "auto", "two_copies", 198, None, None),  # 10.9M
    _c("ssd64_s87_staged", 366, 375, 369, 1, 3, 64, 87, SSD, "auto", "two_copies", 199, None, None),  # 10.7M
    _c("ssd64_s88_global", 371, 371, 400, 0, 0, 64, 88, SSD, "auto", "far_shift", 200, None, None),  # 10.9M
    _c("sad16_s115_staged", 283, 281, 304, 0, 0, 16, 115, SAD, "auto", "far_shift", 201, 13, 2),  # 10.1M
    _c("sad16_s116_global", 285, 283, 292, 4, 8, 16, 116, SAD, "auto", "two_copies", 202, 13, 2),  # 10.3M
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
