"""numpy restatement of the rate-constrained partition search (include/me.h
"rate-constrained partition search").

Grids, partitions, candidate displacements and storage order are
partition_ref's; bits() is rd_ref's.  With one quarter-pel predictor (px, py)
per macroblock,

    R_b(d)  = bits(4 dx - px) + bits(4 dy - py)
    J_p(d)  = SAD_p(d) + lam * R_b(d)          for each of the nine partitions
    J(m)    = sum of the winners' J_p over shape m's partitions + lam * MBITS[m]

Two forms of the same definition:
  search_loops  the definition's own loops: per macroblock, per displacement in
                raster order, J of each clipped partition; strict < keeps the
                first minimum.
  search_frame  per displacement over the whole frame: one |cur - ref(+d)|
                plane and its quadrant sums on the h grid (quad_table), then for
                every cell the first minimum of J over the displacements its
                macroblock has among its candidates, in raster order.  The
                table serves every lambda and predictor.
search_macroblock is search_loops for one macroblock, for spot checks of large
frames.  decide() is the mode decision from the records alone; the leaf field is
partition_ref.leaf_field.  Results are Fields: partition_ref.Fields (cost = J)
plus dist (SAD) and bits (R) lists in the order 2Nx2N, 2NxN, Nx2N, NxN.
"""
import numpy as np

import partition_ref as P
from rd_ref import bits

MBITS = (1, 3, 3, 5)  # ue(m) code length of mode m
REP = ((1, 1), (1, 2), (2, 1), (2, 2))  # cells per macroblock (x, y) of each grid


class Fields(P.Fields):
    def __init__(self, w, h, B):
        super().__init__(w, h, B)
        n = P.counts(w, h, B)
        self.dist = [np.zeros(k, np.uint32) for k in n]
        self.bits = [np.zeros(k, np.uint8) for k in n]


def _pred(pred, n):
    if pred is None:
        return np.zeros((n, 2), np.int64)
    return np.asarray(pred).reshape(n, 2).astype(np.int64)


def search_loops(ref, cur, B, S, lam=0, pred=None):
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    F = Fields(W, H, B)
    g = P.grids(W, H, B)
    pq = _pred(pred, g[0][0] * g[0][1])
    for by in range(g[0][1]):
        for bx in range(g[0][0]):
            x0, y0 = bx * B, by * B
            bw, bh = min(B, W - x0), min(B, H - y0)
            dx0, dx1 = P._window(x0, bw, W, S)
            dy0, dy1 = P._window(y0, bh, H, S)
            px, py = (int(v) for v in pq[by * g[0][0] + bx])
            parts = P._partitions(B, bw, bh)
            best = [None] * len(parts)
            blk = cur[y0:y0 + bh, x0:x0 + bw]
            for dy in range(dy0, dy1 + 1):
                for dx in range(dx0, dx1 + 1):
                    d = np.abs(blk - ref[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw])
                    r = int(bits(4 * dx - px)) + int(bits(4 * dy - py))
                    for n, (_, _, _, qx, qy, qw, qh) in enumerate(parts):
                        c = int(d[qy:qy + qh, qx:qx + qw].sum())
                        j = c + int(lam) * r
                        if best[n] is None or j < best[n][0]:
                            best[n] = (j, c, r, dx, dy)
            for (gi, i, j, *_), (jj, c, r, dx, dy) in zip(parts, best):
                sx, sy = REP[gi]
                cell = (sy * by + j) * g[gi][0] + sx * bx + i
                F.mv[gi][cell] = (dx, dy)
                F.cost[gi][cell], F.dist[gi][cell], F.bits[gi][cell] = jj, c, r
    return decide(F, lam)


def search_macroblock(ref, cur, B, S, lam, pred_b, bx, by):
    """search_loops for the one macroblock (bx, by), its candidates at once:
    ({(grid, cell): ((dx, dy), J, D, R)} over its non-empty partitions, mode,
    mode_cost).  pred_b: the macroblock's (px, py) or None.  For spot checks of
    frames too large for the other forms."""
    ref = np.asarray(ref, np.uint8)
    cur = np.asarray(cur, np.uint8)
    H, W = cur.shape
    g = P.grids(W, H, B)
    x0, y0 = bx * B, by * B
    bw, bh = min(B, W - x0), min(B, H - y0)
    dx0, dx1 = P._window(x0, bw, W, S)
    dy0, dy1 = P._window(y0, bh, H, S)
    px, py = (0, 0) if pred_b is None else (int(pred_b[0]), int(pred_b[1]))
    win = ref[y0 + dy0:y0 + dy1 + bh, x0 + dx0:x0 + dx1 + bw].astype(np.int32)
    v = np.lib.stride_tricks.sliding_window_view(win, (bh, bw))  # [dy, dx, bh, bw]
    d = np.abs(v - cur[y0:y0 + bh, x0:x0 + bw].astype(np.int32))
    r = bits(4 * np.arange(dy0, dy1 + 1) - py)[:, None] + bits(4 * np.arange(dx0, dx1 + 1) - px)[None, :]
    rec, J = {}, [int(lam) * m for m in MBITS]
    for gi, i, j, qx, qy, qw, qh in P._partitions(B, bw, bh):
        sad = d[:, :, qy:qy + qh, qx:qx + qw].sum(axis=(2, 3)).astype(np.int64)
        cost = sad + int(lam) * r
        k = int(cost.argmin())  # raster order: the first minimum
        iy, ix = divmod(k, cost.shape[1])
        sx, sy = REP[gi]
        rec[(gi, (sy * by + j) * g[gi][0] + sx * bx + i)] = (
            (dx0 + ix, dy0 + iy), int(cost[iy, ix]), int(sad[iy, ix]), int(r[iy, ix]))
        J[gi] += int(cost[iy, ix])
    mode = min(range(4), key=lambda m: (J[m], m))
    return rec, mode, J[mode]


def quad_table(ref, cur, B, S):
    """(q int64 [2S+1, 2S+1, 2 nby, 2 nbx], valid bool [2S+1, 2S+1, nby, nbx]):
    the SAD of every h x h quadrant at every displacement (dy, dx) of the
    window, pixels beyond the frame counting nothing, and whether the
    macroblock has that displacement among its candidates.  It depends on
    neither lambda nor the predictor: compute it once per frame pair."""
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    hb = B // 2
    nbx, nby = P.grids(W, H, B)[0]
    wx = np.array([P._window(bx * B, min(B, W - bx * B), W, S) for bx in range(nbx)])
    wy = np.array([P._window(by * B, min(B, H - by * B), H, S) for by in range(nby)])
    PH, PW = nby * B, nbx * B  # the frame padded to whole macroblocks
    pad = np.zeros((PH + 2 * S, PW + 2 * S), np.int32)
    pad[S:S + H, S:S + W] = ref
    curp = np.zeros((PH, PW), np.int32)
    curp[:H, :W] = cur
    inside = np.zeros((PH, PW), bool)
    inside[:H, :W] = True
    n = 2 * S + 1
    q = np.zeros((n, n, 2 * nby, 2 * nbx), np.int64)
    valid = np.zeros((n, n, nby, nbx), bool)
    for dy in range(-S, S + 1):
        vy = (wy[:, 0] <= dy) & (dy <= wy[:, 1])
        if not vy.any():
            continue
        for dx in range(-S, S + 1):
            v = vy[:, None] & ((wx[:, 0] <= dx) & (dx <= wx[:, 1]))[None, :]
            if not v.any():
                continue
            d = np.abs(curp - pad[S + dy:S + dy + PH, S + dx:S + dx + PW])
            d[~inside] = 0  # pixels beyond the frame belong to no partition
            q[dy + S, dx + S] = d.reshape(2 * nby, hb, 2 * nbx, hb).sum(axis=(1, 3))
            valid[dy + S, dx + S] = v
    return q, valid


def search_frame(ref, cur, B, S, lam=0, pred=None, table=None):
    """table: quad_table(ref, cur, B, S), when the caller has it already."""
    H, W = np.asarray(cur).shape
    q, valid = table if table is not None else quad_table(ref, cur, B, S)
    n, _, nby, nbx = valid.shape
    p = _pred(pred, nbx * nby).reshape(nby, nbx, 2)
    d = np.arange(-S, S + 1, dtype=np.int64)
    rx = bits(4 * d[:, None, None] - p[None, :, :, 0])  # [dx, nby, nbx]
    ry = bits(4 * d[:, None, None] - p[None, :, :, 1])  # [dy, nby, nbx]
    r = ry[:, None] + rx[None, :]                        # [dy, dx, nby, nbx]
    c = (q.reshape(n, n, nby, 2, nbx, 2).sum(axis=(3, 5)),   # 2Nx2N
         q.reshape(n, n, 2 * nby, nbx, 2).sum(axis=4),        # 2NxN
         q.reshape(n, n, nby, 2, 2 * nbx).sum(axis=3),        # Nx2N
         q)                                                   # NxN
    F = Fields(W, H, B)
    for k, (nx, ny) in enumerate(P.grids(W, H, B)):
        sx, sy = REP[k]
        cells = lambda a: np.repeat(np.repeat(a, sy, axis=2), sx, axis=3)[:, :, :ny, :nx]
        sad, rk = c[k][:, :, :ny, :nx], cells(r)
        j = np.where(cells(valid), sad + int(lam) * rk, np.iinfo(np.int64).max)
        # candidates in raster order (dy outer, dx inner); argmin keeps the first minimum
        win = j.reshape(n * n, ny * nx).argmin(axis=0)
        col = np.arange(ny * nx)
        pick = lambda a: a.reshape(n * n, ny * nx)[win, col]
        F.mv[k][:, 0] = win % n - S
        F.mv[k][:, 1] = win // n - S
        F.cost[k][:], F.dist[k][:], F.bits[k][:] = pick(j), pick(sad), pick(rk)
    return decide(F, lam)


def _per_macroblock(F, arrs):
    """[4] arrays [nby, nbx]: per shape, the sum of arrs[k] over the
    macroblock's non-empty partitions (missing ones add 0)."""
    g = P.grids(F.w, F.h, F.B)
    nbx, nby = g[0]
    out = []
    for k, (nx, ny) in enumerate(g):
        sx, sy = REP[k]
        p = np.zeros((sy * nby, sx * nbx), np.int64)
        p[:ny, :nx] = np.asarray(arrs[k]).reshape(ny, nx)
        out.append(p.reshape(nby, sy, nbx, sx).sum(axis=(1, 3)))
    return out


def decide(F, lam):
    """F's records with the mode / mode_cost of every macroblock at lambda =
    lam (the lambda the records were searched with): a new Fields sharing F's
    arrays; F is not changed."""
    J = [s + MBITS[k] * int(lam) for k, s in enumerate(_per_macroblock(F, F.cost))]
    best, mode = J[0].copy(), np.zeros(J[0].shape, np.uint8)
    for k in (1, 2, 3):
        upd = J[k] < best
        best[upd] = J[k][upd]
        mode[upd] = k
    out = Fields.__new__(Fields)
    out.w, out.h, out.B = F.w, F.h, F.B
    out.mv, out.cost, out.dist, out.bits = F.mv, F.cost, F.dist, F.bits
    out.mode = mode.reshape(-1)
    out.mode_cost = best.reshape(-1).astype(np.uint32)
    return out


def chosen(F, arrs):
    """int64 [macroblocks]: the sum of arrs over the partitions of each
    macroblock's chosen mode."""
    s = np.stack([a.reshape(-1) for a in _per_macroblock(F, arrs)])
    return s[np.asarray(F.mode, np.int64), np.arange(s.shape[1])]


def summary(F, lam):
    """(mode histogram [4], sum J(mode), sum dist and sum bits over the chosen
    modes' partitions).  sum J = sum dist + lam * (sum bits + sum MBITS[mode])."""
    hist = np.bincount(F.mode, minlength=4)
    return (hist.tolist(), int(F.mode_cost.astype(np.int64).sum()),
            int(chosen(F, F.dist).sum()), int(chosen(F, F.bits).sum()))
