"""numpy restatement of the rate-constrained search and refinement
(include/me.h "rate-constrained motion search").

    bits(v) = 2 floor(log2(2 |v| + 1)) + 1          (signed exp-Golomb length)
    R(d)    = bits(4 dx - px) + bits(4 dy - py)      (p: quarter-pel predictor)
    J(d)    = SAD(d) + lam * R(d)

Two forms of the integer search:
  search_loops  the definition's own loops: per block, per displacement in
                raster order; strict < keeps the first minimum of J.
  search_frame  per displacement over the whole frame: one |cur - ref(+d)|
                plane and its block sums (sad_table), then for every block the
                first minimum of J over the displacements it has among its
                candidates, in raster order.  Fast enough for +-32 on a small
                frame, and the table serves every lambda and predictor.
Both return (mv int16 [n, 2], J uint32 [n], D uint32 [n], R uint8 [n]);
search_block is search_loops for one block, for spot checks of large frames.
refine() is qpel_ref.refine with lam * (bits(qx - px) + bits(qy - py)) added to
every candidate's cost; it returns (q int16 [n, 2], Jq uint32 [n], D uint32 [n]).
"""
import numpy as np

import qpel_ref


def bits(v):
    """Code length of v (int or integer array), exact integers."""
    u = 2 * np.abs(np.asarray(v, np.int64)) + 1
    n = np.zeros(u.shape, np.int64)  # floor(log2(u))
    for s in (32, 16, 8, 4, 2, 1):
        big = (u >> s) > 0
        n = n + np.where(big, s, 0)
        u = np.where(big, u >> s, u)
    return 2 * n + 1


def _pred(pred, n):
    if pred is None:
        return np.zeros((n, 2), np.int64)
    return np.asarray(pred).reshape(n, 2).astype(np.int64)


def _window(x0, bw, W, S):
    """Displacements of a block along one axis: [lo, hi] (me_full_search's)."""
    return max(0, x0 - S) - x0, min(W, x0 + bw + S) - bw - x0


def search_loops(ref, cur, B, S, lam=0, pred=None):
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    nbx, nby = -(-W // B), -(-H // B)
    n = nbx * nby
    p = _pred(pred, n)
    mv = np.zeros((n, 2), np.int16)
    J, D, R = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for by in range(nby):
        for bx in range(nbx):
            b = by * nbx + bx
            x0, y0 = bx * B, by * B
            bw, bh = min(B, W - x0), min(B, H - y0)
            dx0, dx1 = _window(x0, bw, W, S)
            dy0, dy1 = _window(y0, bh, H, S)
            blk = cur[y0:y0 + bh, x0:x0 + bw]
            best = None
            for dy in range(dy0, dy1 + 1):
                for dx in range(dx0, dx1 + 1):
                    d = int(np.abs(blk - ref[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw]).sum())
                    r = int(bits(4 * dx - p[b, 0])) + int(bits(4 * dy - p[b, 1]))
                    j = d + int(lam) * r
                    if best is None or j < best[0]:
                        best = (j, d, r, dx, dy)
            J[b], D[b], R[b] = best[:3]
            mv[b] = best[3:]
    return mv, J, D, R


def search_block(ref, cur, B, S, lam, pred_b, bx, by):
    """search_loops for the one block (bx, by), its candidates at once:
    ((dx, dy), J, D, R).  pred_b: the block's (px, py) or None.  For spot checks
    of frames too large for the other forms."""
    ref = np.asarray(ref, np.uint8)
    cur = np.asarray(cur, np.uint8)
    H, W = cur.shape
    x0, y0 = bx * B, by * B
    bw, bh = min(B, W - x0), min(B, H - y0)
    dx0, dx1 = _window(x0, bw, W, S)
    dy0, dy1 = _window(y0, bh, H, S)
    px, py = (0, 0) if pred_b is None else (int(pred_b[0]), int(pred_b[1]))
    win = ref[y0 + dy0:y0 + dy1 + bh, x0 + dx0:x0 + dx1 + bw].astype(np.int32)
    v = np.lib.stride_tricks.sliding_window_view(win, (bh, bw))  # [dy, dx, bh, bw]
    sad = np.abs(v - cur[y0:y0 + bh, x0:x0 + bw].astype(np.int32)).sum(axis=(2, 3)).astype(np.int64)
    r = bits(4 * np.arange(dy0, dy1 + 1) - py)[:, None] + bits(4 * np.arange(dx0, dx1 + 1) - px)[None, :]
    j = sad + int(lam) * r
    k = int(j.argmin())  # raster order: the first minimum
    iy, ix = divmod(k, j.shape[1])
    return (dx0 + ix, dy0 + iy), int(j[iy, ix]), int(sad[iy, ix]), int(r[iy, ix])


def sad_table(ref, cur, B, S):
    """(sad int64 [2S+1, 2S+1, nby, nbx], valid bool of that shape): the SAD of
    every block at every displacement (dy, dx) of the window, and whether the
    block has that displacement among its candidates.  One |cur - ref(+d)|
    plane and its block sums per displacement.  It depends on neither lambda
    nor the predictor: compute it once per frame pair and pass it on."""
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    nbx, nby = -(-W // B), -(-H // B)
    wx = np.array([_window(bx * B, min(B, W - bx * B), W, S) for bx in range(nbx)])
    wy = np.array([_window(by * B, min(B, H - by * B), H, S) for by in range(nby)])
    PH, PW = nby * B, nbx * B  # the frame padded to whole blocks
    pad = np.zeros((PH + 2 * S, PW + 2 * S), np.int32)
    pad[S:S + H, S:S + W] = ref
    curp = np.zeros((PH, PW), np.int32)
    curp[:H, :W] = cur
    inside = np.zeros((PH, PW), bool)
    inside[:H, :W] = True
    n = 2 * S + 1
    sad = np.zeros((n, n, nby, nbx), np.int64)
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
            d[~inside] = 0  # pixels beyond the frame belong to no block
            sad[dy + S, dx + S] = d.reshape(nby, B, nbx, B).sum(axis=(1, 3))
            valid[dy + S, dx + S] = v
    return sad, valid


def search_frame(ref, cur, B, S, lam=0, pred=None, table=None):
    """table: sad_table(ref, cur, B, S), when the caller has it already."""
    sad, valid = table if table is not None else sad_table(ref, cur, B, S)
    n, _, nby, nbx = sad.shape
    p = _pred(pred, nbx * nby).reshape(nby, nbx, 2)
    d = np.arange(-S, S + 1, dtype=np.int64)
    rx = bits(4 * d[:, None, None] - p[None, :, :, 0])  # [dx, nby, nbx]
    ry = bits(4 * d[:, None, None] - p[None, :, :, 1])  # [dy, nby, nbx]
    r = ry[:, None] + rx[None, :]
    j = np.where(valid, sad + int(lam) * r, np.iinfo(np.int64).max)
    # candidates in raster order (dy outer, dx inner); argmin keeps the first minimum
    k = j.reshape(n * n, nby * nbx).argmin(axis=0)
    col = np.arange(nby * nbx)
    pick = lambda a: a.reshape(n * n, nby * nbx)[k, col]
    mv = np.stack([k % n - S, k // n - S], axis=1).astype(np.int16)
    return (mv, pick(j).astype(np.uint32), pick(sad).astype(np.uint32),
            pick(r).astype(np.uint8))


def refine(ref, cur, blk, mv, lam=0, pred=None, cost="ssd"):
    """qpel_ref.refine on Jq = cost + lam * (bits(qx - px) + bits(qy - py))."""
    F = qpel_ref._Frame(ref, blk)
    c = np.asarray(cur, np.uint8).astype(np.int64)
    mv = np.asarray(mv).reshape(-1, 2).astype(np.int64)
    p = _pred(pred, len(mv))

    def costs(q):
        d = c - F.predict(q)
        e = np.abs(d) if cost == "sad" else d * d
        dist = np.bincount(F.bidx.ravel(), weights=e.ravel(), minlength=F.n).astype(np.int64)
        return dist, dist + int(lam) * (bits(q[:, 0] - p[:, 0]) + bits(q[:, 1] - p[:, 1]))

    bq = 4 * mv
    bd, best = costs(bq)
    for step in (2, 1):
        centre = bq.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                cand = centre + step * np.array([dx, dy])
                d, v = costs(cand)
                better = v < best
                best[better] = v[better]
                bd[better] = d[better]
                bq[better] = cand[better]
    return bq.astype(np.int16), best.astype(np.uint32), bd.astype(np.uint32)


def summary(mv, J, D, R):
    """(sum D, sum R, blocks with a zero vector, sum J)."""
    zero = int(((mv[:, 0] == 0) & (mv[:, 1] == 0)).sum())
    return (int(D.astype(np.int64).sum()), int(R.astype(np.int64).sum()), zero,
            int(J.astype(np.int64).sum()))
