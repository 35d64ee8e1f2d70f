"""Numpy restatement of the SATD cost (include/me.h "SATD cost", DESIGN.md
"SATD cost") and of the three procedures that take it: the quarter-pel
refinement, the rate-constrained refinement and the bi-prediction.  Exact
integer arithmetic on top of qpel_ref's prediction samples, written from the
definition and independent of the kernels: the GPU tests compare with it bit
for bit.

The definition, for a block clipped to bw x bh with prediction P and current
block C: the residual d = C - P inside the block and 0 outside; 4x4 tiles
anchored at the block's own top-left, ceil(bw / 4) x ceil(bh / 4) of them,
partial tiles zero padded; T = H D H^T per tile with H the order-4 +-1 Hadamard
matrix; satd = (sum over tiles of sum |T|) >> 1.

Two forms of everything, as in qpel_ref and bipred_ref: the *_blockwise
functions word the definition block by block, tile by tile and candidate by
candidate (qpel_ref._Block.predict); the others work on whole frames
(qpel_ref._Frame.predict) and are fast enough for the GPU tests."""
import numpy as np

import bipred_ref as BP
import qpel_ref as Q
import rd_ref as RD

H4 = np.array([[1, 1, 1, 1],
               [1, 1, -1, -1],
               [1, -1, -1, 1],
               [1, -1, 1, -1]], np.int64)


def tile_coefficients(d):
    """T = H D H^T of one 4x4 residual tile."""
    return H4 @ np.asarray(d, np.int64) @ H4.T


def satd(cur_blk, pred):
    """The satd of one block, tile by tile as the definition words it."""
    d = np.asarray(cur_blk, np.int64) - np.asarray(pred, np.int64)
    bh, bw = d.shape
    total = 0
    for ty in range(0, bh, 4):
        for tx in range(0, bw, 4):
            tile = np.zeros((4, 4), np.int64)  # zero padded
            part = d[ty:ty + 4, tx:tx + 4]
            tile[:part.shape[0], :part.shape[1]] = part
            total += int(np.abs(tile_coefficients(tile)).sum())
    return total >> 1


class _Tiles:
    """Whole-frame form: every block of the frame gets a cell of P x P samples,
    P = 4 ceil(blk / 4), in a zero plane, its residual at the cell's top-left,
    so the plane's own 4x4 grid is every block's tile grid with its padding."""

    def __init__(self, w, h, blk):
        self.nbx, self.nby = (w + blk - 1) // blk, (h + blk - 1) // blk
        self.P = P = 4 * ((blk + 3) // 4)
        yy, xx = np.mgrid[0:h, 0:w]
        self.py = (yy // blk) * P + yy % blk
        self.px = (xx // blk) * P + xx % blk

    def costs(self, d):
        """satd of every block for the frame residual d [h, w]: int64 [n]."""
        P, nbx, nby = self.P, self.nbx, self.nby
        plane = np.zeros((nby * P, nbx * P), np.int64)
        plane[self.py, self.px] = d
        t = plane.reshape(nby * P // 4, 4, nbx * P // 4, 4)
        t = np.einsum("ua,yaxb,vb->yuxv", H4, t, H4)
        per_tile = np.abs(t).sum(axis=(1, 3))  # [tile rows, tile columns]
        per_blk = per_tile.reshape(nby, P // 4, nbx, P // 4).sum(axis=(1, 3))
        return per_blk.reshape(-1) >> 1


def block_costs(cur, pred, blk):
    """satd of every block of the prediction frame pred against cur."""
    cur = np.asarray(cur, np.uint8)
    h, w = cur.shape
    return _Tiles(w, h, blk).costs(cur.astype(np.int64) - np.asarray(pred, np.int64))


# ---- quarter-pel refinement (qpel_ref.refine with cost = satd) ----

def refine_rd_blockwise(ref, cur, blk, mv, lam=0, pred=None):
    """The rate-constrained refinement on Jq = satd + lam * bits, block by
    block and candidate by candidate.  Returns (q int16 [n, 2], Jq uint32 [n],
    dist uint32 [n])."""
    ref, cur = np.asarray(ref, np.uint8), np.asarray(cur, np.uint8)
    h, w = ref.shape
    mv = np.asarray(mv).reshape(-1, 2).astype(np.int64)
    p = RD._pred(pred, len(mv))
    q = np.zeros((len(mv), 2), np.int16)
    J = np.zeros(len(mv), np.uint32)
    D = np.zeros(len(mv), np.uint32)
    for n, (x0, y0, bw, bh) in enumerate(Q._blocks(w, h, blk)):
        mx, my = int(mv[n, 0]), int(mv[n, 1])
        B = Q._Block(ref, x0 + mx, y0 + my, bw, bh)
        c = cur[y0:y0 + bh, x0:x0 + bw].astype(np.int64)

        def jq(cand):
            dist = satd(c, B.predict(4 * x0 + cand[0], 4 * y0 + cand[1]))
            rate = int(RD.bits(cand[0] - p[n, 0])) + int(RD.bits(cand[1] - p[n, 1]))
            return dist, dist + int(lam) * rate

        bq = (4 * mx, 4 * my)
        bd, best = jq(bq)
        for step in (2, 1):
            centre = bq
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    cand = (centre[0] + step * dx, centre[1] + step * dy)
                    d, v = jq(cand)
                    if v < best:
                        best, bd, bq = v, d, cand
        q[n], J[n], D[n] = bq, best, bd
    return q, J, D


def refine_blockwise(ref, cur, blk, mv):
    """The plain refinement on satd (the rate-constrained one without a rate
    term is the same procedure).  Returns (q int16 [n, 2], satd uint32 [n])."""
    q, _, d = refine_rd_blockwise(ref, cur, blk, mv, 0, None)
    return q, d


def refine_rd(ref, cur, blk, mv, lam=0, pred=None):
    """Whole-frame form of refine_rd_blockwise."""
    F = Q._Frame(ref, blk)
    T = _Tiles(F.w, F.h, blk)
    c = np.asarray(cur, np.uint8).astype(np.int64)
    mv = np.asarray(mv).reshape(-1, 2).astype(np.int64)
    p = RD._pred(pred, len(mv))

    def costs(q):
        dist = T.costs(c - F.predict(q))
        return dist, dist + int(lam) * (RD.bits(q[:, 0] - p[:, 0]) + RD.bits(q[:, 1] - p[:, 1]))

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


def refine(ref, cur, blk, mv):
    """Whole-frame form of refine_blockwise: (q int16 [n, 2], satd uint32 [n])."""
    q, _, d = refine_rd(ref, cur, blk, mv, 0, None)
    return q, d


# ---- bi-prediction (bipred_ref.bipred with cost = satd) ----

def bipred(ref0, ref1, cur, blk, q0, q1, refine=1):
    """Returns (out0 int16 [n, 2], out1 int16 [n, 2], mode uint8 [n],
    block_cost uint32 [n], cost3 uint32 [n, 3] = (c0, c1, cb)), all in satd."""
    F0, F1 = Q._Frame(ref0, blk), Q._Frame(ref1, blk)
    T = _Tiles(F0.w, F0.h, blk)
    c = np.asarray(cur, np.uint8).astype(np.int64)
    q0 = np.asarray(q0).reshape(-1, 2).astype(np.int64)
    q1 = np.asarray(q1).reshape(-1, 2).astype(np.int64)
    costs = lambda pred: T.costs(c - pred)

    P0, P1 = F0.predict(q0), F1.predict(q1)
    c0, c1, cb = costs(P0), costs(P1), costs(BP._avg(P0, P1))
    b0, b1 = q0.copy(), q1.copy()
    if refine:
        # pass 1 holds b0 and moves b1, pass 2 holds pass 1's b1 and moves b0
        for moving in (1, 0):
            held = F0.predict(b0) if moving else F1.predict(b1)
            centre = (b1 if moving else b0).copy()
            for d in BP.NEIGHBOURS:
                cand = centre + np.array(d)
                v = costs(BP._avg(held, (F1 if moving else F0).predict(cand)))
                better = v < cb
                cb[better] = v[better]
                (b1 if moving else b0)[better] = cand[better]
    mode, best = BP._decide(c0, c1, cb)
    return BP._pack(q0, q1, b0, b1, mode, best, c0, c1, cb)


def bipred_blockwise(ref0, ref1, cur, blk, q0, q1, refine=1):
    """The same, one block and one candidate at a time (slow)."""
    ref0, ref1 = np.asarray(ref0, np.uint8), np.asarray(ref1, np.uint8)
    cur = np.asarray(cur, np.uint8)
    h, w = cur.shape
    q0 = np.asarray(q0).reshape(-1, 2).astype(np.int64)
    q1 = np.asarray(q1).reshape(-1, 2).astype(np.int64)
    b0, b1 = q0.copy(), q1.copy()
    c3 = np.zeros((len(q0), 3), np.int64)
    for k, (x0, y0, bw, bh) in enumerate(Q._blocks(w, h, blk)):
        B0 = Q._Block(ref0, x0 + int(BP._nearest(q0[k, 0])), y0 + int(BP._nearest(q0[k, 1])), bw, bh)
        B1 = Q._Block(ref1, x0 + int(BP._nearest(q1[k, 0])), y0 + int(BP._nearest(q1[k, 1])), bw, bh)
        c = cur[y0:y0 + bh, x0:x0 + bw].astype(np.int64)
        p0 = lambda v: B0.predict(4 * x0 + int(v[0]), 4 * y0 + int(v[1]))
        p1 = lambda v: B1.predict(4 * x0 + int(v[0]), 4 * y0 + int(v[1]))
        v0, v1 = tuple(q0[k]), tuple(q1[k])
        c3[k, 0] = satd(c, p0(v0))
        c3[k, 1] = satd(c, p1(v1))
        cb = satd(c, BP._avg(p0(v0), p1(v1)))
        if refine:
            centre = v1
            for dx, dy in BP.NEIGHBOURS:
                cand = (centre[0] + dx, centre[1] + dy)
                v = satd(c, BP._avg(p0(v0), p1(cand)))
                if v < cb:
                    cb, v1 = v, cand
            centre = v0
            for dx, dy in BP.NEIGHBOURS:
                cand = (centre[0] + dx, centre[1] + dy)
                v = satd(c, BP._avg(p0(cand), p1(v1)))
                if v < cb:
                    cb, v0 = v, cand
        c3[k, 2] = cb
        b0[k], b1[k] = v0, v1
    mode, best = BP._decide(c3[:, 0].copy(), c3[:, 1].copy(), c3[:, 2].copy())
    return BP._pack(q0, q1, b0, b1, mode, best, c3[:, 0], c3[:, 1], c3[:, 2])
