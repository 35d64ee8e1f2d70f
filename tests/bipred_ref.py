"""Numpy restatement of the bi-prediction definition (include/me.h, DESIGN.md
"Bi-prediction"): per block the costs of predicting from ref0 at q0, from ref1
at q1 and from the rounded average of both, the joint quarter-step refinement
of the averaged pair, the mode decision and the compensation that follows from
it.  Exact integer arithmetic on top of qpel_ref's prediction samples, written
from the definition and independent of the kernels: the GPU tests compare with
it bit for bit.

Two forms, as in qpel_ref: bipred / compensate work on whole frames
(qpel_ref._Frame.predict), bipred_blockwise / compensate_blockwise word the
definition block by block and candidate by candidate (qpel_ref._Block.predict)."""
import numpy as np

import qpel_ref as Q

L0, L1, BI = 0, 1, 2
MAX_Q = 32766  # ME_BIPRED_MAX_Q: q +- 1 fits int16
# the eight neighbours in raster order, dy outer
NEIGHBOURS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]


def _avg(a, b):
    return (a + b + 1) >> 1


def _decide(c0, c1, cb):
    """L0, L1, BI in that order; a later mode wins only if strictly smaller."""
    mode = np.zeros(len(c0), np.uint8)
    best = c0.copy()
    for m, c in ((L1, c1), (BI, cb)):
        better = c < best
        best[better] = c[better]
        mode[better] = m
    return mode, best


def _pack(q0, q1, b0, b1, mode, best, c0, c1, cb):
    bi = (mode == BI)[:, None]
    out0 = np.where(bi, b0, q0).astype(np.int16)
    out1 = np.where(bi, b1, q1).astype(np.int16)
    return (out0, out1, mode, best.astype(np.uint32),
            np.stack([c0, c1, cb], axis=1).astype(np.uint32))


def bipred(ref0, ref1, cur, blk, q0, q1, cost="ssd", refine=1):
    """Returns (out0 int16 [n, 2], out1 int16 [n, 2], mode uint8 [n],
    block_cost uint32 [n], cost3 uint32 [n, 3] = (c0, c1, cb))."""
    F0, F1 = Q._Frame(ref0, blk), Q._Frame(ref1, blk)
    c = np.asarray(cur, np.uint8).astype(np.int64)
    q0 = np.asarray(q0).reshape(-1, 2).astype(np.int64)
    q1 = np.asarray(q1).reshape(-1, 2).astype(np.int64)

    def costs(pred):
        d = c - pred
        e = np.abs(d) if cost == "sad" else d * d
        return np.bincount(F0.bidx.ravel(), weights=e.ravel(), minlength=F0.n).astype(np.int64)

    P0, P1 = F0.predict(q0), F1.predict(q1)
    c0, c1, cb = costs(P0), costs(P1), costs(_avg(P0, P1))
    b0, b1 = q0.copy(), q1.copy()
    if refine:
        # pass 1 holds b0 and moves b1, pass 2 holds pass 1's b1 and moves b0
        for moving in (1, 0):
            held = F0.predict(b0) if moving else F1.predict(b1)
            centre = (b1 if moving else b0).copy()
            for d in NEIGHBOURS:
                cand = centre + np.array(d)
                v = costs(_avg(held, (F1 if moving else F0).predict(cand)))
                better = v < cb
                cb[better] = v[better]
                (b1 if moving else b0)[better] = cand[better]
    mode, best = _decide(c0, c1, cb)
    return _pack(q0, q1, b0, b1, mode, best, c0, c1, cb)


def _nearest(q):
    return (q + 2) >> 2


def bipred_blockwise(ref0, ref1, cur, blk, q0, q1, cost="ssd", refine=1):
    """The same, one block and one candidate at a time (slow)."""
    ref0, ref1 = np.asarray(ref0, np.uint8), np.asarray(ref1, np.uint8)
    cur = np.asarray(cur, np.uint8)
    h, w = cur.shape
    q0 = np.asarray(q0).reshape(-1, 2).astype(np.int64)
    q1 = np.asarray(q1).reshape(-1, 2).astype(np.int64)
    n = len(q0)
    b0, b1 = q0.copy(), q1.copy()
    c3 = np.zeros((n, 3), np.int64)
    for k, (x0, y0, bw, bh) in enumerate(Q._blocks(w, h, blk)):
        # each window sits at the vector's nearest integer position: the
        # vector and its eight neighbours are within 3 quarter units of it
        B0 = Q._Block(ref0, x0 + int(_nearest(q0[k, 0])), y0 + int(_nearest(q0[k, 1])), bw, bh)
        B1 = Q._Block(ref1, x0 + int(_nearest(q1[k, 0])), y0 + int(_nearest(q1[k, 1])), bw, bh)
        c = cur[y0:y0 + bh, x0:x0 + bw].astype(np.int64)
        p0 = lambda v: B0.predict(4 * x0 + int(v[0]), 4 * y0 + int(v[1]))
        p1 = lambda v: B1.predict(4 * x0 + int(v[0]), 4 * y0 + int(v[1]))
        v0, v1 = tuple(q0[k]), tuple(q1[k])
        c3[k, 0] = Q._cost(c, p0(v0), cost)
        c3[k, 1] = Q._cost(c, p1(v1), cost)
        cb = Q._cost(c, _avg(p0(v0), p1(v1)), cost)
        if refine:
            centre = v1
            for dx, dy in NEIGHBOURS:
                cand = (centre[0] + dx, centre[1] + dy)
                v = Q._cost(c, _avg(p0(v0), p1(cand)), cost)
                if v < cb:
                    cb, v1 = v, cand
            centre = v0
            for dx, dy in NEIGHBOURS:
                cand = (centre[0] + dx, centre[1] + dy)
                v = Q._cost(c, _avg(p0(cand), p1(v1)), cost)
                if v < cb:
                    cb, v0 = v, cand
        c3[k, 2] = cb
        b0[k], b1[k] = v0, v1
    mode, best = _decide(c3[:, 0].copy(), c3[:, 1].copy(), c3[:, 2].copy())
    return _pack(q0, q1, b0, b1, mode, best, c3[:, 0], c3[:, 1], c3[:, 2])


def compensate(ref0, ref1, blk, v0, v1, mode):
    """mc[y][x] = P0(v0), P1(v1) or PB(v0, v1) of the pixel's block, by its mode."""
    F0, F1 = Q._Frame(ref0, blk), Q._Frame(ref1, blk)
    v0 = np.asarray(v0).reshape(-1, 2).astype(np.int64)
    v1 = np.asarray(v1).reshape(-1, 2).astype(np.int64)
    m = np.asarray(mode).ravel()[F0.bidx]
    P0, P1 = F0.predict(v0), F1.predict(v1)
    return np.where(m == L0, P0, np.where(m == L1, P1, _avg(P0, P1))).astype(np.uint8)


def compensate_blockwise(ref0, ref1, blk, v0, v1, mode):
    ref0, ref1 = np.asarray(ref0, np.uint8), np.asarray(ref1, np.uint8)
    h, w = ref0.shape
    v0 = np.asarray(v0).reshape(-1, 2).astype(np.int64)
    v1 = np.asarray(v1).reshape(-1, 2).astype(np.int64)
    mode = np.asarray(mode).ravel()
    mc = np.zeros((h, w), np.uint8)
    for k, (x0, y0, bw, bh) in enumerate(Q._blocks(w, h, blk)):
        def pred(ref, v):
            qx, qy = int(v[0]), int(v[1])
            return Q._Block(ref, x0 + qx // 4, y0 + qy // 4, bw, bh).predict(4 * x0 + qx, 4 * y0 + qy)
        if mode[k] == L0:
            p = pred(ref0, v0[k])
        elif mode[k] == L1:
            p = pred(ref1, v1[k])
        else:
            p = _avg(pred(ref0, v0[k]), pred(ref1, v1[k]))
        mc[y0:y0 + bh, x0:x0 + bw] = p
    return mc


def block_costs(cur, mc, blk, cost):
    """The cost of every block of the compensated frame mc."""
    cur = np.asarray(cur, np.uint8)
    h, w = cur.shape
    d = mc.astype(np.int64) - cur
    e = np.abs(d) if cost == "sad" else d * d
    return np.array([int(e[y0:y0 + bh, x0:x0 + bw].sum())
                     for x0, y0, bw, bh in Q._blocks(w, h, blk)], np.int64)


def foreman(cost):
    """Foreman 1 -> 2 <- 4, 16x16, +-7, from the integer oracle's searches and
    qpel_ref's refinements: (ref0, ref1, cur, q0, c0, q1, c1)."""
    import oracle_lib as O
    f1, f2, f4 = (O.load_frame(k) for k in ("ForemanYF1", "ForemanYF2", "ForemanYF4"))
    out = [f1, f4, f2]
    for ref in (f1, f4):
        mv = O.full_search(ref, f2, 16, 7, cost, threads=16)[0]
        out += list(Q.refine(ref, f2, 16, mv, cost))
    return tuple(out)


def planted(w, h, blk, seed):
    """Frames with a known answer of every mode: ref0 and ref1 are random
    bytes, per-block vectors qa, qb are random in [-9, 9], block n of cur is
    P0(qa), P1(qb) or PB(qa, qb) by n % 3 plus noise in [-2, 2]; the inputs are
    qa, qb each jittered by [-1, 1].  Returns (ref0, ref1, cur, q0, q1)."""
    rng = np.random.default_rng(seed)
    ref0 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    ref1 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    n = len(list(Q._blocks(w, h, blk)))
    qa = rng.integers(-9, 10, (n, 2))
    qb = rng.integers(-9, 10, (n, 2))
    clean = compensate(ref0, ref1, blk, qa, qb, np.arange(n) % 3).astype(np.int64)
    cur = np.clip(clean + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    q0 = (qa + rng.integers(-1, 2, (n, 2))).astype(np.int16)
    q1 = (qb + rng.integers(-1, 2, (n, 2))).astype(np.int16)
    return ref0, ref1, cur, q0, q1
