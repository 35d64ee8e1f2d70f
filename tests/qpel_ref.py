"""Numpy restatement of the quarter-pel definition (include/me.h, DESIGN.md
"Quarter-pel refinement"): the H.264 luma interpolation over an edge-replicated
reference, the two-stage (half, then quarter) refinement of an integer field
and the sub-pel compensation.  Exact integer arithmetic, written from the
definition and independent of the kernels: the GPU tests compare with it bit
for bit.

Coordinates: (X, Y) are half-pel units, (QX, QY) quarter-pel units, both
absolute (pixel x is X = 2x, QX = 4x)."""
import numpy as np

TAPS = np.array([1, -5, 20, 20, -5, 1], np.int64)


def _clip255(a):
    return np.clip(a, 0, 255)


def _fir(a, axis):
    """The 6-tap filter along `axis`, valid part only (length n - 5): output i
    is the half sample between inputs i + 2 and i + 3."""
    n = a.shape[axis] - 5
    out = np.zeros_like(np.take(a, range(n), axis=axis))
    for k, t in enumerate(TAPS):
        out = out + t * np.take(a, range(k, k + n), axis=axis)
    return out


def half_plane(ref, X0, X1, Y0, Y1):
    """P2(X, Y) for X in [X0, X1), Y in [Y0, Y1) as uint8 [Y1 - Y0, X1 - X0]."""
    ref = np.asarray(ref)
    H, W = ref.shape
    xa, xb = X0 // 2 - 2, (X1 - 1) // 2 + 4   # integer columns the taps may touch
    ya, yb = Y0 // 2 - 2, (Y1 - 1) // 2 + 4
    xs = np.clip(np.arange(xa, xb), 0, W - 1)
    ys = np.clip(np.arange(ya, yb), 0, H - 1)
    R = ref[np.ix_(ys, xs)].astype(np.int64)  # R[y - ya, x - xa], edge replicated
    b1 = _fir(R, 1)                           # b1[y - ya, x - (xa + 2)], unrounded
    h1 = _fir(R, 0)                           # h1[y - (ya + 2), x - xa]
    j1 = _fir(b1, 0)                          # j1[y - (ya + 2), x - (xa + 2)]
    Xs, Ys = np.arange(X0, X1), np.arange(Y0, Y1)
    xe, ye = Xs % 2 == 0, Ys % 2 == 0
    out = np.zeros((len(Ys), len(Xs)), np.int64)
    # integer columns / rows of the even coordinates, half columns / rows of the odd
    ci, ri = Xs[xe] // 2 - xa, Ys[ye] // 2 - ya
    ch, rh = (Xs[~xe] - 1) // 2 - (xa + 2), (Ys[~ye] - 1) // 2 - (ya + 2)
    out[np.ix_(ye, xe)] = R[np.ix_(ri, ci)]
    out[np.ix_(ye, ~xe)] = _clip255((b1[np.ix_(ri, ch)] + 16) >> 5)
    out[np.ix_(~ye, xe)] = _clip255((h1[np.ix_(rh, ci)] + 16) >> 5)
    out[np.ix_(~ye, ~xe)] = _clip255((j1[np.ix_(rh, ch)] + 512) >> 10)
    return out.astype(np.uint8)


class _Block:
    """The half-pel plane around one block at integer position (bx, by):
    enough for every quarter position within +-3 quarter units of it."""
    M = 4  # margin in half units (needs 2, floor(-3 / 2) = -2)

    def __init__(self, ref, bx, by, w, h):
        self.bx, self.by, self.w, self.h = bx, by, w, h
        self.X0, self.Y0 = 2 * bx - self.M, 2 * by - self.M
        self.P = half_plane(ref, self.X0, 2 * (bx + w - 1) + self.M + 1,
                            self.Y0, 2 * (by + h - 1) + self.M + 1).astype(np.int64)

    def _at(self, X, Y):
        """P2 at (X + 2 i, Y + 2 j) for the block's pixels (i, j)."""
        x, y = X - self.X0, Y - self.Y0
        return self.P[y:y + 2 * self.h:2, x:x + 2 * self.w:2]

    def predict(self, QX, QY):
        """The prediction block whose top-left sample is at quarter position (QX, QY)."""
        Xa, Ya = QX // 2, QY // 2
        xo, yo = QX % 2, QY % 2
        if not xo and not yo:
            return self._at(Xa, Ya)
        if xo and not yo:
            return (self._at(Xa, Ya) + self._at(Xa + 1, Ya) + 1) >> 1
        if yo and not xo:
            return (self._at(Xa, Ya) + self._at(Xa, Ya + 1) + 1) >> 1
        # both odd: the two corners with an odd coordinate sum (the horizontal
        # and the vertical half sample)
        if (Xa + Ya) % 2:
            return (self._at(Xa, Ya) + self._at(Xa + 1, Ya + 1) + 1) >> 1
        return (self._at(Xa + 1, Ya) + self._at(Xa, Ya + 1) + 1) >> 1


def _blocks(w, h, blk):
    for y0 in range(0, h, blk):
        for x0 in range(0, w, blk):
            yield x0, y0, min(blk, w - x0), min(blk, h - y0)


def _cost(cur_blk, pred, cost):
    d = cur_blk - pred
    return int(np.abs(d).sum()) if cost == "sad" else int((d * d).sum())


def refine_blockwise(ref, cur, blk, mv, cost="ssd"):
    """The refinement, block by block and candidate by candidate as the
    definition words it (slow; refine() is the same over whole frames)."""
    ref, cur = np.asarray(ref, np.uint8), np.asarray(cur, np.uint8)
    h, w = ref.shape
    mv = np.asarray(mv).reshape(-1, 2).astype(np.int64)
    q = np.zeros((len(mv), 2), np.int16)
    cst = np.zeros(len(mv), np.uint32)
    for n, (x0, y0, bw, bh) in enumerate(_blocks(w, h, blk)):
        mx, my = int(mv[n, 0]), int(mv[n, 1])
        B = _Block(ref, x0 + mx, y0 + my, bw, bh)
        c = cur[y0:y0 + bh, x0:x0 + bw].astype(np.int64)
        bq = (4 * mx, 4 * my)
        best = _cost(c, B.predict(4 * x0 + bq[0], 4 * y0 + bq[1]), cost)
        for step in (2, 1):
            centre = bq
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    cand = (centre[0] + step * dx, centre[1] + step * dy)
                    v = _cost(c, B.predict(4 * x0 + cand[0], 4 * y0 + cand[1]), cost)
                    if v < best:
                        best, bq = v, cand
        q[n] = bq
        cst[n] = best
    return q, cst


def compensate_blockwise(ref, blk, q):
    ref = np.asarray(ref, np.uint8)
    h, w = ref.shape
    q = np.asarray(q).reshape(-1, 2).astype(np.int64)
    mc = np.zeros((h, w), np.uint8)
    for n, (x0, y0, bw, bh) in enumerate(_blocks(w, h, blk)):
        qx, qy = int(q[n, 0]), int(q[n, 1])
        B = _Block(ref, x0 + qx // 4, y0 + qy // 4, bw, bh)
        mc[y0:y0 + bh, x0:x0 + bw] = B.predict(4 * x0 + qx, 4 * y0 + qy)
    return mc


class _Frame:
    """Whole-frame form: the half-pel plane of the frame and a margin, looked
    up per pixel.  Beyond 3 pixels outside the frame every tap reads the edge
    pixel, so P2 no longer changes along that axis and clamping the half
    coordinate to the margin is exact for any vector."""
    M = 4  # margin in pixels

    def __init__(self, ref, blk):
        ref = np.asarray(ref, np.uint8)
        self.h, self.w = h, w = ref.shape
        self.P = half_plane(ref, -2 * self.M, 2 * (w + self.M), -2 * self.M,
                            2 * (h + self.M)).astype(np.int64)
        yy, xx = np.mgrid[0:h, 0:w]
        self.xx, self.yy = xx, yy
        self.bidx = (yy // blk) * ((w + blk - 1) // blk) + xx // blk
        self.n = int(self.bidx.max()) + 1

    def _at(self, X, Y):
        X = np.clip(X, -2 * self.M, 2 * (self.w + self.M) - 1) + 2 * self.M
        Y = np.clip(Y, -2 * self.M, 2 * (self.h + self.M) - 1) + 2 * self.M
        return self.P[Y, X]

    def predict(self, q):
        """The prediction frame for the per-block quarter-pel vectors q [n, 2]."""
        QX = 4 * self.xx + q[self.bidx, 0]
        QY = 4 * self.yy + q[self.bidx, 1]
        Xa, Ya, xo, yo = QX >> 1, QY >> 1, QX & 1, QY & 1
        both, odd = xo & yo, (Xa + Ya) & 1
        # the two samples to average (the same one twice on the half grid); with
        # both axes odd, the two corners whose coordinate sum is odd
        ax = Xa + (both & (1 - odd))
        bx = np.where(both == 1, Xa + odd, Xa + xo)
        by = np.where(both == 1, Ya + 1, Ya + yo)
        return (self._at(ax, Ya) + self._at(bx, by) + 1) >> 1


def refine(ref, cur, blk, mv, cost="ssd"):
    """Quarter-pel refinement of the integer field mv [n, 2].  Returns
    (q int16 [n, 2] in quarter units, cost uint32 [n])."""
    F = _Frame(ref, blk)
    c = np.asarray(cur, np.uint8).astype(np.int64)
    mv = np.asarray(mv).reshape(-1, 2).astype(np.int64)

    def costs(q):
        d = c - F.predict(q)
        e = np.abs(d) if cost == "sad" else d * d
        return np.bincount(F.bidx.ravel(), weights=e.ravel(), minlength=F.n).astype(np.int64)

    bq = 4 * mv
    best = costs(bq)
    for step in (2, 1):
        centre = bq.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                cand = centre + step * np.array([dx, dy])
                v = costs(cand)
                better = v < best
                best[better] = v[better]
                bq[better] = cand[better]
    return bq.astype(np.int16), best.astype(np.uint32)


def compensate(ref, blk, q):
    """mc[y][x] = the prediction sample of the pixel's block at that block's q."""
    q = np.asarray(q).reshape(-1, 2).astype(np.int64)
    return _Frame(ref, blk).predict(q).astype(np.uint8)


def planes(ref, cur, mc):
    """The 5-plane output [ref, cur, mc, |ref - cur|, |mc - cur|] (5H, W)."""
    d = lambda a, b: np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)
    return np.concatenate([ref, cur, mc, d(ref, cur), d(mc, cur)])
