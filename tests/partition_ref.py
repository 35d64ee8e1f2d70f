"""numpy restatement of the partition search (include/me.h "partition search").

Two forms of the same definition:
  search_loops  the definition's own loops: per macroblock, per displacement in
                raster order, the SAD of each clipped partition; strict < keeps
                the first minimum.
  search_frame  per displacement over the whole frame: one |cur - ref(+d)|
                plane, quadrant sums on the h grid, and a masked strict-<
                update of every cell whose macroblock has d among its
                candidates.  Fast enough for +-32 on a 256x144 frame.
decide() is the mode decision, leaf_field() the leaf field, both from the
records alone.  Results are Fields: mv / cost lists in the order 2Nx2N, 2NxN,
Nx2N, NxN, each in the raster order of its own grid.
"""
import numpy as np

MODES = ("2Nx2N", "2NxN", "Nx2N", "NxN")
VECTORS = (1, 2, 2, 4)  # nominal vector count (and lambda multiplier) of a mode


def grids(w, h, B):
    """((nx, ny) of the 2Nx2N, 2NxN, Nx2N and NxN grids)."""
    hb = B // 2
    nbx, nby = -(-w // B), -(-h // B)
    nhx, nhy = -(-w // hb), -(-h // hb)
    return ((nbx, nby), (nbx, nhy), (nhx, nby), (nhx, nhy))


def counts(w, h, B):
    return tuple(nx * ny for nx, ny in grids(w, h, B))


class Fields:
    def __init__(self, w, h, B):
        self.w, self.h, self.B = w, h, B
        n = counts(w, h, B)
        self.mv = [np.zeros((k, 2), np.int16) for k in n]
        self.cost = [np.zeros(k, np.uint32) for k in n]
        self.mode = np.zeros(n[0], np.uint8)
        self.mode_cost = np.zeros(n[0], np.uint32)


def _window(x0, bw, W, S):
    """Displacements of a macroblock along one axis: [lo, hi]."""
    return max(0, x0 - S) - x0, min(W, x0 + bw + S) - bw - x0


def _partitions(B, bw, bh):
    """(grid index, cell offset (i, j), x, y, w, h) of a clipped macroblock's
    non-empty partitions, relative to its top-left."""
    hb = B // 2
    out = [(0, 0, 0, 0, 0, bw, bh)]
    for j in range(2):
        if j * hb < bh:
            out.append((1, 0, j, 0, j * hb, bw, min(hb, bh - j * hb)))
    for i in range(2):
        if i * hb < bw:
            out.append((2, i, 0, i * hb, 0, min(hb, bw - i * hb), bh))
    for j in range(2):
        for i in range(2):
            if i * hb < bw and j * hb < bh:
                out.append((3, i, j, i * hb, j * hb, min(hb, bw - i * hb), min(hb, bh - j * hb)))
    return out


def search_loops(ref, cur, B, S, lam=0):
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    F = Fields(W, H, B)
    g = grids(W, H, B)
    for by in range(g[0][1]):
        for bx in range(g[0][0]):
            x0, y0 = bx * B, by * B
            bw, bh = min(B, W - x0), min(B, H - y0)
            dx0, dx1 = _window(x0, bw, W, S)
            dy0, dy1 = _window(y0, bh, H, S)
            parts = _partitions(B, bw, bh)
            best = [None] * len(parts)
            blk = cur[y0:y0 + bh, x0:x0 + bw]
            for dy in range(dy0, dy1 + 1):
                for dx in range(dx0, dx1 + 1):
                    d = np.abs(blk - ref[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw])
                    for n, (_, _, _, px, py, pw, ph) in enumerate(parts):
                        c = int(d[py:py + ph, px:px + pw].sum())
                        if best[n] is None or c < best[n][0]:
                            best[n] = (c, dx, dy)
            for (gi, i, j, *_), (c, dx, dy) in zip(parts, best):
                sx, sy = (1, 1, 2, 2)[gi], (1, 2, 1, 2)[gi]
                cell = (sy * by + j) * g[gi][0] + sx * bx + i
                F.mv[gi][cell] = (dx, dy)
                F.cost[gi][cell] = c
    return decide(F, lam)


def search_frame(ref, cur, B, S, lam=0):
    ref = np.asarray(ref, np.int32)
    cur = np.asarray(cur, np.int32)
    H, W = cur.shape
    hb = B // 2
    g = grids(W, H, B)
    nbx, nby = g[0]
    # macroblock displacement windows
    wx = np.array([_window(bx * B, min(B, W - bx * B), W, S) for bx in range(nbx)])
    wy = np.array([_window(by * B, min(B, H - by * B), H, S) for by in range(nby)])
    PH, PW = 2 * nby * hb, 2 * nbx * hb  # the frame padded to whole macroblocks
    pad = np.zeros((PH + 2 * S, PW + 2 * S), np.int32)
    pad[S:S + H, S:S + W] = ref
    curp = np.zeros((PH, PW), np.int32)
    curp[:H, :W] = cur
    inside = np.zeros((PH, PW), bool)
    inside[:H, :W] = True
    rep = ((1, 1), (1, 2), (2, 1), (2, 2))  # cells per macroblock (x, y) of each grid
    big = np.iinfo(np.int64).max
    best = [np.full((ry * nby, rx * nbx), big, np.int64) for rx, ry in rep]
    bdx = [np.zeros(b.shape, np.int16) for b in best]
    bdy = [np.zeros(b.shape, np.int16) for b in best]
    for dy in range(-S, S + 1):
        vy = (wy[:, 0] <= dy) & (dy <= wy[:, 1])
        if not vy.any():
            continue
        for dx in range(-S, S + 1):
            valid = vy[:, None] & ((wx[:, 0] <= dx) & (dx <= wx[:, 1]))[None, :]
            if not valid.any():
                continue
            d = np.abs(curp - pad[S + dy:S + dy + PH, S + dx:S + dx + PW])
            d[~inside] = 0  # pixels beyond the frame belong to no partition
            q = d.reshape(2 * nby, hb, 2 * nbx, hb).sum(axis=(1, 3)).astype(np.int64)
            c = (q.reshape(nby, 2, nbx, 2).sum(axis=(1, 3)),       # 2Nx2N
                 q.reshape(2 * nby, nbx, 2).sum(axis=2),            # 2NxN
                 q.reshape(nby, 2, 2 * nbx).sum(axis=1),            # Nx2N
                 q)                                                 # NxN
            for k, (rx, ry) in enumerate(rep):
                v = np.repeat(np.repeat(valid, ry, axis=0), rx, axis=1)
                upd = v & (c[k] < best[k])
                best[k][upd] = c[k][upd]
                bdx[k][upd] = dx
                bdy[k][upd] = dy
    F = Fields(W, H, B)
    for k, (nx, ny) in enumerate(g):
        F.mv[k][:, 0] = bdx[k][:ny, :nx].reshape(-1)
        F.mv[k][:, 1] = bdy[k][:ny, :nx].reshape(-1)
        F.cost[k][:] = best[k][:ny, :nx].reshape(-1)
    return decide(F, lam)


def decide(F, lam):
    """F's records with the mode / mode_cost of every macroblock at lambda =
    lam: a new Fields sharing F's vector and cost arrays; F is not changed."""
    g = grids(F.w, F.h, F.B)
    nbx, nby = g[0]
    pads = []
    for k, (nx, ny) in enumerate(g):
        rx, ry = (1, 1, 2, 2)[k], (1, 2, 1, 2)[k]
        p = np.zeros((ry * nby, rx * nbx), np.int64)  # missing partitions cost 0
        p[:ny, :nx] = F.cost[k].reshape(ny, nx)
        pads.append(p.reshape(nby, ry, nbx, rx).sum(axis=(1, 3)))
    J = [pads[k] + VECTORS[k] * int(lam) for k in range(4)]
    best, mode = J[0].copy(), np.zeros((nby, nbx), np.uint8)
    for k in (1, 2, 3):
        upd = J[k] < best
        best[upd] = J[k][upd]
        mode[upd] = k
    out = Fields.__new__(Fields)
    out.w, out.h, out.B, out.mv, out.cost = F.w, F.h, F.B, F.mv, F.cost
    out.mode = mode.reshape(-1)
    out.mode_cost = best.reshape(-1).astype(np.uint32)
    return out


def leaf_field(F):
    """int16 [nhx * nhy, 2]: every N x N cell takes the vector of the partition
    of its macroblock's mode that contains it."""
    g = grids(F.w, F.h, F.B)
    (nbx, nby), (nhx, nhy) = g[0], g[3]
    leaf = np.zeros((nhx * nhy, 2), np.int16)
    for hy in range(nhy):
        for hx in range(nhx):
            bx, by = hx // 2, hy // 2
            m = F.mode[by * nbx + bx]
            src = (F.mv[0][by * nbx + bx], F.mv[1][hy * nbx + bx], F.mv[2][by * nhx + hx],
                   F.mv[3][hy * nhx + hx])[m]
            leaf[hy * nhx + hx] = src
    return leaf


def summary(F, lam):
    """(mode histogram [4], sum J, sum distortion): the distortion of a
    macroblock is J - lam * (nominal vector count of its mode)."""
    hist = np.bincount(F.mode, minlength=4)
    sj = int(F.mode_cost.astype(np.int64).sum())
    return hist.tolist(), sj, sj - int(lam) * int(np.dot(hist, VECTORS))
