"""Passive tracers ("Tracers") restated in numpy, operation by operation.

Every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its own like the
device code (no FMA, IEEE divide).  Imports nothing from the product and nothing from the other restatements.  It is
fed by the grid the walk read: the cell-sorted positions and velocities and the cell table's {start, end} ranges
(sph_download_grid + sph_download_state, or the oracle's sort and table).

Sums are formed with np.cumsum in float32 over a row that begins with +0, which adds strictly left to right from +0:
the accumulation order of the definition (dz, dy, dx from -1 to 1 in that nesting, each cell's rows in stream order).
A candidate that is not taken contributes a SELECTED +0 term, np.where(take, m * v, 0): that changes no bit, because a
sum that starts at +0 is never -0 under round-to-nearest.  Positions that do not move are copied as 32-bit words."""
import numpy as np

F = np.float32
MASS = F(0.02)


def cells_of(p, h, D):
    """per coordinate: (cell, outside).  c = (int)(p / h); outside when !(p >= 0) or !(p / h < (float)D)."""
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        q = p / F(h)
        assert q.dtype == F
        outside = ~(p >= F(0)) | ~(q < F(D))
        c = np.where(outside, F(0), q).astype(np.int32)
    return c, outside


def neighbourhood(cell_ranges, D, cx, cy, cz):
    """stream rows of the 27 cells around (cx, cy, cz), in the order of the walk"""
    runs = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sx, sy, sz = cx + dx, cy + dy, cz + dz
                if min(sx, sy, sz) < 0 or max(sx, sy, sz) >= D:
                    continue
                s, e = cell_ranges[(sz * D + sy) * D + sx]
                runs.append(np.arange(s, e, dtype=np.int64))
    return np.concatenate(runs) if runs else np.zeros(0, np.int64)


def sum_from_zero(terms):
    """left-to-right float32 sum of every row, starting from +0"""
    zero = np.zeros((terms.shape[0], 1), F)
    return np.cumsum(np.concatenate([zero, terms], axis=1), axis=1, dtype=F)[:, -1]


def advect(pos, vel, cell_ranges, h, dcoef, D, tracers, dt):
    """pos (n, 3), vel (n, 3): the SORTED stream; cell_ranges (D^3, 2) int32; tracers (m, 3) float32.
    Returns {"pos" (m, 3), "den" (m,), "vel" (m, 3), "num" (m, 3) (the three numerators): float32;
    "taken" (m,): candidates with d2 <= h*h}."""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    cell_ranges = np.asarray(cell_ranges, dtype=np.int32).reshape(-1, 2)
    tracers = np.ascontiguousarray(tracers, dtype=F).reshape(-1, 3)
    D, m = int(D), len(tracers)
    dt = F(dt)
    h2 = F(h) * F(h)
    den = np.zeros(m, F)
    u = np.zeros((m, 3), F)
    num = np.zeros((m, 3), F)
    taken = np.zeros(m, np.int64)
    c, outside = cells_of(tracers, h, D)
    inside = ~outside.any(axis=1)
    key = (c[:, 2].astype(np.int64) * D + c[:, 1]) * D + c[:, 0]
    for k in (np.unique(key[inside]) if len(pos) else ()):
        who = np.flatnonzero(inside & (key == k))
        j = neighbourhood(cell_ranges, D, int(k % D), int(k // D % D), int(k // (D * D)))
        if len(j) == 0:
            continue
        p = tracers[who]
        with np.errstate(all="ignore"):
            dx = p[:, None, 0] - pos[None, j, 0]
            dy = p[:, None, 1] - pos[None, j, 1]
            dz = p[:, None, 2] - pos[None, j, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            take = ~(d2 > h2)
            diff = h2 - d2
            mj = MASS * (((F(dcoef) * diff) * diff) * diff)
            assert mj.dtype == F
            d = sum_from_zero(np.where(take, mj, F(0)))
            n = [sum_from_zero(np.where(take, mj * vel[None, j, a], F(0))) for a in range(3)]
            den[who] = d
            for a in range(3):
                num[who, a] = n[a]
                u[who, a] = np.where(d > F(0), n[a] / d, F(0))
        taken[who] = take.sum(axis=1)
    out = tracers.copy()
    if dt != F(0):
        moved = den > F(0)
        with np.errstate(all="ignore"):
            step = tracers + u * dt                   # one multiply, then one add, per axis
        assert step.dtype == F
        # (word-wise: the positions that stay are copied, not recomputed)
        out.view(np.uint32)[moved] = step.view(np.uint32)[moved]
    return dict(pos=out, den=den, vel=u, num=num, taken=taken)
