"""The field sample ("The field sample") restated in numpy, operation by operation.

Every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its own like
the device code (no FMA, IEEE divide, correctly rounded square root).  Shares no code with the HIP side.  It is
fed by the grid the sampler walked: the cell-sorted positions, velocities and densities and the cell table's
{start, end} ranges (sph_download_grid + sph_download_state, or the oracle's sort and table).

Sums are formed with np.cumsum in float32, which adds strictly left to right: the accumulation order of the
definition (dz, dy, dx from -1 to 1 in that nesting, each cell's rows in stream order).  A candidate beyond h
contributes a +0 term, which changes no bit of a sum that starts at +0 and only ever adds values >= +0."""
import numpy as np

F = np.float32
MASS = F(0.02)
GAS_CONSTANT = F(1)
REST_DENSITY = F(1000)
EPS_F = F(1e-4)
FIELDS = ("speed", "density", "pressure")


def lattice_axis(origin, spacing, count):
    """p = origin + (float)i * spacing: one multiply, one add"""
    return F(origin) + np.arange(count, dtype=np.int32).astype(F) * F(spacing)


def lattice_points(origin, spacing, shape):
    """(nz, ny, nx, 3) float32: the points in output order, index (iz * ny + iy) * nx + ix"""
    nz, ny, nx = shape
    x, y, z = (lattice_axis(origin[a], spacing[a], c) for a, c in ((0, nx), (1, ny), (2, nz)))
    pts = np.empty((nz, ny, nx, 3), F)
    pts[..., 0] = x[None, None, :]
    pts[..., 1] = y[None, :, None]
    pts[..., 2] = z[:, None, None]
    return pts


def cells_of(p, h, D):
    """per coordinate: (cell, outside).  c = (int)(p / h); outside when !(p >= 0) or c >= D."""
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        q = p / F(h)
        assert q.dtype == F
        outside = ~(p >= F(0)) | ~(q < F(D))       # (q >= D  <=>  (int)q >= D: D is an integer)
        c = np.where(outside, F(0), q).astype(np.int32)
    return c, outside


def scalar(vel, rho, field):
    """section 10a's a_j, from the values sph_download_state returns for the row"""
    if field == "speed":
        vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
        return np.sqrt((vx * vx + vy * vy) + vz * vz)
    if field == "pressure":
        return np.maximum(F(0), GAS_CONSTANT * (rho - REST_DENSITY))
    raise ValueError(field)


def weights(p, cand, h, dcoef):
    """(points, candidates) float32: m, or +0 where d2 > h*h"""
    h2 = F(h) * F(h)
    dx = p[:, None, 0] - cand[None, :, 0]
    dy = p[:, None, 1] - cand[None, :, 1]
    dz = p[:, None, 2] - cand[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    diff = h2 - d2
    m = MASS * (((F(dcoef) * diff) * diff) * diff)
    assert m.dtype == F
    return np.where(d2 > h2, F(0), m)


def ordered_sum(terms):
    """left-to-right float32 sum of every row, starting from 0"""
    if terms.shape[1] == 0:
        return np.zeros(terms.shape[0], F)
    return np.cumsum(terms, axis=1, dtype=F)[:, -1]


def sample(pos, vel, rho, cell_ranges, h, dcoef, D, field, origin, spacing, shape):
    """pos (n, 3), vel (n, 3), rho (n): the SORTED stream; cell_ranges (D^3, 2) int32.  Returns (nz, ny, nx) float32."""
    assert field in FIELDS
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    rho = np.ascontiguousarray(rho, dtype=F).reshape(-1)
    cell_ranges = np.asarray(cell_ranges, dtype=np.int32).reshape(-1, 2)
    D = int(D)
    pts = lattice_points(origin, spacing, shape).reshape(-1, 3)
    c, outside = cells_of(pts, h, D)
    inside = ~outside.any(axis=1)
    out = np.zeros(len(pts), F)                      # outside points: +0
    a = scalar(vel, rho, field) if field != "density" and len(pos) else None
    key = (c[:, 2].astype(np.int64) * D + c[:, 1]) * D + c[:, 0]
    for k in np.unique(key[inside]):
        who = np.flatnonzero(inside & (key == k))
        cx, cy, cz = int(k % D), int(k // D % D), int(k // (D * D))
        runs = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    sx, sy, sz = cx + dx, cy + dy, cz + dz
                    if min(sx, sy, sz) < 0 or max(sx, sy, sz) >= D:
                        continue
                    s, e = cell_ranges[(sz * D + sy) * D + sx]
                    runs.append(np.arange(s, e, dtype=np.int64))
        j = np.concatenate(runs) if runs else np.zeros(0, np.int64)
        if len(j) == 0:                              # empty sums: +0 for every field
            continue
        m = weights(pts[who], pos[j], h, dcoef)
        den = ordered_sum(m)
        if field == "density":
            out[who] = den
        else:
            num = ordered_sum(m * a[j][None, :])
            with np.errstate(all="ignore"):
                out[who] = np.where(den > F(0), num / den, F(0))
    return out.reshape(shape)
