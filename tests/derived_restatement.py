"""The derived per-particle fields ("Derived fields") restated in numpy, operation by operation.

derive(): every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its own
like the device code (no FMA, IEEE divide).  Imports nothing from the product and nothing from the other
restatements.  It is fed by the grid the sweep walked: the cell-sorted positions and velocities and the cell table's
{start, end} ranges (sph_download_grid + sph_download_state, or the oracle's sort and table), and returns its results
per ROW of that stream.

Sums are formed with np.cumsum in float32 over a row that begins with +0, which adds strictly left to right from +0:
the accumulation order of the definition (dz, dy, dx from -1 to 1 in that nesting, each cell's rows in stream order).
A candidate that is not taken contributes a SELECTED +0 term, np.where(take, term, 0): that changes no bit, because a
sum that starts at +0 is never -0 under round-to-nearest.

derive_f64(): the same sums in float64 over the candidates the fp32 walk took, with, for a unit roundoff u, a bound
on what a computation of that roundoff may be away from the exact value (tests/test_derived_cpu.py derives it)."""
import numpy as np

F = np.float32
MASS = F(0.02)
SIX = F(6)
SUMS = ("rho", "gx", "gy", "gz", "s", "cx", "cy", "cz")


def row_cells(pos, h, D):
    """sweep_cell: (int)(x / h) per axis, clamped to 0 .. D - 1"""
    q = np.asarray(pos, dtype=F) / F(h)
    assert q.dtype == F and np.isfinite(q).all()
    return np.clip(q.astype(np.int64), 0, int(D) - 1)


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
    """left-to-right sum of every row in the terms' own type, starting from +0"""
    zero = np.zeros((terms.shape[0], 1), terms.dtype)
    return np.cumsum(np.concatenate([zero, terms], axis=1), axis=1, dtype=terms.dtype)[:, -1]


def _inputs(pos, vel, cell_ranges):
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    return pos, vel, np.asarray(cell_ranges, dtype=np.int32).reshape(-1, 2)


def _groups(pos, cell_ranges, h, D):
    """(rows of one cell, their candidates) for every occupied cell"""
    c = row_cells(pos, h, D)
    key = (c[:, 2] * D + c[:, 1]) * D + c[:, 0]
    for k in np.unique(key):
        who = np.flatnonzero(key == k)
        yield who, neighbourhood(cell_ranges, D, int(k % D), int(k // D % D), int(k // (D * D)))


def _pair_terms(pos, vel, who, j, h2, dcoef, T):
    """e, u, d2, diff of every (row, candidate) pair in type T, one ufunc per operation"""
    p, v = pos.astype(T), vel.astype(T)
    e = [p[None, j, a] - p[who, None, a] for a in range(3)]
    u = [v[None, j, a] - v[who, None, a] for a in range(3)]
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    diff = T(h2) - d2
    assert d2.dtype == T and diff.dtype == T
    return e, u, d2, diff


def derive(pos, vel, cell_ranges, h, dcoef, D):
    """pos (n, 3), vel (n, 3): the SORTED stream; cell_ranges (D^3, 2) int32.  Per row of the stream:
    {"vorticity" (n, 3), "divergence" (n,), "grad_rho" (n, 3), "rho" (n,): float32; "neighbours" (n,): uint32;
    "sums" (n, 8): the eight float sums in the order of SUMS}."""
    pos, vel, cell_ranges = _inputs(pos, vel, cell_ranges)
    D, n = int(D), len(pos)
    h2 = F(h) * F(h)
    sums = np.zeros((n, 8), F)
    count = np.zeros(n, np.uint32)
    for who, j in (_groups(pos, cell_ranges, h, D) if n else ()):
        with np.errstate(all="ignore"):
            e, u, d2, diff = _pair_terms(pos, vel, who, j, h2, dcoef, F)
            take = ~(d2 > h2)
            a = (F(dcoef) * diff) * diff
            m = MASS * (a * diff)
            w = MASS * a
            terms = [m, w * e[0], w * e[1], w * e[2],
                     w * ((u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]),
                     w * (e[1] * u[2] - e[2] * u[1]),
                     w * (e[2] * u[0] - e[0] * u[2]),
                     w * (e[0] * u[1] - e[1] * u[0])]
        for k, t in enumerate(terms):
            assert t.dtype == F
            sums[who, k] = sum_from_zero(np.where(take, t, F(0)))
        count[who] = take.sum(axis=1)
    rho = sums[:, 0]
    some = rho > F(0)
    with np.errstate(all="ignore"):
        grad = SIX * sums[:, 1:4]
        div = np.where(some, (SIX * sums[:, 4]) / rho, F(0))
        vort = np.where(some[:, None], (SIX * sums[:, 5:8]) / rho[:, None], F(0))
    assert grad.dtype == div.dtype == vort.dtype == F
    return dict(vorticity=vort, divergence=div, grad_rho=grad, rho=rho.copy(), neighbours=count, sums=sums)


def derive_f64(pos, vel, cell_ranges, h, dcoef, D, u):
    """The same eight sums in float64 over the candidates the fp32 walk takes (fp32 d2 <= fp32 h*h), and the results
    formed from them in float64.  -> {"sums" (n, 8), "bound" (n, 8), "taken" (n,), "vorticity", "divergence",
    "grad_rho", "rho"}.  bound: what a left-to-right evaluation in which every operation has relative error <= u may
    be away from the exact sums, as tests/test_derived_cpu.py derives it; the float64 sums themselves are such an
    evaluation with u = 2^-53."""
    pos, vel, cell_ranges = _inputs(pos, vel, cell_ranges)
    D, n = int(D), len(pos)
    T = np.float64
    h2f = F(h) * F(h)
    h2, c, mass = T(h2f), T(F(dcoef)), T(MASS)
    sums, bound, taken = np.zeros((n, 8), T), np.zeros((n, 8), T), np.zeros(n, np.int64)
    g5, g4 = (1 + u) ** 5 - 1, (1 + u) ** 4 - 1
    for who, j in (_groups(pos, cell_ranges, h, D) if n else ()):
        with np.errstate(all="ignore"):
            _, _, d2f, _ = _pair_terms(pos, vel, who, j, h2f, dcoef, F)
        take = ~(d2f > h2f)
        e, v, d2, diff = _pair_terms(pos, vel, who, j, h2f, dcoef, T)
        ad = np.abs(diff)
        dd = d2 * g5 * (1 + u) + u * ad                              # |computed diff - diff|
        q = [np.ones_like(d2), e[0], e[1], e[2],
             (v[0] * e[0] + v[1] * e[1]) + v[2] * e[2],
             e[1] * v[2] - e[2] * v[1], e[2] * v[0] - e[0] * v[2], e[0] * v[1] - e[1] * v[0]]
        ae, av = [np.abs(x) for x in e], [np.abs(x) for x in v]
        # |computed q - q|: e and u are one rounding each, a product of two one more, and the adds after it
        dq = [np.zeros_like(d2), ae[0] * u, ae[1] * u, ae[2] * u,
              (av[0] * ae[0] + av[1] * ae[1] + av[2] * ae[2]) * g5,
              (ae[1] * av[2] + ae[2] * av[1]) * g4, (ae[2] * av[0] + ae[0] * av[2]) * g4, (ae[0] * av[1] + ae[1] * av[0]) * g4]
        K = take.sum(axis=1)
        for k in range(8):
            p = 3 if k == 0 else 2
            exact = mass * c * diff ** p * q[k]
            top = mass * c * (ad + dd) ** p * (np.abs(q[k]) + dq[k]) * (1 + u) ** 4   # >= |computed term|
            sums[who, k] = np.where(take, exact, 0.0).sum(axis=1)
            per_term = np.where(take, top - np.abs(exact), 0.0).sum(axis=1)
            adds = ((1 + u) ** np.maximum(K - 1, 0) - 1) * np.where(take, top, 0.0).sum(axis=1)
            bound[who, k] = per_term + adds
        taken[who] = K
    rho = sums[:, 0]
    some = rho > 0
    safe = np.where(some, rho, 1.0)
    return dict(sums=sums, bound=bound, taken=taken, rho=rho.copy(), grad_rho=6.0 * sums[:, 1:4],
                divergence=np.where(some, 6.0 * sums[:, 4] / safe, 0.0),
                vorticity=np.where(some[:, None], 6.0 * sums[:, 5:8] / safe[:, None], 0.0))
