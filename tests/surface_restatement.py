"""The surface mesh restated in numpy: marching tetrahedra over a lattice of fp32 values.
The tables are derived here, at import, from the geometry alone -- independently of csrc/surface_tables.h, which
tests/test_surface_cpu.py holds against them entry by entry."""
import itertools

import numpy as np

F = np.float32

# the seven edges a point owns, as (dx, dy, dz), and the six Kuhn tetrahedra as permutations of the axes
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def tet_path(perm):
    """the corners c0..c3 of the tetrahedron, as (dx, dy, dz)"""
    c = [0, 0, 0]
    path = [tuple(c)]
    for axis in perm:
        c[axis] = 1
        path.append(tuple(c))
    return path


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _triangles(path, case):
    """the triangles of one tetrahedron: lists of three edges (inside position, outside position), wound, and
    whether each was swapped"""
    ins = [p for p in range(4) if case >> p & 1]
    outs = [p for p in range(4) if not case >> p & 1]
    if len(ins) in (0, 4):
        return [], []
    if len(ins) == 1:
        tris = [[(ins[0], outs[0]), (ins[0], outs[1]), (ins[0], outs[2])]]
    elif len(ins) == 3:
        tris = [[(ins[0], outs[0]), (ins[1], outs[0]), (ins[2], outs[0])]]
    else:
        q = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    # from the centroid of O to the centroid of I, scaled to integers
    gi = [sum(path[p][k] for p in ins) * len(outs) for k in range(3)]
    go = [sum(path[p][k] for p in outs) * len(ins) for k in range(3)]
    g = [gi[k] - go[k] for k in range(3)]
    wound, swapped = [], []
    for tri in tris:
        mid = [[path[a][k] + path[b][k] for k in range(3)] for a, b in tri]   # twice the midpoints
        n = _cross([mid[1][k] - mid[0][k] for k in range(3)], [mid[2][k] - mid[0][k] for k in range(3)])
        side = sum(n[k] * g[k] for k in range(3))
        assert side != 0
        swapped.append(side > 0)
        wound.append([tri[0], tri[2], tri[1]] if side > 0 else tri)
    return wound, swapped


def _edge(path, a, b):
    """the edge between path positions a and b as (owner offset, direction d)"""
    lo, hi = min(a, b), max(a, b)
    d = DIRS.index(tuple(path[hi][k] - path[lo][k] for k in range(3)))
    return path[lo], d


def make_tables():
    """TABLE[sigma][case] = list of triangles, each three (owner offset (dx, dy, dz), d); SWAPPED alongside"""
    table, swaps = [], []
    for perm in PERMS:
        path = tet_path(perm)
        rows, srows = [], []
        for case in range(16):
            tris, sw = _triangles(path, case)
            rows.append([[_edge(path, a, b) for a, b in tri] for tri in tris])
            srows.append(sw)
        table.append(rows)
        swaps.append(srows)
    return table, swaps


TABLE, SWAPPED = make_tables()


def corner_number(off):
    return off[0] + 2 * off[1] + 4 * off[2]


def _shift(a, off):
    """a[z + dz, y + dy, x + dx] over the points where that exists, and the slices of those points"""
    dx, dy, dz = off
    nz, ny, nx = a.shape
    own = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
    far = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
    return own, a[far]


def extract(field, origin, spacing, iso):
    """field: (nz, ny, nx) float32.  Returns (vertices float32 (V, 3), triangles uint32 (T, 3), detail) where detail
    holds per vertex its owner L, direction d and t."""
    f = np.ascontiguousarray(field, dtype=F)
    nz, ny, nx = f.shape
    iso = F(iso)
    origin = [F(o) for o in origin]
    spacing = [F(s) for s in (spacing if np.ndim(spacing) else (spacing,) * 3)]
    with np.errstate(invalid="ignore"):
        inside = f >= iso
    N = nz * ny * nx
    crossed = np.zeros((nz, ny, nx, 7), bool)
    for d, off in enumerate(DIRS):
        own, far = _shift(inside, off)
        crossed[own + (d,)] = inside[own] != far
    flat = crossed.reshape(N * 7)
    vidx = (np.cumsum(flat) - flat).reshape(nz, ny, nx, 7)          # number of the vertex on edge (L, d)
    V = int(flat.sum())
    coords = [origin[k] + np.arange(n, dtype=np.int64).astype(F) * spacing[k] for k, n in enumerate((nx, ny, nz))]
    verts = np.zeros((V, 3), F)
    owner_L = np.zeros(V, np.int64)
    owner_d = np.zeros(V, np.int64)
    ts = np.zeros(V, F)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for d, off in enumerate(DIRS):
        sel = crossed[..., d]
        if not sel.any():
            continue
        z, y, x = iz[sel], iy[sel], ix[sel]
        fa = f[z, y, x]
        fb = f[z + off[2], y + off[1], x + off[0]]
        with np.errstate(all="ignore"):
            t = ((iso - fa) / (fb - fa)).astype(F)
        k = vidx[..., d][sel]
        for axis, (i, o) in enumerate(((x, off[0]), (y, off[1]), (z, off[2]))):
            pa, pb = coords[axis][i], coords[axis][i + o]
            with np.errstate(all="ignore"):
                verts[k, axis] = pa + (t * (pb - pa)).astype(F)
        owner_L[k] = (z * ny + y) * nx + x
        owner_d[k] = d
        ts[k] = t
    # triangles, cell by cell
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    cellL = ((iz * ny + iy) * nx + ix)[:cz, :cy, :cx]
    keys, tris = [], []
    for s, perm in enumerate(PERMS):
        path = tet_path(perm)
        case = np.zeros((cz, cy, cx), np.int64)
        for p, off in enumerate(path):
            case |= inside[off[2]:off[2] + cz, off[1]:off[1] + cy, off[0]:off[0] + cx].astype(np.int64) << p
        for c in range(1, 15):
            sel = case == c
            if not sel.any():
                continue
            for k, tri in enumerate(TABLE[s][c]):
                idx = [vidx[off[2]:off[2] + cz, off[1]:off[1] + cy, off[0]:off[0] + cx, d][sel] for off, d in tri]
                tris.append(np.stack(idx, axis=1))
                keys.append(np.stack([cellL[sel], np.full(int(sel.sum()), s), np.full(int(sel.sum()), k)], axis=1))
    if tris:
        tris = np.concatenate(tris)
        keys = np.concatenate(keys)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        tris = tris[order].astype(np.uint32)
    else:
        tris = np.zeros((0, 3), np.uint32)
    return verts, tris, dict(L=owner_L, d=owner_d, t=ts)


# ---- what the tests ask of a mesh ----
def directed_edges(tris):
    """every directed edge (a, b) of the triangles, as a * 2^32 + b"""
    t = tris.astype(np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return e[:, 0] << 32 | e[:, 1]


def edge_pairing(tris):
    """(largest multiplicity of a directed edge, directed edges whose reverse does not occur exactly once)"""
    e = directed_edges(tris)
    if not len(e):
        return 0, np.zeros((0, 2), np.int64)
    uniq, counts = np.unique(e, return_counts=True)
    rev = (uniq & 0xFFFFFFFF) << 32 | uniq >> 32
    pos = np.searchsorted(uniq, rev)
    pos[pos >= len(uniq)] = 0
    paired = (uniq[pos] == rev) & (counts[pos] == 1)
    lone = uniq[~paired]
    return int(counts.max()), np.stack([lone >> 32, lone & 0xFFFFFFFF], axis=1)


def euler(verts, tris):
    """V - E + F with E the undirected edges"""
    t = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64), axis=1)
    E = len(np.unique(t[:, 0] << 32 | t[:, 1]))
    return len(verts) - E + len(tris)


def signed_volume(verts, tris):
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)
