"""The tracer sets the CPU and the GPU tests of the tracers share (float32 (m, 3) arrays), and the count of groups
per wave the walk kernel must report, computed from the tracers' cells alone.  Imports nothing from the product."""
import numpy as np

F = np.float32
SHIFT = np.array([0.003, -0.002, 0.001], F)


def blob():
    """A: 200 points in the cell [4.10, 4.20) x [1.10, 1.20) x [4.10, 4.20): one group, four waves, the last partial"""
    lo = np.array([4.10, 1.10, 4.10])
    return np.ascontiguousarray(lo + 0.1 * np.random.default_rng(1).random((200, 3)), dtype=F)


def line():
    """B: 130 points along x through seven cells of one row, over the x-block boundary at cell 40"""
    p = np.empty((130, 3), F)
    p[:, 0] = F(3.85) + F(0.005) * np.arange(130, dtype=np.int32).astype(F)
    p[:, 1] = F(1.15)
    p[:, 2] = F(4.15)
    return p


def scatter(pos):
    """C: particles 0 .. 149 shifted off their positions"""
    return np.ascontiguousarray(np.asarray(pos, dtype=F)[:150] + SHIFT)


def row_sets(pos, h, D):
    """D: for every g from 1 to the number of (cy, cz) rows of cells the particles occupy (at most 25), 64 tracers
    at particle positions drawn from exactly g distinct rows"""
    pos = np.asarray(pos, dtype=F)
    c = (pos / F(h)).astype(np.int32)
    row = c[:, 2].astype(np.int64) * D + c[:, 1]
    rows = np.unique(row)[:25]
    members = [np.flatnonzero(row == r) for r in rows]
    out = []
    for g in range(1, len(rows) + 1):
        pick = [members[k % g][(k // g) % len(members[k % g])] for k in range(64)]
        out.append(np.ascontiguousarray(pos[pick]))
    return out


def specials(pos):
    """E: outside and special values, one tracer exactly on particle 7, three identical tracers, cells 0 and D - 1"""
    a = [float(v) for v in np.asarray(pos, dtype=F)[7]]
    nan = np.array([0x7FC12345], np.uint32).view(F)[0]              # a NaN with a payload
    rows = [(-0.05, a[1], a[2]), (a[0], 10.0, a[2]), (a[0], a[1], nan), (np.inf, a[1], a[2]), (a[0], -np.inf, a[2]),
            (-0.0, a[1], a[2]), (0.0, 0.0, 0.0), tuple(a), (4.15, 1.15, 4.15), (4.15, 1.15, 4.15), (4.15, 1.15, 4.15),
            (0.05, 0.05, 0.05), (9.95, 9.95, 9.95), (9.95, 0.05, 4.15), (nan, nan, nan), (-0.0, -0.0, -0.0)]
    out = np.array(rows, dtype=F)
    w = out.view(np.uint32)                                         # (word for word: the payload survives)
    w[2, 2] = 0x7FC12345
    w[14, :] = (0x7FC12345, 0xFFC00001, 0x7FC00000)
    return out


def all_sets(pos, h, D):
    """name -> tracers, for a state with particle positions `pos` (id order)"""
    sets = {"A": blob(), "B": line(), "C": scatter(pos), "E": specials(pos)}
    for m in (1, 63, 64, 65):
        sets["E%d" % m] = np.ascontiguousarray(blob()[:m])
    for g, t in enumerate(row_sets(pos, h, D), start=1):
        sets["D%d" % g] = t
    return sets


def wave_groups(tracers, h, D, block_x=8):
    """groups per wave of 64 tracers in the order of a stable sort by cell key (outside tracers last): a group is
    one (cy, cz) row of cells and one block of `block_x` cells in x; outside tracers belong to none"""
    t = np.asarray(tracers, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = t / F(h)
        outside = (~(t >= F(0)) | ~(q < F(D))).any(axis=1)
        c = np.where(outside[:, None], F(0), q).astype(np.int64)
    key = np.where(outside, D ** 3, (c[:, 2] * D + c[:, 1]) * D + c[:, 0])
    group = np.where(outside, -1, (c[:, 2] * D + c[:, 1]) * D + c[:, 0] // block_x * block_x)
    order = np.argsort(key, kind="stable")
    g = group[order]
    return [len(set(g[w:w + 64].tolist()) - {-1}) for w in range(0, len(g), 64)]


# ---- the same sets for any grid: `pos` the particle positions (id order), cells of size h, D per axis ----

def crowded_cell(pos, h, D):
    """(cx, cy, cz) of the cell that holds the most particles (the first in key order among equals)"""
    c = (np.asarray(pos, dtype=F) / F(h)).astype(np.int64)
    key = (c[:, 2] * D + c[:, 1]) * D + c[:, 0]
    keys, count = np.unique(key, return_counts=True)
    k = int(keys[np.argmax(count)])
    return k % D, k // D % D, k // (D * D)


def blob_in(cell, h, m=200, seed=1):
    """A: m points inside the middle 90 % of `cell`: one group, four waves, the last partial (m = 200)"""
    lo = np.asarray(cell, dtype=np.float64)
    return np.ascontiguousarray((lo + 0.05 + 0.9 * np.random.default_rng(seed).random((m, 3))) * float(F(h)), dtype=F)


def line_cells(D):
    """the stretch of x the line covers, in cells: the whole row where D < 8, else 6.5 cells around the block
    boundary 7|8 (ending 0.05 cells below the box where D < 12)"""
    if D < 8:
        return 0.02, D - 0.02
    lo = min(4.75, D - 6.55)
    return lo, lo + 6.5


def line_in(pos, h, D):
    """B: 130 points along x through the middle of the row (cy, cz) of the most crowded cell"""
    _, cy, cz = crowded_cell(pos, h, D)
    lo, hi = line_cells(D)
    hf = float(F(h))
    p = np.empty((130, 3), F)
    p[:, 0] = np.linspace(lo * hf, hi * hf, 130, endpoint=False).astype(F)
    p[:, 1] = F((cy + 0.5) * hf)
    p[:, 2] = F((cz + 0.5) * hf)
    return p


def scatter_in(pos, h, m=150):
    """C: m particle positions (cycled where the state has fewer), shifted by SHIFT in units of h / 0.1"""
    pos = np.asarray(pos, dtype=F)
    shift = (SHIFT.astype(np.float64) * (float(F(h)) / 0.1)).astype(F)
    return np.ascontiguousarray(pos[np.arange(m) % len(pos)] + shift)


def specials_in(pos, h, D):
    """E: specials() rebuilt from h and D: -0.05 h and exactly `box` (both outside), NaNs with payloads, +-inf, -0.0,
    one tracer exactly on particle 7, three identical tracers in the most crowded cell, cells 0 and D - 1"""
    hf = float(F(h))
    box = float(F(h) * F(D))
    a = [float(v) for v in np.asarray(pos, dtype=F)[7]]
    b = tuple((c + 0.5) * hf for c in crowded_cell(pos, h, D))
    nan = np.array([0x7FC12345], np.uint32).view(F)[0]
    last = box - 0.5 * hf
    rows = [(-0.05 * hf, a[1], a[2]), (a[0], box, a[2]), (a[0], a[1], nan), (np.inf, a[1], a[2]), (a[0], -np.inf, a[2]),
            (-0.0, a[1], a[2]), (0.0, 0.0, 0.0), tuple(a), b, b, b,
            (0.5 * hf,) * 3, (last,) * 3, (last, 0.5 * hf, b[2]), (nan, nan, nan), (-0.0, -0.0, -0.0)]
    out = np.array(rows, dtype=F)
    w = out.view(np.uint32)
    w[2, 2] = 0x7FC12345
    w[14, :] = (0x7FC12345, 0xFFC00001, 0x7FC00000)
    return out


SPECIALS_OUTSIDE = [0, 1, 2, 3, 4, 14]      # the rows of specials_in() that lie outside every grid


def outside_interleaved(h, D, seed=2):
    """F: 128 tracers in caller order, 88 in cell (0, 0, 0) and 40 outside the grid (below 0, at and beyond `box`,
    a NaN, an infinity), alternating inside / outside until the 40 are used up.  Sorted with the outside key
    behind every cell, the waves hold [64 inside] and [24 inside, 40 outside]: wave_groups gives [1, 1]."""
    hf = float(F(h))
    box = float(F(h) * F(D))
    rng = np.random.default_rng(seed)
    inside = ((0.05 + 0.9 * rng.random((88, 3))) * hf).astype(F)
    outside = ((0.05 + 0.9 * rng.random((40, 3))) * hf).astype(F)
    for k in range(40):
        axis = k % 3
        outside[k, axis] = [F(-0.05 * hf) * F(1 + k), F(box), F(box) + F(hf) * F(k), F(np.nan), F(np.inf)][k % 5]
    out = np.empty((128, 3), F)
    out[0:80:2] = inside[:40]
    out[1:80:2] = outside
    out[80:] = inside[40:]
    return out


def many_in(pos, h, m=4097):
    """G: m tracers at particle positions, cycled; every cycle through the particles shifted once more by SHIFT in
    units of h / 0.1 (more than four 1,024-key tiles of the tracers' sort)"""
    pos = np.asarray(pos, dtype=F)
    k = np.arange(m)
    shift = SHIFT.astype(np.float64) * (float(F(h)) / 0.1)
    return np.ascontiguousarray(pos[k % len(pos)].astype(np.float64) + (1 + k // len(pos))[:, None] * shift, dtype=F)


def grid_sets(pos, h, D):
    """name -> tracers, for a state on any grid"""
    sets = {"F": outside_interleaved(h, D), "A": blob_in(crowded_cell(pos, h, D), h), "B": line_in(pos, h, D),
            "C": scatter_in(pos, h), "E": specials_in(pos, h, D), "G": many_in(pos, h)}
    for g, t in enumerate(row_sets(pos, h, D), start=1):
        sets["D%d" % g] = t
    return sets
