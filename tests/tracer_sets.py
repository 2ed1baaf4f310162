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
