"""What tests/test_walk_grids_cpu.py (restatements, without a GPU) and tests/test_gpu_walk_grids.py (the kernels) share:
the grids of tests/grid_states.py the point walks are held to, the lattices of the field sample on them, and the D7
state with one long run.  Imports nothing from the product.  A lattice is (origin, spacing, (nz, ny, nx))."""
import numpy as np

import grid_states as G
import tracer_sets as TS

F = np.float32
GRIDS = ["D1", "D2", "D3", "D7", "D10h025", "D11", "D40", "D101", "D102", "D161h005", "D256", "D257"]
WIDE = ("D256", "D257")       # the grids that get the lattice whose lanes lie two cells apart
SHAPE = (3, 3, 130)           # two bricks of 64 lanes and a two-lane tail, nine lattice rows
LONG_CELL = (3, 3, 3)         # D7: the cell the long run lies in
LONG_ROWS = 1500


def anchor(pos, h, D):
    """the particle of the most crowded cell that lies nearest to that cell's centre, as three Python floats"""
    pos = np.asarray(pos, dtype=F)
    cell = np.array(TS.crowded_cell(pos, h, D))
    inside = np.flatnonzero((G.cells_of(pos, h) == cell).all(axis=1))
    d = np.abs(pos[inside].astype(np.float64) / float(F(h)) - (cell + 0.5)).max(axis=1)
    return tuple(float(v) for v in pos[inside[np.argmin(d)]])


def lattices(name, pos, h, D):
    """name -> lattice, around anchor(pos):
    "row":  x in steps of h / 3 (43 cells) from one spacing below 0 (past the box on the small grids), or centred on
            the anchor where that would not reach it; the y rows -0.3 h (outside the grid), the anchor's, and as far
            again beyond it; the z rows h / 2 apart.
    "fine": 130 points across the anchor's support in x (h / 65 apart), the y and z rows h / 3 apart: every point
            sees the anchor's cell; three bricks inside at most three cells.
    "wide": (D256, D257) x from one spacing below 0 in steps of box / 128, two cells and more: every lane of a brick
            has a window of its own and the first brick's hull is half the row of cells, the anchor's row and its
            y and z neighbours h / 3 away; the x origin is shifted by less than a spacing so that a point falls on
            the anchor's x.
    "span": (D256, D257) the same with 65 points box / 63 apart, more than four cells: the windows of two lanes
            never touch, and the hull of the first brick is the whole row of 256 or 257 cells."""
    hf = float(F(h))
    ax, ay, az = anchor(pos, h, D)
    ox = -hf / 3 if ax < 40 * hf else ax - 65 * hf / 3
    out = {"row": ((ox, -0.3 * hf, az - hf / 2), (hf / 3, ay + 0.3 * hf, hf / 2), SHAPE),
           "fine": ((ax - hf, ay - hf / 3, az - hf / 3), (hf / 65, hf / 3, hf / 3), SHAPE)}
    if name in WIDE:
        sp = float(G.box_of(h, D)) / 128
        out["wide"] = ((ax % sp - sp, ay - hf / 3, az - hf / 3), (sp, hf / 3, hf / 3), SHAPE)
        sp = float(G.box_of(h, D)) / 63
        out["span"] = ((ax % sp - sp, ay - hf / 3, az - hf / 3), (sp, hf / 3, hf / 3), (3, 3, 65))
    return out


def long_run_state():
    """D7's state with rows 0 .. LONG_ROWS - 1 moved into the middle 90 % of LONG_CELL -> pos, vel, g"""
    pos, vel, g = G.grid_state("D7")
    pos = pos.copy()
    rng = np.random.default_rng(21)
    pos[:LONG_ROWS] = ((np.array(LONG_CELL) + 0.05 + 0.9 * rng.random((LONG_ROWS, 3))) * float(F(g["h"]))).astype(F)
    c = G.assert_inside(pos, g["h"], g["cells"], "the long run")
    assert (c[:LONG_ROWS] == LONG_CELL).all()
    return np.ascontiguousarray(pos), vel, g


def long_run_sets(h):
    """name -> tracers: a blob of 200 in the long run's cell and in each of its two x-neighbours, and the three as one
    set of 600 (waves that hold two cells)"""
    cx, cy, cz = LONG_CELL
    sets = {"L%d" % dx: TS.blob_in((cx + dx, cy, cz), h, seed=30 + dx) for dx in (-1, 0, 1)}
    sets["Lall"] = np.ascontiguousarray(np.concatenate([sets["L-1"], sets["L0"], sets["L1"]]))
    return sets


def long_run_lattice(h, D):
    """130 points in x from 0.05 h below 0 to 0.05 h beyond the box through the long run's cell, rows h / 3 apart"""
    hf = float(F(h))
    cx, cy, cz = LONG_CELL
    return (-0.05 * hf, (cy + 0.5) * hf - hf / 3, (cz + 0.5) * hf - hf / 3), ((D + 0.1) * hf / 129, hf / 3, hf / 3), SHAPE
