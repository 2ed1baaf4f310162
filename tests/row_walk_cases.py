"""What tests/test_row_walks_cpu.py (restatements, without a GPU) and tests/test_gpu_row_walks.py (the kernels) share:
the states the six passes that walk the nine runs around every ROW of the sorted stream -- derived fields, neighbour
lists, bodies, per-body moments, body tracks, pair statistics -- are held to off the reference's 100^3 grid, the lengths they are asked
for, and a plain restatement of what the staged row walk (walk_common.h, walk_runs_staged) counts.  The grids are
walk_grid_cases.GRIDS.  Imports nothing from the product."""
import functools

import numpy as np

import bodies_restatement as BR
import grid_states as G
import neighbour_restatement as NR
import neighbour_states as NS
import walk_grid_cases as W

F = np.float32
GRIDS = list(W.GRIDS)
CUBE_ROWS = 600             # rows moved into the cube, and the first row put on the walls by walls()
CUBE_SIDE = 3.0             # in cells
SEED = 77
D1_ROWS = 256               # the rows of D1's state here: four waves in the one cell
# the floors row_state() asserts (D1 .. D3 are one body or two and get no cube: the list floors alone)
MIN_ENTRIES, MIN_LONGEST = 30000, 100         # neighbour lists at radius h
MIN_BODIES, MIN_BIG_BODY = 50, 64             # at link 0.3 h: bodies of two or more rows, the rows of the largest
MIN_ONE_BODY = 600                            # at link 0.5 h: the rows of the largest body
long_run_state = W.long_run_state


def radii(h):
    """the neighbour radii and the link lengths of every case: 0 (which means h), 0.5 h, 0.3 h"""
    return (0.0, 0.5 * float(h), 0.3 * float(h))


def cube_rows(name):
    """the rows row_state() moves: 0 .. 599; on D102 the 600 rows after its own cluster"""
    first = G.CLUSTER_ROWS if name == "D102" else 0
    return np.arange(first, first + CUBE_ROWS)


def reach(pos, h, D):
    """what a state gives the row passes, over a grid built on the CPU -> dict(entries, longest: the lists at radius
    h; bodies, biggest: the bodies of two or more rows and the largest body's rows at link 0.3 h; one_body: the
    largest body's rows at link 0.5 h)"""
    offsets, _ = NR.all_pairs(pos, h, 0.0)
    out = dict(entries=int(offsets[-1]), longest=int(np.diff(offsets.astype(np.int64)).max()))
    rows, ids, cells = NR.grid_of(pos, h, D)
    count = BR.bodies(rows, ids, cells, h, D, 0.3 * float(h))["table"][:, 1]
    out.update(bodies=int((count >= 2).sum()), biggest=int(count.max()))
    out["one_body"] = int(BR.bodies(rows, ids, cells, h, D, 0.5 * float(h))["table"][:, 1].max())
    return out


@functools.lru_cache(maxsize=None)
def _row_state(name):
    pos, vel, g = G.grid_state(name)
    h, D = g["h"], g["cells"]
    if name == "D1":
        # its 40 rows can list 40 x 39 = 1,560 entries at the most: the state keeps them and gains rows of the same kind
        more = G.state(D1_ROWS - len(pos), h, D, SEED)
        pos, vel = np.concatenate([pos, more[0]]), np.concatenate([vel, more[1]])
    if D >= 4:
        # 3,001 rows in 64,000 cells and more are too sparse for a row pass: 600 of them into a cube of three cells
        # a side about the cell corner (c, c, c) h, c = min(8, D / 2): four cells per axis, and from D = 16 on across
        # the boundary between the cells 7 and 8 (two blocks of eight cells of a row)
        c = min(8, D // 2)
        rng = np.random.default_rng(SEED)
        pos[cube_rows(name)] = ((c - CUBE_SIDE / 2 + CUBE_SIDE * rng.random((CUBE_ROWS, 3))) * float(F(h))).astype(F)
    G.assert_inside(pos, h, D, name)
    got = reach(pos, h, D)
    assert got["entries"] >= MIN_ENTRIES and got["longest"] >= MIN_LONGEST, (name, got)
    if D >= 4:
        assert got["bodies"] >= MIN_BODIES and got["biggest"] >= MIN_BIG_BODY and got["one_body"] >= MIN_ONE_BODY, (name, got)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel, g, got


def row_state(name):
    """-> pos, vel, g: grid_states.grid_state(name) with, where D >= 4, CUBE_ROWS rows moved into a cube of side 3 h
    (uniform, a fixed seed); D1's 40 rows are followed by 216 more (len(pos), not g["n"], is the row count); the
    floors above are asserted.  The arrays are the caller's own."""
    pos, vel, g, _ = _row_state(name)
    return pos.copy(), vel.copy(), g


def reached(name):
    """what row_state(name) reaches (reach() of it)"""
    return dict(_row_state(name)[3])


def walls(name):
    """row_state(name) with rows moved onto the wall planes (neighbour_states.put_on_the_walls): the rows from
    CUBE_ROWS on where a cube was made, so that it stays whole, else the first ones.  Cells 0 and D - 1 take part."""
    pos, vel, g = row_state(name)
    first = CUBE_ROWS if g["cells"] >= 4 else 0
    return NS.put_on_the_walls(pos, g, name + " on the walls", first), vel, g


def staged_direct(pos_rows, cell_ranges, h, D, slice):
    """What walk_runs_staged counts over a sorted stream: for every 64 consecutive rows (one wave) and each of the
    nine runs r = (dz, dy), the union [u0, u1) of the lanes' runs -- a lane's run reaches from the start of the first
    non-empty cell to the end of the last non-empty cell among cx - 1 .. cx + 1 of the row of cells (cy + dy, cz +
    dz), and is empty where that row lies outside the grid.  Nothing is counted where every lane's run is empty; the
    union is walked from global memory (direct) where u1 - u0 > slice, and staged otherwise.  -> (staged, direct)"""
    cell_ranges = np.asarray(cell_ranges).reshape(-1, 2)
    D, n = int(D), len(pos_rows)
    cells = BR.row_cells(pos_rows, h, D).tolist()
    staged = direct = 0
    for wave in range(0, n, 64):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                u0 = u1 = None
                for cx, cy, cz in cells[wave:wave + 64]:
                    sy, sz = cy + dy, cz + dz
                    if sy < 0 or sy >= D or sz < 0 or sz >= D:
                        continue
                    runs = [cell_ranges[(sz * D + sy) * D + sx] for sx in range(max(cx - 1, 0), min(cx + 1, D - 1) + 1)]
                    runs = [(int(s), int(e)) for s, e in runs if e > s]
                    if not runs:
                        continue
                    s, e = max(runs[0][0], 0), min(runs[-1][1], n)
                    u0 = s if u0 is None else min(u0, s)
                    u1 = e if u1 is None else max(u1, e)
                if u0 is None:
                    continue
                if u1 - u0 > slice:
                    direct += 1
                else:
                    staged += 1
    return staged, direct
