"""Settings and states on grids other than the reference's 100^3, by name, for tests/test_gpu_grids.py (GPU against
the oracle) and tests/test_grids_cpu.py (the oracle against float64, and every precondition below, without a GPU).
One row of GRIDS per sort plan of sort.hip's digit_bits(): the key width of a D^3 table selects the plan.
Every builder asserts its own preconditions."""
import ctypes as C

import numpy as np

from oracle import oracle as O

F = np.float32
REST_DENSITY = F(1000.0)
PUSH_STRENGTH = 5.0
CLICK = (400, 300)          # window pixel of the click tests: the middle of the box
BOX_MIN_X, BOX_MAX_X, BOX_MIN_Y, BOX_MAX_Y = 200, 600, 150, 450


def kernel_coeffs(h):
    """(v_kernel_coeff, d_kernel_coeff) formed in fp32 from h the way main() does (main.cpp:57-63)"""
    hf = F(h)
    v = float(F(45.0) / (F(3.14159265) * F(float(hf) ** 6)))
    d = float(F(315.0) / (F(64.0) * F(3.14159265) * F(float(hf) ** 9)))
    return v, d


def box_of(h, cells):
    return F(h) * F(cells)


def settings_for(n, h, cells, dt=0.004, factory=None):
    """A Settings struct (factory(n, random_init): the library's default_settings, or the oracle's by default) for
    `cells` cells of size h per axis."""
    s = (factory or O.make_settings)(n, False)
    s.h = h
    s.boxDim = float(box_of(h, cells))
    s.numCellsPerDim = cells
    s.timestep = dt
    s.v_kernel_coeff, s.d_kernel_coeff = kernel_coeffs(s.h)
    return s


def oracle_sim(s):
    """An OracleSim that runs the settings `s` (any layout-identical Settings struct)"""
    ref = O.OracleSim(s.numParticles, False)
    C.memmove(C.byref(ref.settings), C.byref(s), C.sizeof(ref.settings))
    ref.close()
    ref._h = O.lib().oracle_sim_create(C.byref(ref.settings))
    return ref


def cells_of(pos, h):
    """(int)(p / h), the fp32 divide of getGridCell"""
    q = np.asarray(pos, F) / F(h)
    assert q.dtype == F
    return q.astype(np.int64)


def assert_inside(pos, h, cells, what=""):
    c = cells_of(pos, h)
    assert (np.asarray(pos) >= 0).all() and c.min() >= 0 and c.max() < cells, f"{what}: a position outside the grid"
    return c


def key_bits(cells):
    """sph_step.hip's key_bits(): the width the library sorts for a D^3 table"""
    bits = 1
    while (1 << bits) < cells ** 3:
        bits += 1
    return bits


def plan_of(bits):
    """sort.hip's digit_bits() / sort_impl(): (digit width, passes)"""
    digit = 10 if (8 < bits <= 10) or (16 < bits <= 20) or (24 < bits <= 30) else 8
    return digit, -(-bits // digit)


def state(n, h, cells, seed):
    """Positions uniform in (0.02 h, box - 0.02 h) per axis -- beyond the wall planes, inside the grid, so cells 0 and
    D - 1 are occupied -- clipped below the box; velocities uniform in +-10 h."""
    rng = np.random.default_rng(seed)
    box = box_of(h, cells)
    pos = rng.uniform(0.02 * h, float(box) - 0.02 * h, (n, 3)).astype(F)
    pos = np.minimum(pos, np.nextafter(box, F(0)))
    vel = rng.uniform(-10 * h, 10 * h, (n, 3)).astype(F)
    assert_inside(pos, h, cells, f"state({n}, {h}, {cells})")
    return np.ascontiguousarray(pos), vel


# name -> D, h, n, key bits, (digit, passes), crowded (pressure on after step 1)
GRIDS = {
    "D1": dict(cells=1, h=0.1, n=40, bits=1, plan=(8, 1), crowded=False),
    "D2": dict(cells=2, h=0.1, n=700, bits=3, plan=(8, 1), crowded=True),
    "D3": dict(cells=3, h=0.1, n=2000, bits=5, plan=(8, 1), crowded=True),
    "D6": dict(cells=6, h=0.1, n=14000, bits=8, plan=(8, 1), crowded=True),
    "D7": dict(cells=7, h=0.1, n=2500, bits=9, plan=(10, 1), crowded=False),
    "D10h025": dict(cells=10, h=0.25, n=3000, bits=10, plan=(10, 1), crowded=False),
    "D11": dict(cells=11, h=0.1, n=3001, bits=11, plan=(8, 2), crowded=False),
    "D40": dict(cells=40, h=0.1, n=3001, bits=16, plan=(8, 2), crowded=False),
    "D41": dict(cells=41, h=0.1, n=3001, bits=17, plan=(10, 2), crowded=False),
    "D101": dict(cells=101, h=0.1, n=3001, bits=20, plan=(10, 2), crowded=False),
    "D102": dict(cells=102, h=0.1, n=3001, bits=21, plan=(8, 3), crowded=True),
    "D161h005": dict(cells=161, h=0.05, n=3001, bits=22, plan=(8, 3), crowded=False),
    "D256": dict(cells=256, h=0.1, n=3001, bits=24, plan=(8, 3), crowded=False),
    "D257": dict(cells=257, h=0.1, n=3001, bits=25, plan=(10, 3), crowded=False),
}
STEP_GRIDS = [k for k in GRIDS if k != "D1"]   # D = 1: every particle leaves the grid in its first step
# D102: CLUSTER_ROWS rows moved into a cube of +-CLUSTER_HALF CELLS about the middle of the box, so every row of the
# cluster sums all of it (rho ~ 2e4, pressure on; runs of hundreds of rows in eight cells).  In length units a +-0.3
# cube would hold 1000 rows in 0.216, rho ~ 93: far below the rest density, and the pressure term would not run.
CLUSTER_ROWS, CLUSTER_HALF = 1000, 0.3


def integer_keys(pos, h, cells):
    c = cells_of(pos, h)
    return (c[:, 0] + c[:, 1] * cells + c[:, 2] * cells * cells).astype(np.uint32)


def assert_oracle_keys_are_integer_keys(s, pos, what):
    """The D = 257 rule: the oracle flattens in fp32, exact while every key formed stays below 2^24 -- rows below
    z-layer 253 (253 * 257^2 + 257^2 - 1 < 2^24), with a layer to spare."""
    h, D = s.h, int(s.numCellsPerDim)
    top = int(cells_of(pos, h)[:, 2].max())
    assert top + 1 < 254, f"{what}: occupied z-layer {top}"
    assert np.array_equal(O.cell_keys(s, pos), integer_keys(pos, h, D)), f"{what}: fp32 keys differ from integer keys"
    return top


def grid_state(name, seed=1):
    """-> pos, vel, g (the GRIDS row).  D102: CLUSTER_ROWS rows moved into a small cube (pressure on).  D257: z scaled
    by 252/257, all rows below layer 253, the oracle's keys equal to the integer keys."""
    g = GRIDS[name]
    h, D, n = g["h"], g["cells"], g["n"]
    assert key_bits(D) == g["bits"] and plan_of(g["bits"]) == g["plan"], name
    pos, vel = state(n, h, D, seed)
    if name == "D102":
        rng = np.random.default_rng(seed + 100)
        mid = float(box_of(h, D)) / 2
        half = CLUSTER_HALF * h
        pos[:CLUSTER_ROWS] = (mid + rng.uniform(-half, half, (CLUSTER_ROWS, 3))).astype(F)
    if name == "D257":
        pos[:, 2] = (pos[:, 2] * F(252.0 / 257.0)).astype(F)
        assert_oracle_keys_are_integer_keys(settings_for(n, h, D), pos, name)
    assert_inside(pos, h, D, name)
    return np.ascontiguousarray(pos), vel, g


# ---- the click: reference threads t own z-layer (int)((float)t * h / h); some layers get none, some two ----

CLICK_GRIDS = {
    "h0.3": dict(h=0.3, cells=33, none=[15, 30], two=[14, 29], triples=[14]),
    "h0.07": dict(h=0.07, cells=143, none=[15, 30, 60, 63, 117, 120, 123, 126], two=[14, 29, 59, 62, 116, 119, 122, 125],
                  triples=[14, 62]),
}
PER_CELL = 70               # rows per footprint cell: more than one 64-lane trip
BACKGROUND, EDGE = 2000, 300
EDGE_CLICKS = ((400, 150), (200, 300))   # cy = D (the rows D-2, D-1 remain); cx = 0 (the columns 0..2 remain)


def owners(h, cells):
    """how many reference threads own each z-layer, in numpy fp32 (simulator.cu:329-340)"""
    t = np.arange(cells, dtype=np.int32).astype(F)
    z = t * F(h)
    layer = (z / F(h)).astype(np.int64)
    return np.bincount(layer[(layer >= 0) & (layer < cells)], minlength=cells)


def click_cell(h, cells, pixel=CLICK):
    """(cx, cy) of a click, as kernelMoveParticles computes it"""
    box = box_of(h, cells)
    x = F(F(pixel[0] - BOX_MIN_X) / F(BOX_MAX_X - BOX_MIN_X)) * box
    y = F(F(pixel[1] - BOX_MIN_Y) / F(BOX_MAX_Y - BOX_MIN_Y)) * box
    cx = int(x / F(h))
    cy = int(F(cells) - F(int(y / F(h))))
    return cx, cy


def click_state(name, seed=7):
    """-> pos, vel, info.  PER_CELL rows in each of the 25 footprint cells of the click at CLICK, on each layer of
    every triple (two owners, none, one), jittered inside the middle 60 % of the cell; BACKGROUND rows anywhere; EDGE
    rows under each of the two EDGE_CLICKS.  info: h, cells, cx, cy, and `rows`: {layer: {(dx, dy): row indices}}."""
    g = CLICK_GRIDS[name]
    h, D = g["h"], g["cells"]
    own = owners(h, D)
    assert np.flatnonzero(own == 0).tolist() == g["none"] and np.flatnonzero(own == 2).tolist() == g["two"], name
    assert own.max() == 2 and own.sum() == D
    rng = np.random.default_rng(seed)
    cx, cy = click_cell(h, D)
    assert 2 <= cx < D - 2 and 2 <= cy < D - 2
    hf = float(F(h))
    parts, rows, at = [], {}, 0
    for first in g["triples"]:
        assert (own[first], own[first + 1], own[first + 2]) == (2, 0, 1)
        for layer in (first, first + 1, first + 2):
            rows[layer] = {}
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cell = np.array([cx + dx, cy + dy, layer], np.float64)
                    parts.append((cell + rng.uniform(0.2, 0.8, (PER_CELL, 3))) * hf)
                    rows[layer][(dx, dy)] = np.arange(at, at + PER_CELL)
                    at += PER_CELL
    box = float(box_of(h, D))
    parts.append(rng.uniform(0.02 * h, box - 0.02 * h, (BACKGROUND, 3)))
    e = rng.uniform(0.02 * h, box - 0.02 * h, (EDGE, 3))       # under the click with cy = D
    e[:, 0] = rng.uniform((cx - 2) * hf, (cx + 3) * hf, EDGE)
    e[:, 1] = rng.uniform((D - 2.8) * hf, box - 0.02 * h, EDGE)
    parts.append(e)
    e = rng.uniform(0.02 * h, box - 0.02 * h, (EDGE, 3))       # under the click with cx = 0
    e[:, 0] = rng.uniform(0.02 * h, 2.9 * hf, EDGE)
    e[:, 1] = rng.uniform((cy - 2) * hf, (cy + 3) * hf, EDGE)
    parts.append(e)
    pos = np.minimum(np.concatenate(parts).astype(F), np.nextafter(box_of(h, D), F(0)))
    vel = rng.uniform(-1, 1, pos.shape).astype(F)
    c = assert_inside(pos, h, D, name)
    for layer, cellrows in rows.items():
        for (dx, dy), r in cellrows.items():
            assert (c[r] == (cx + dx, cy + dy, layer)).all(), "a footprint row left its cell"
    for (px, py), want in zip(EDGE_CLICKS, ((cx, D), (0, cy))):
        assert click_cell(h, D, (px, py)) == want
    return np.ascontiguousarray(pos), vel, dict(h=h, cells=D, cx=cx, cy=cy, rows=rows, owners=own)


def assert_click_applied(plain_vel, clicked_vel, info):
    """On the ORACLE's velocities with and without the click at CLICK (same step): rows of a two-owner layer took the
    impulse twice, rows of a layer without an owner not at all, rows of a one-owner layer once."""
    own = info["owners"]
    d = clicked_vel.astype(np.float64) - plain_vel.astype(np.float64)
    tol = 4 * np.spacing(np.maximum(np.abs(plain_vel), F(16))).astype(np.float64)
    seen = set()
    for layer, cellrows in info["rows"].items():
        k = int(own[layer])
        seen.add(k)
        for (dx, dy), r in cellrows.items():
            want = np.array([k * PUSH_STRENGTH / dx if dx else 0.0, k * PUSH_STRENGTH / dy if dy else 0.0,
                             -k * PUSH_STRENGTH if dx == 0 and dy == 0 else 0.0])
            if k == 0:
                assert np.array_equal(clicked_vel[r].view(np.uint32), plain_vel[r].view(np.uint32)), f"layer {layer}: no owner"
            else:
                assert (np.abs(d[r] - want) <= tol[r]).all(), f"layer {layer} ({k} owners), cell ({dx}, {dy})"
        centre = cellrows[(0, 0)]
        assert len(centre) > 64 and (np.abs(d[centre, 2] + k * PUSH_STRENGTH) <= tol[centre, 2]).all()
    assert seen == {0, 1, 2}


# ---- slabs: the thinnest legal ones, and a cut through the click's layers ----

SLABS = {
    "D8x4": dict(h=0.1, cells=8, n=3000, world=4, steps=6, clicks=(), cut_between=None, thin=True),
    "D7x3": dict(h=0.1, cells=7, n=2500, world=3, steps=6, clicks=(), cut_between=None, thin=False),
    "click33x4": dict(h=0.3, cells=33, n=None, world=4, steps=6, clicks=(2, 4), cut_between=(14, 16), thin=False),
}


def slab_state(name):
    sl = SLABS[name]
    if name == "click33x4":
        pos, vel, _ = click_state("h0.3")
    else:
        pos, vel = state(sl["n"], sl["h"], sl["cells"], 3)
    return pos, vel, sl


def partition_layers(hist, world, min_layers=2):
    """The driver's cuts, restated from its rule: slabs of about equal row counts on layer boundaries, each at
    least min_layers thick.  -> [0, c1, ..., D]"""
    D = len(hist)
    cum = np.concatenate([[0], np.cumsum(hist)]).astype(np.int64)
    total = int(cum[D])
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        z = min(int(np.searchsorted(cum, int(np.ceil(target)), side="left")), D)
        if z > 0 and abs(cum[z - 1] - target) <= abs(cum[z] - target):
            z -= 1
        z = max(z, cuts[-1] + min_layers)
        z = min(z, D - (world - r) * min_layers)
        cuts.append(z)
    return cuts + [D]
