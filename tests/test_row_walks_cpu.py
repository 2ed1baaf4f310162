"""The restatements of the passes that walk the nine runs around every row of the sorted stream -- derived fields,
neighbour lists, bodies, pair statistics -- on the states of tests/row_walk_cases.py (every grid of tests/walk_grid_cases.py with rows
on its walls, and D7 with one long run), without a GPU: the floors the states reach, the walk over the cell table
against all pairs, the derived fields against float64 under the bound tests/test_derived_cpu.py derives, what the
staged walk's restatement counts, the premise of the case whose rows lie outside the grid, and the premises of the pair
statistics' cases: tables with pairs in most bins, a slice that the counters tell from the derived fields', and a
restatement that stays cheap."""
import functools
import time

import numpy as np
import pytest

import bodies_restatement as BR
import derived_restatement as DR
import grid_states as G
import neighbour_restatement as NR
import pair_restatement as PR
import pair_states as PST
import row_walk_cases as R
from test_derived_cpu import hold_to_float64

F = np.float32
CASES = R.GRIDS + ["long run"]
DERIVE_SLICE, NBR_SLICE = 320, 640      # derived.hip's kDeriveSlice, neighbours.hip's kNbrSlice
PAIR_SLICE = PST.SLICE                  # pairs.hip's kPairSlice
RATIOS, COUNTED = {}, {}


@functools.lru_cache(maxsize=None)
def case(name):
    """the state the GPU cases upload and its grid built on the CPU: computed once, shared, never written to"""
    pos, vel, g = R.long_run_state() if name == "long run" else R.walls(name)
    h, D = g["h"], g["cells"]
    rows, ids, cells = NR.grid_of(pos, h, D)
    return dict(pos=pos, vel=vel, h=h, D=D, rows=rows, ids=ids, cells=cells, lengths=R.radii(h))


@pytest.mark.parametrize("name", R.GRIDS)
def test_the_states_reach_their_floors(name):
    got = R.reached(name)           # (row_state() has asserted them: here they are on record)
    print(f"{name}: {got}")
    assert got["entries"] >= 30000 and got["longest"] >= 100
    pos, _, g = R.row_state(name)
    if g["cells"] >= 4:
        assert got["bodies"] >= 50 and got["biggest"] >= 64 and got["one_body"] >= 600
        c = BR.row_cells(pos[R.cube_rows(name)], g["h"], g["cells"])
        corner = min(8, g["cells"] // 2)
        for a in range(3):          # the cube lies across a cell boundary: 7 | 8 (two blocks of eight cells) from D = 16 on
            assert set(c[:, a].tolist()) == {corner - 2, corner - 1, corner, corner + 1}, (name, a)
    # the walls' rows are not the cube's, and cells 0 and D - 1 are occupied
    wpos = R.walls(name)[0]
    changed = np.flatnonzero((wpos != pos).any(axis=1))
    assert len(changed) >= 10 and not set(changed.tolist()) & (set(R.cube_rows(name).tolist()) if g["cells"] >= 4 else set())
    c = BR.row_cells(wpos, g["h"], g["cells"])
    assert (c == 0).all(axis=1).any() and (c == g["cells"] - 1).all(axis=1).any()


def test_the_long_run_is_longer_than_every_slice():
    c = case("long run")
    cx, cy, cz = R.W.LONG_CELL
    run = c["cells"][(cz * c["D"] + cy) * c["D"] + cx]
    assert run[1] - run[0] >= R.W.LONG_ROWS > 1024 > NBR_SLICE > DERIVE_SLICE


@pytest.mark.parametrize("name", CASES)
def test_the_cell_walk_finds_what_all_pairs_finds(name):
    c = case(name)
    for radius in c["lengths"]:
        want = NR.all_pairs(c["pos"], c["h"], radius)
        got = NR.walk_order(c["rows"], c["ids"], c["cells"], c["h"], c["D"], radius)
        assert np.array_equal(got[0], want[0]), (name, radius)
        for i, (a, b) in enumerate(zip(NR.lists_of(*got), NR.lists_of(*want))):
            assert np.array_equal(np.sort(a), b), (name, radius, i)
        assert int(want[0][-1]) > 0


@pytest.mark.parametrize("name", CASES)
def test_the_bodies_are_the_components_of_all_pairs(name):
    c = case(name)
    n = len(c["pos"])
    for link in c["lengths"]:
        out = BR.bodies(c["rows"], c["ids"], c["cells"], c["h"], c["D"], link)
        k, comp, links = BR.all_pairs_components(c["pos"], c["h"], link)
        assert out["num_bodies"] == k and out["links"] == links, (name, link)
        first = np.full(k, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))
        labels = first[comp].astype(np.uint32)
        assert np.array_equal(out["labels"], labels), (name, link)
        table, largest = BR.table_of(c["pos"], labels)
        assert np.array_equal(out["table"], table) and out["largest"] == largest, (name, link)


@pytest.mark.parametrize("name", CASES)
def test_the_derived_fields_stay_within_their_bound_of_float64(name):
    c = case(name)
    dcoef = G.kernel_coeffs(c["h"])[1]
    grid = (c["rows"], c["vel"][c["ids"]], c["cells"])
    out = DR.derive(*grid, c["h"], dcoef, c["D"])
    RATIOS[name] = hold_to_float64(name, grid, c["h"], dcoef, c["D"], out)
    print(f"{name}: largest error / bound {RATIOS[name]:.4f}; so far, over all grids: {max(RATIOS.values()):.4f}")
    assert 0 < RATIOS[name] <= 1
    assert (out["vorticity"] != 0).any() and (out["divergence"] != 0).any() and int(out["neighbours"].max()) >= 100


def counted(name):
    if name not in COUNTED:
        c = case(name)
        COUNTED[name] = {s: R.staged_direct(c["rows"], c["cells"], c["h"], c["D"], s) for s in (PAIR_SLICE, DERIVE_SLICE, NBR_SLICE)}
    return COUNTED[name]


def test_what_the_staged_walk_counts():
    """(staged, direct) at the derived fields' slice and at the neighbour lists', on record for every state.  Every
    state stages runs; the long run walks runs from global memory at both slices, and so does at least one grid at the
    derived fields'."""
    for name in CASES:
        got = counted(name)
        print(f"{name}: slice {DERIVE_SLICE}: {got[DERIVE_SLICE]}, slice {NBR_SLICE}: {got[NBR_SLICE]}")
        for s in (DERIVE_SLICE, NBR_SLICE):
            staged, direct = got[s]
            assert staged > 0, (name, s)
            waves = -(-len(case(name)["pos"]) // 64)
            assert waves <= staged + direct <= 9 * waves, (name, s)
        assert got[NBR_SLICE][1] <= got[DERIVE_SLICE][1]
    assert counted("long run")[DERIVE_SLICE][1] > 0 and counted("long run")[NBR_SLICE][1] > 0
    direct = [name for name in R.GRIDS if counted(name)[DERIVE_SLICE][1] > 0]
    print(f"grids with direct runs at slice {DERIVE_SLICE}: {direct}")
    assert direct


def test_the_pair_walks_slice_shows_in_what_it_counts():
    """The pair statistics stage runs of up to 192 rows, the derived fields runs of up to 320: the counters
    tests/test_gpu_row_walks.py pins tell the two apart on D102's and on D40's walls state (a pair walk built with the
    derived fields' slice gives the same words and other counters); the long run has direct runs at 192 as well."""
    assert PAIR_SLICE == 192 < DERIVE_SLICE
    for name in CASES:
        got = counted(name)
        print(f"{name}: slice {PAIR_SLICE}: {got[PAIR_SLICE]}, slice {DERIVE_SLICE}: {got[DERIVE_SLICE]}")
        # (D1's one cell holds 256 rows: every run of it is longer than the pairs' slice)
        assert (got[PAIR_SLICE][0] > 0 or name == "D1") and sum(got[PAIR_SLICE]) == sum(got[DERIVE_SLICE]) and got[PAIR_SLICE][1] >= got[DERIVE_SLICE][1], name
    for name in ("D102", "D40"):
        assert counted(name)[PAIR_SLICE] != counted(name)[DERIVE_SLICE], name
    assert counted("long run")[PAIR_SLICE][1] > 0


@pytest.mark.parametrize("name", CASES)
def test_the_pair_tables_of_the_states(name):
    """What tests/test_gpu_row_walks.py asks of restatement (a) on one state -- the pairs at the three radii, found once
    each, and two tables of each -- costs under 5 s on one core (a cap against a runaway state, not a performance
    claim); at radius h the 32-bin table of every grid's walls state has pairs in at least half its bins, and its
    total is half the entries of the all-pairs lists; no term saturates."""
    c = case(name)
    t0 = time.perf_counter()
    tables = {}
    for radius in c["lengths"]:
        p = PR.prepared(c["pos"], c["vel"], c["h"], radius)
        tables[radius] = [p.table(PR.edges2(radius, c["h"], bins)) for bins in (0, 128)]
    seconds = time.perf_counter() - t0
    table = tables[0.0][0]
    total = int(table["pairs"].sum())
    print(f"{name}: {seconds:.2f} s; {total} pairs within h, {int((table['pairs'] > 0).sum())} of 32 bins hold some")
    assert seconds < 5.0, name
    assert 2 * total == int(NR.all_pairs(c["pos"], c["h"], 0.0)[0][-1]) > 0, name
    if name != "long run":
        assert (table["pairs"] > 0).sum() >= 16, name
    for radius in c["lengths"]:
        for t in tables[radius]:
            assert int(t["pairs"].sum()) == int(tables[radius][0]["pairs"].sum()) and not t["saturated"].any(), (name, radius)
    assert int(tables[c["lengths"][1]][0]["pairs"].sum()) <= total


def test_staged_direct_by_hand():
    """two cells of one row of a D = 4 grid: 70 rows in cell (1, 1, 1) and 5 in (2, 1, 1).  Wave 0 (64 rows of the first
    cell) and wave 1 (6 + 5 rows) both see the one run [0, 75) in the row (dy, dz) = (0, 0) and nothing elsewhere."""
    D, h = 4, 0.1
    pos = np.array([[0.15, 0.15, 0.15]] * 70 + [[0.25, 0.15, 0.15]] * 5, F)
    cells = np.zeros((D ** 3, 2), np.int32)
    cells[(1 * D + 1) * D + 1] = (0, 70)
    cells[(1 * D + 1) * D + 2] = (70, 75)
    assert R.staged_direct(pos, cells, h, D, 75) == (2, 0)
    assert R.staged_direct(pos, cells, h, D, 74) == (0, 2)
    # a third cell two to the right, (3, 1, 1): only the rows of cell 2 reach it, so wave 0's union stays [0, 75)
    pos = np.concatenate([pos, np.array([[0.35, 0.15, 0.15]] * 10, F)])
    cells[(1 * D + 1) * D + 3] = (75, 85)
    assert R.staged_direct(pos, cells, h, D, 75) == (1, 1)      # (wave 1: [0, 85))
    assert R.staged_direct(pos, cells, h, D, 85) == (2, 0)


def test_after_one_step_every_row_of_D1_lies_outside_the_grid():
    """the premise of the GPU case whose rows sweep_cell clamps into the edge cells, with the oracle; and there the
    restatements, which clamp alike, against all pairs, which knows no grid"""
    pos, vel, g = R.walls("D1")
    h, D = g["h"], g["cells"]
    ref = G.oracle_sim(G.settings_for(len(pos), h, D))
    ref.upload(pos, vel)
    ref.step()
    after = ref.download()
    ref.close()
    p = after["pos"]
    assert ((p < 0) | (p / F(h) >= D)).any(axis=1).all(), "premise: D1's step leaves no particle inside"
    finite = bool(np.isfinite(p).all() and np.isfinite(after["vel"]).all() and np.isfinite(after["rho"]).all())
    print(f"D1 after a step: every coordinate finite: {finite}; distinct positions: {len(np.unique(p, axis=0))}")
    assert finite, "the GPU case runs derive and the moments on this state"
    rows, ids, cells = NR.grid_of(p, h, D)
    assert cells.tolist() == [[0, len(p)]]
    for radius in R.radii(h):
        want = NR.all_pairs(p, h, radius)
        got = NR.walk_order(rows, ids, cells, h, D, radius)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])      # (one cell in id order: ascending)
        out = BR.bodies(rows, ids, cells, h, D, radius)
        k, _, links = BR.all_pairs_components(p, h, radius)
        assert (out["num_bodies"], out["links"]) == (k, links) and 2 * links == int(want[0][-1])
        # ... and the pair statistics: more than 10,000 pairs at every radius, the bodies' links
        pairs = PR.all_pairs(p, after["vel"], h, radius, 9)["pairs"]
        print(f"D1 after a step, radius {radius}: {int(pairs.sum())} pairs, by bin {pairs.tolist()}")
        assert int(pairs.sum()) == links > 10000
