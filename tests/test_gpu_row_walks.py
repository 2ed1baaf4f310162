"""The six analysis passes that walk the nine runs around every ROW of the sorted stream -- derived fields
(derived.hip), neighbour lists (neighbours.hip), bodies (bodies.hip), the per-body moments and the body tracks that
label through the bodies, and the pair statistics (pairs.hip) -- off the reference's 100^3 grid: on one grid per sort
plan of tests/grid_states.py, on grids too small for a 3 x 3 x 3 neighbourhood or a full block of eight cells, with h
other than 0.1, with rows on the wall planes, across a step, over a run of 1,500 rows in one cell, with every row
outside the grid, after a click, and on fast-math handles.  Each against its restatement fed by sph_download_grid +
sph_download_state taken after the call (the pair statistics: by the state alone, every pair tested), through the
helpers of the passes' own test files, the check path against the default path, and what walk_runs_staged counted
against its restatement (tests/row_walk_cases.py) at each walk's own slice: 320, 640 and the pairs' 192.  Every
comparison is of 32-bit words.  tests/test_row_walks_cpu.py holds the restatements to all pairs and to float64 on the
same states, and the premises the pair statistics' cases rest on.  Measured on an MI355X: the 29 cases take 34 to 47 s
(three runs), the costliest -- the long run -- 4.4 s, D256, D257 and D102 3.5 to 3.7 s, every other under 2.2 s."""
import numpy as np
import pytest

import body_moments_restatement as M
import body_states as BS
import grid_states as G
import pair_restatement as PR
import pair_states as PST
import row_walk_cases as R
import test_gpu_bodies as TB
import test_gpu_body_moments as TM
import test_gpu_body_tracks as TT
import test_gpu_derived as TD
import test_gpu_neighbours as TN
import test_gpu_pairs as TP
from test_gpu_walk_grids import click_state, make, sweeps_of

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ("SPH_DERIVE_PLAIN", "SPH_NEIGHBOURS_PLAIN", "SPH_BODIES_PLAIN", "SPH_PAIRS_PLAIN")
PAIR_BINS = (128, 1, 9)     # the pair tables' bins, by the position of a length among the lengths of a case


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def set_plain(monkeypatch, value):
    for env in PLAIN:
        monkeypatch.setenv(env, value)


def counted(sim, slice):
    """staged_direct over the grid the handle holds (call after a pass)"""
    g = sim.download_grid()
    rows = sim.download_state()["pos"][g["ids"].astype(np.int64)]
    return R.staged_direct(rows, g["cells"], sim.settings.h, int(sim.settings.numCellsPerDim), slice)


def all_passes(sim, monkeypatch, what, lengths, measure):
    """derive, neighbour_lists (both orders), label_bodies and pair_statistics at every length, measure_bodies at
    `measure`: each on both paths against its restatement, the runs the walks counted against staged_direct, and the
    pins between the passes on the device -> the default path's results, and dict(derive, neighbours, pairs) of the
    walks' counters"""
    out = {}
    out["derive"], dst = TD.both_paths(sim, monkeypatch, what)
    runs = dict(derive=(dst["runs_staged"], dst["runs_direct"]))
    assert runs["derive"] == counted(sim, TD.SLICE), (what, dst)
    want, want_pairs = counted(sim, TN.SLICE), counted(sim, PST.SLICE)
    for r in lengths:
        out["lists", r], nst = TN.both_paths(sim, monkeypatch, what, r)
        # two calls, a count and an emit walk in each
        assert (nst["runs_staged"], nst["runs_direct"]) == (4 * want[0], 4 * want[1]), (what, r, nst, want)
        runs["neighbours"] = (nst["runs_staged"], nst["runs_direct"])
        runs["longest", r] = nst["longest"]
        out["bodies", r], _, _ = TB.both_paths(sim, monkeypatch, f"{what}, link {r}", r)
        sim.body_stats(reset=True)
        sim.label_bodies(r)
        st = sim.body_stats(reset=True)
        runs["unions", r] = st["unions"]
        assert len(out["lists", r]["neighbours"]) == int(out["lists", r]["offsets"][-1]) == 2 * st["links"], (what, r, st)
        # the sixth walk: restatement (a) word for word on both paths (test_gpu_pairs.both_paths), its own slice, and
        # the same pairs as the bodies' links and half the lists' entries
        out["pairs", r], pst = TP.both_paths(sim, monkeypatch, what, PAIR_BINS[lengths.index(r) % 3], r)
        runs["pairs"] = (pst["runs_staged"], pst["runs_direct"])
        assert runs["pairs"] == want_pairs, (what, r, pst, want_pairs)
        pairs = int(out["pairs", r]["pairs"].sum())
        assert pairs == st["links"] and 2 * pairs == len(out["lists", r]["neighbours"]), (what, r, pairs, st)
    assert lengths[0] == 0.0
    lists = out["lists", 0.0]
    assert np.array_equal(np.diff(lists["offsets"].astype(np.int64)) + 1, out["derive"]["neighbours"].astype(np.int64)), what
    out["moments"], _ = TM.both_paths(sim, monkeypatch, f"{what}, moments at link {measure}", measure)
    return out, runs


def assert_same_passes(sim, first, monkeypatch, what, lengths, measure):
    """the default path of every pass of another handle of the same state: the first handle's words; the walk-order
    lists: the restatement over this handle's own grid"""
    set_plain(monkeypatch, "0")
    TD.assert_same_fields(sim.derive(), first["derive"], what)
    for r in lengths:
        TN.assert_same_lists(sim.neighbour_lists(r), first["lists", r], f"{what}, radius {r}")
        TN.assert_same_lists(sim.neighbour_lists(r, walk_order=True), TN.walk_of(sim, r), f"{what}, radius {r}, walk order")
        TB.assert_same_bodies(sim.label_bodies(r), first["bodies", r], f"{what}, link {r}")
        got = sim.pair_statistics(PAIR_BINS[lengths.index(r) % 3], r)
        PR.assert_same_table(got, first["pairs", r], f"{what}, pairs within {r}")
        assert got["rows"].tobytes() == first["pairs", r]["rows"].tobytes() and np.array_equal(words(got["edges2"]), words(first["pairs", r]["edges2"])), (what, r)
    assert sim.body_stats()["gave_up"] == 0
    got = sim.measure_bodies(measure)
    TM.assert_same_bodies(got, first["moments"], f"{what}, moments")
    M.assert_same_rows(got["moments"], first["moments"]["moments"], f"{what}, moments")
    assert np.array_equal(got["size_hist"], first["moments"]["size_hist"]), what


def tracked(pair, what, link):
    """one call of the pair (default and check path against the tracker), the labels it tracked being the bodies'
    restatement's over the grid the call walked"""
    got, want = pair.call(what, link)
    restated = TB.restate(pair.sims[0], link)
    assert np.array_equal(got["labels"], restated["labels"]) and np.array_equal(got["table"], restated["table"]), what
    return got, want


# ---- every grid ----

@pytest.mark.parametrize("name", R.GRIDS)
def test_the_row_passes_on_every_grid(name, monkeypatch):
    """D1 .. D7: one partial block of cells per row, D1 and D2 without a 3 x 3 x 3 neighbourhood; D10h025 and D161h005:
    h2, the link length "0 means h" and dcoef at h = 0.25 and 0.05; D40 and D256: D a multiple of 8; D256 / D257: their
    sort plans, and tables of 16.8 million cells.  Rows on the wall planes everywhere: cells 0 and D - 1 are walked."""
    pos, vel, g = R.walls(name)
    h, D = g["h"], g["cells"]
    lengths, measure = R.radii(h), 0.3 * float(h)
    sims = [make(pos, vel, h, D, sweep) for sweep in sweeps_of(name)]
    first, runs = all_passes(sims[0], monkeypatch, name, lengths, measure)
    assert runs["derive"][0] > 0 and runs["neighbours"][0] > 0 and (runs["pairs"][0] > 0 or name == "D1")   # (D1: 256 rows in the one cell)
    assert len(first["lists", 0.0]["neighbours"]) >= R.MIN_ENTRIES
    assert len(first["pairs", 0.0]["pairs"]) == 128 and len(first["pairs", lengths[1]]["pairs"]) == 1
    if D >= 4:
        assert first["bodies", lengths[2]]["num_bodies"] >= R.MIN_BODIES
    for sim, sweep in zip(sims[1:], sweeps_of(name)[1:]):
        assert_same_passes(sim, first, monkeypatch, f"{name}, sweep {sweep}", lengths, measure)
    for sim in sims:
        sim.close()


# ---- across a step ----

@pytest.mark.parametrize("name", [k for k in R.GRIDS if k in G.STEP_GRIDS])
def test_tracks_and_the_next_steps_density_across_a_step(name, monkeypatch):
    """Two labellings at link 0.3 h with one step between them, tracked on both paths against the tracks' restatement
    driven by the bodies' restated labels; and DESIGN.md section 10f's pin, on every sweep: rho of derive() is, word
    for word, the density the next step's sweep stores (where it is above EPS_F)."""
    pos, vel, g = R.walls(name)
    h, D = g["h"], g["cells"]
    link = 0.3 * float(h)
    for sweep in ("list", "direct"):
        pair = TT.Pair(pos, vel, h, D, monkeypatch=monkeypatch, sweep=sweep)
        pair.reset()
        first, _ = tracked(pair, f"{name}, sweep {sweep}, first call", link)
        assert first["summary"]["born"] == first["num_bodies"] and first["summary"]["edges"] == 0
        if sweep == "list":
            # one handle of the two walks the labelling's grid once more, for the pairs; the step leaves both the same
            assert pair.sims[0].pair_statistics(7, link)["pairs"].sum() > 0
        pair.simulate(1)
        mine, other = (s.download_state() for s in pair.sims)
        for k in other:
            assert np.array_equal(words(mine[k]), words(other[k])), f"{name}, sweep {sweep}: {k} after the step differs between the two handles"
        second, _ = tracked(pair, f"{name}, sweep {sweep}, after a step", link)
        s = second["summary"]
        assert s["edges"] >= 1 and s["born"] + s["continued"] == s["bodies"] == second["num_bodies"], (name, sweep, s)
        assert s["previous_bodies"] == first["num_bodies"] and s["sequence"] == 2
        pair.close()
    set_plain(monkeypatch, "0")
    for sweep in sweeps_of(name):
        sim = make(pos, vel, h, D, sweep)
        rho = sim.derive()["rho"]
        sim.simulate()
        after = sim.download_state()["rho"]
        above = rho > TD.EPS_F
        bad = above & (words(rho) != words(after))
        print(f"{name}, sweep {sweep}: rho of {int(above.sum())} of {len(rho)} rows above EPS_F, {int(bad.sum())} differ from the next step's")
        assert above.sum() > len(rho) // 2
        assert not bad.any(), f"{name}, sweep {sweep}: rho of {int(bad.sum())} rows differs from the next step's density, first row {np.flatnonzero(bad)[:1]}"
        sim.close()
    # the grid the pair statistics build ahead, as the first walker after the upload, is the one the next step uses: the
    # state after that step is a bare handle's, and the pairs of that state are again the restatement's
    bare = make(pos, vel, h, D, "list")
    bare.simulate()
    want = bare.download_state()
    bare.close()
    sim = make(pos, vel, h, D, "list")
    before, _ = TP.both_paths(sim, monkeypatch, f"{name}, the first walker before the step", 7, 0.5 * float(h))
    assert before["pairs"].sum() > 0
    sim.simulate()
    got = sim.download_state()
    for k in want:
        assert np.array_equal(words(got[k]), words(want[k])), f"{name}: {k} after a step whose grid the pair statistics built differs from a bare handle's"
    TP.both_paths(sim, monkeypatch, f"{name}, pairs after the step", 128, 0.5 * float(h))
    sim.close()


# ---- one long run ----

def test_the_row_passes_over_a_long_run(monkeypatch):
    """D7 with 1,500 rows in one cell: every wave of them walks runs longer than either slice from global memory, their
    lists are longer than the sort's slice (the chunked odd-even sort, on a grid other than 100^3), the cell is one
    body whose every merge lands on one root."""
    pos, vel, g = R.long_run_state()
    h, D = g["h"], g["cells"]
    lengths = R.radii(h)[:2]
    sims = [make(pos, vel, h, D, sweep) for sweep in ("list", "direct", "lds")]
    first, runs = all_passes(sims[0], monkeypatch, "long run", lengths, lengths[1])
    assert runs["derive"][1] > 0 and runs["neighbours"][1] > 0 and runs["pairs"][1] > 0
    assert runs["longest", 0.0] >= R.W.LONG_ROWS - 1 > TN.SORT_SLICE
    assert runs["unions", 0.0] >= R.W.LONG_ROWS - 1
    row = first["bodies", 0.0]["labels"][:R.W.LONG_ROWS]
    assert (row == row[0]).all(), "the long run's cell is not one body"
    for sim, sweep in zip(sims[1:], ("direct", "lds")):
        assert_same_passes(sim, first, monkeypatch, f"long run, sweep {sweep}", lengths, lengths[1])
    for sim in sims:
        sim.close()
    pair = TT.Pair(pos, vel, h, D, monkeypatch=monkeypatch)
    pair.reset()
    tracked(pair, "long run, first call", lengths[1])
    again, _ = tracked(pair, "long run, at link h", 0.0)
    assert again["summary"]["edges"] >= 1 and again["summary"]["born"] == 0
    pair.close()


# ---- rows outside the grid ----

def test_rows_outside_the_grid_are_walked_from_the_edge_cells(monkeypatch):
    """D1 after one step: the walls have put every row at a coordinate of h or beyond, outside the one cell.  sweep_cell
    clamps such a row into the edge cell, whose runs it walks, and so do the restatements; all pairs knows no grid and
    finds the same lists.  (tests/test_row_walks_cpu.py: every coordinate of that state is finite.)"""
    pos, vel, g = R.walls("D1")
    h, D = g["h"], g["cells"]
    for sweep in sweeps_of("D1"):
        sim = make(pos, vel, h, D, sweep)
        sim.simulate()
        st = sim.download_state()
        p = st["pos"]
        assert ((p < 0) | (p / F(h) >= D)).any(axis=1).all(), "premise: D1's step leaves no particle inside"
        assert np.isfinite(p).all() and np.isfinite(st["vel"]).all() and np.isfinite(st["rho"]).all()
        out, runs = all_passes(sim, monkeypatch, f"D1 after a step, sweep {sweep}", R.radii(h), 0.3 * float(h))
        assert sim.download_grid()["cells"].tolist() == [[0, len(pos)]]
        assert len(out["lists", 0.0]["neighbours"]) > len(pos) and runs["derive"][0] + runs["derive"][1] == -(-len(pos) // 64)
        # (tests/test_row_walks_cpu.py: more than 10,000 pairs at every one of the radii)
        for r in R.radii(h):
            assert out["pairs", r]["pairs"].sum() > 10000, (sweep, r)
        assert runs["pairs"][0] + runs["pairs"][1] == -(-len(pos) // 64)
        sim.close()


# ---- after a click ----

@pytest.mark.parametrize("sweep", ["list", "direct"])
def test_a_derive_after_a_click_sees_the_clicked_velocities(sweep, monkeypatch):
    """Three steps, the four passes (the first builds the next step's grid ahead, and with the list sweep gathers the
    velocities into its interleaved records), a click (which drops that grid), the four passes again: derive and the
    pair statistics walk a grid rebuilt from the clicked velocities; what depends on the positions alone does not
    change."""
    pos, vel = click_state()
    sim = make(pos, vel, 0.1, 100, sweep)
    for _ in range(3):
        sim.simulate()
    set_plain(monkeypatch, "0")
    first = (sim.derive(), sim.neighbour_lists(), sim.label_bodies())
    # the pairs within h in 16 bins, on both paths against the restatement over the downloaded state
    pairs = [TP.both_paths(sim, monkeypatch, f"{sweep}: the pairs before the click", 16, key=("click", sweep, 0))[0]]
    before = sim.download_state()["vel"]
    sim.moveParticles(G.CLICK)
    assert (words(sim.download_state()["vel"]) != words(before)).any(axis=1).sum() > 500, "premise: the click pushed rows"
    second = (sim.derive(), sim.neighbour_lists(), sim.label_bodies())
    pairs.append(TP.both_paths(sim, monkeypatch, f"{sweep}: the pairs after the click", 16, key=("click", sweep, 1))[0])
    # the click moves no row: the same pairs in the same bins, the same sums of d2; the sums over the velocities are the
    # clicked ones (premise, from the restatements of the two states: some differ)
    restated = [TP.want_of(sim, 16, 0.0, key=("click", sweep, k)) for k in (0, 1)]
    assert restated[0]["pairs"].sum() > 0 and any(int(restated[0]["sums"][b, s]) != int(restated[1]["sums"][b, s]) for b in range(16) for s in (1, 2, 3)), \
        "premise: the click changes a sum of w2, a or l2"
    assert np.array_equal(pairs[1]["pairs"], pairs[0]["pairs"]) and np.array_equal(pairs[1]["words"][:, 0], pairs[0]["words"][:, 0]), sweep
    assert (pairs[1]["words"][:, 1:] != pairs[0]["words"][:, 1:]).any(), f"{sweep}: no sum over the velocities saw the click"
    TD.assert_same_fields(second[0], TD.restate(sim), f"{sweep}: the derive after the click")
    changed = (words(second[0]["vorticity"]) != words(first[0]["vorticity"])).any(axis=1) | (words(second[0]["divergence"]) != words(first[0]["divergence"]))
    assert changed.sum() > 10, f"{sweep}: {int(changed.sum())} rows saw the click"
    for k in ("rho", "grad_rho", "neighbours"):                                # (the click moves no row)
        assert np.array_equal(words(second[0][k]), words(first[0][k])), (sweep, k)
    assert int(second[0]["neighbours"].max()) > 1
    TN.assert_same_lists(second[1], first[1], f"{sweep}: the lists after the click")
    TB.assert_same_bodies(second[2], first[2], f"{sweep}: the bodies after the click")
    set_plain(monkeypatch, "1")
    TD.assert_same_fields(sim.derive(), second[0], f"{sweep}: the check path after the click")
    TN.assert_same_lists(sim.neighbour_lists(), second[1], f"{sweep}: the check path after the click")
    TB.assert_same_bodies(sim.label_bodies(), second[2], f"{sweep}: the check path after the click")
    set_plain(monkeypatch, "0")
    sim.close()


# ---- fast-math handles ----

@pytest.mark.parametrize("sweep", ["list", "lds"])
def test_the_row_passes_do_not_depend_on_the_math_mode(sweep, monkeypatch):
    """SPH_MATH_FAST changes the step's sweeps and nothing else: all six passes of a fast handle equal their
    restatements (strict fp32, operation by operation) fed by that handle's own grid and state, on both paths."""
    pos, vel = TD.golden("dense4096")
    pair = TT.Pair(pos, vel, monkeypatch=monkeypatch, sweep=sweep, math="fast")
    pair.simulate(3)
    sim = pair.sims[0]
    assert (sim.download_state()["prs"] > 0).any()
    lengths = R.radii(sim.settings.h)
    out, runs = all_passes(sim, monkeypatch, f"fast {sweep}", lengths, lengths[2])
    assert runs["derive"][0] > 0 and (out["derive"]["vorticity"] != 0).any()
    # (at 0.3 h this state is one body: the tracks at the link tests/body_states.py gives it, several bodies)
    link = [l for s, l in BS.BIG if s == "dense4096"][-1]
    pair.reset()
    tracked(pair, f"fast {sweep}, first call", link)
    pair.simulate(1)
    got, _ = tracked(pair, f"fast {sweep}, after a step", link)
    assert got["summary"]["edges"] >= 1 and got["num_bodies"] > 1
    pair.close()
