"""The three analysis passes that walk the grid around points the CALLER chooses -- tracers (tracers.hip), the field
sample (sample.hip) and the surface (which samples its lattice with the same kernel) -- off the reference's 100^3 grid:
on one grid per sort plan of tests/grid_states.py (the tracers sort themselves with a key width of their own, one bit
wider than the grid's where D^3 is a power of two), on grids too small for a 3 x 3 x 3 neighbourhood or a full block of
eight cells, with h other than 0.1, over a run of 1,500 rows in one cell, after a click, and on fast-math handles.
Each against its numpy restatement fed by sph_download_grid + sph_download_state taken after the call, and the check
path against the default path.  Every comparison is of 32-bit words.  tests/test_walk_grids_cpu.py holds the
restatements to float64 on the same grids and proves what the sets and lattices (tests/tracer_sets.py,
tests/walk_grid_cases.py) reach."""
import os

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
import field_sample_restatement as FS
import grid_states as G
import tracer_restatement as TR
import tracer_sets as TS
import walk_grid_cases as W
from test_gpu_field_sample import assert_same_bits
from test_gpu_surface import assert_same_mesh
from test_gpu_surface import restate as restate_mesh
from test_gpu_tracers import assert_same_tracers

pytestmark = pytest.mark.gpu

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def sweeps_of(name):
    return ("list", "direct", "lds") if name in ("D7", "D102") else ("list", "direct")


def make(pos, vel, h, D, sweep, **kw):
    sim = sph.Simulator(G.settings_for(len(pos), h, D, factory=sph.default_settings), sweep=sweep, **kw)
    sim.upload_state(pos, vel)
    return sim


def sorted_state(sim):
    """what the restatements are fed with: the grid that was walked and the state, row by row of the sorted stream"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    return st["pos"][ids], st["vel"][ids], st["rho"][ids], g["cells"]


def restate_tracers(sim, grid, t, dt):
    s = sim.settings
    return TR.advect(grid[0], grid[1], grid[3], s.h, s.d_kernel_coeff, s.numCellsPerDim, t, dt)


def restate_field(sim, grid, field, lattice):
    s = sim.settings
    return FS.sample(grid[0], grid[1], grid[2], grid[3], s.h, s.d_kernel_coeff, s.numCellsPerDim, field, *lattice)


def advected(sim, t, dt, plain, monkeypatch):
    monkeypatch.setenv("SPH_TRACER_PLAIN", plain)
    sim.set_tracers(t)
    sim.advect_tracers(dt)
    return sim.tracers()


def check_tracers(sims, sets, what, monkeypatch, counted=True):
    """Every set, dt = timestep and dt = 0: the default path of sims[0] against the restatement (fed by the grid that
    call walked), its check path and both paths of the other handles (other sweeps, the same state) against those
    words; what the walk kernel counted against the groups of the tracers' cells.  -> hits, moved, the counters by set"""
    s = sims[0].settings
    h, D = s.h, int(s.numCellsPerDim)
    grid = None
    hits = moved = 0
    stats = {}
    for key, t in sets.items():
        want = None
        for dt in (s.timestep, 0.0):
            sims[0].tracer_stats(reset=True)
            got = advected(sims[0], t, dt, "0", monkeypatch)
            st = sims[0].tracer_stats(reset=True)
            if grid is None:
                grid = sorted_state(sims[0])
            if want is None:
                want = restate_tracers(sims[0], grid, t, dt)
                moved += int((bits(want["pos"]) != bits(t)).any(axis=1).sum())
                hits += int((want["den"] > 0).sum())
            else:
                want = {**want, "pos": t}             # (den and vel do not depend on dt; dt = 0 copies the words)
            assert_same_tracers(got, want, f"{what}, set {key}, dt = {dt}")
            if counted:
                groups = TS.wave_groups(t, h, D)
                assert st["calls"] == 1 and st["groups"] == sum(groups), (what, key, st, groups)
                assert st["waves_shared"] + st["waves_direct"] == len(groups) == -(-len(t) // 64), (what, key, st)
                assert st["waves_direct"] == sum(1 for n in groups if n > 4), (what, key, st, groups)
                stats[key] = st
            for k, sim in enumerate(sims):
                for plain in ("0", "1"):
                    if k or plain == "1":
                        assert_same_tracers(advected(sim, t, dt, plain, monkeypatch), got, f"{what}, set {key}, dt = {dt}: handle {k}, plain={plain}")
    return hits, moved, stats


# ---- tracers ----

@pytest.mark.parametrize("name", W.GRIDS)
def test_tracers_on_every_sort_plan(name, monkeypatch):
    """D2 and D256: the tracers' keys run to D^3 itself, a power of two -- one bit more than the grid's (on D256 another
    plan: 10 + 10 + 10 against 8 + 8 + 8).  With the grid's key_bits() instead, D256 fails here through the counters
    (the outside-interleaved set: 41 groups in two direct waves against [1, 1]); D2 cannot, one pass of 8-bit
    digits reads the key 8 whole whatever the width asked for.  D1 .. D7: one partial block of cells per row.  D40, D256: D a multiple of 8."""
    pos, vel, g = G.grid_state(name)
    h, D = g["h"], g["cells"]
    sims = [make(pos, vel, h, D, sweep) for sweep in sweeps_of(name)]
    sets = TS.grid_sets(pos, h, D)
    hits, moved, stats = check_tracers(sims, sets, name, monkeypatch)
    assert hits >= 100 and moved >= 100, f"{name}: the sets miss the fluid ({hits} hits, {moved} moved)"
    # the blob and the outside-interleaved set walk shared; the latter is two waves of one group each, which it is only
    # if the sort put every outside tracer behind every cell
    assert (stats["A"]["waves_shared"], stats["A"]["waves_direct"], stats["A"]["groups"]) == (4, 0, 4), stats["A"]
    assert TS.wave_groups(sets["F"], h, D) == [1, 1]
    assert (stats["F"]["waves_shared"], stats["F"]["waves_direct"], stats["F"]["groups"]) == (2, 0, 2), stats["F"]
    if name == "D1":
        # every tracer inside sums the one cell ...
        t = sets["A"]
        got = advected(sims[0], t, 0.0, "0", monkeypatch)
        cells = sims[0].download_grid()["cells"]
        assert cells.tolist() == [[0, len(pos)]] and (got["den"] > 0).all()
        # ... and after one step every particle has left the grid: the advect still answers
        for sim in sims:
            sim.simulate()
        after = sims[0].download_state()["pos"]
        assert ((after < 0) | (after / F(h) >= 1)).any(axis=1).all(), "premise: D1's step leaves no particle inside"
        few = {k: sets[k] for k in ("A", "C", "E", "F")}
        check_tracers(sims, few, name + " after a step", monkeypatch)
    for sim in sims:
        sim.close()


def test_tracers_and_sample_over_a_long_run(monkeypatch):
    """D7 with 1,500 rows in one cell: the row of three cells is one run of more than 1,100 stream rows, three chunks
    and more of kTracerChunk and of kSampleChunk with a partial last one (tests/test_walk_grids_cpu.py)."""
    pos, vel, g = W.long_run_state()
    h, D = g["h"], g["cells"]
    sims = [make(pos, vel, h, D, sweep) for sweep in ("list", "direct", "lds")]
    hits, moved, stats = check_tracers(sims, W.long_run_sets(h), "long run", monkeypatch)
    assert hits == 1200 and moved == 1200
    assert all((st["waves_direct"], st["groups"]) == (0, st["waves_shared"]) for st in stats.values()), stats
    cells = sims[0].download_grid()["cells"]
    cx, cy, cz = W.LONG_CELL
    run = cells[(cz * D + cy) * D + cx]
    assert run[1] - run[0] >= W.LONG_ROWS
    nonzero = check_fields(sims, {"long": W.long_run_lattice(h, D)}, ("density", "speed"), "long run", monkeypatch)
    assert nonzero["density"] > 500 and nonzero["speed"] > 500
    for sim in sims:
        sim.close()


# ---- the field sample ----

def check_fields(sims, lattices, fields, what, monkeypatch):
    """Every lattice and field: the tile path of sims[0] against the restatement, its plain path and both paths of the
    other handles against those words.  -> field -> non-zero points"""
    grid = None
    nonzero = dict.fromkeys(fields, 0)
    for key, lattice in lattices.items():
        for field in fields:
            monkeypatch.setenv("SPH_SAMPLE_PLAIN", "0")
            got = sims[0].sample_field(field, *lattice)
            if grid is None:
                grid = sorted_state(sims[0])
            assert_same_bits(got, restate_field(sims[0], grid, field, lattice), f"{what}, lattice {key}, {field}")
            nonzero[field] += int((got != 0).sum())
            for k, sim in enumerate(sims):
                for plain in ("0", "1"):
                    if k or plain == "1":
                        monkeypatch.setenv("SPH_SAMPLE_PLAIN", plain)
                        assert_same_bits(sim.sample_field(field, *lattice), got, f"{what}, lattice {key}, {field}: handle {k}, plain={plain}")
    return nonzero


@pytest.mark.parametrize("name", W.GRIDS)
def test_field_sample_with_several_bricks(name, monkeypatch):
    """130 x 3 x 3 lattices (two bricks and a two-lane tail) with rows outside the grid; on D256 and D257 the lattices
    whose lanes lie two and four cells apart, one wave's hull half the row of cells and the whole of it.  Density and
    speed of the uploaded state; after one step the pressure, on lattices around the state it left."""
    pos, vel, g = G.grid_state(name)
    h, D = g["h"], g["cells"]
    sims = [make(pos, vel, h, D, sweep) for sweep in sweeps_of(name)]
    nonzero = check_fields(sims, W.lattices(name, pos, h, D), ("density", "speed"), name, monkeypatch)
    assert nonzero["density"] >= 200 and nonzero["speed"] >= 200, (name, nonzero)
    if name in G.STEP_GRIDS:
        for sim in sims:
            sim.simulate()
        st = sims[0].download_state()
        assert (st["rho"] > 0).all()
        nonzero = check_fields(sims, W.lattices(name, st["pos"], h, D), ("pressure", "density"), name + " after a step", monkeypatch)
        if g["crowded"]:
            assert (st["prs"] > 0).any() and nonzero["pressure"] >= 200, (name, nonzero)
    for sim in sims:
        sim.close()


# ---- the surface ----

@pytest.mark.parametrize("name", ["D7", "D10h025"])
def test_surface_off_the_reference_grid(name, monkeypatch):
    """An 8^3 lattice over the box at half the sampled maximum: both paths against the surface's restatement fed with the field sample's RESTATEMENT of that lattice."""
    pos, vel, g = G.grid_state(name)
    h, D = g["h"], g["cells"]
    box = float(G.box_of(h, D))
    origin, spacing, shape = (0.0, 0.0, 0.0), box / 7, (8, 8, 8)
    for sweep in ("list", "direct"):
        sim = make(pos, vel, h, D, sweep)
        monkeypatch.setenv("SPH_SURFACE_PLAIN", "0")
        monkeypatch.setenv("SPH_SAMPLE_PLAIN", "0")
        sampled = sim.sample_field("density", origin, (spacing,) * 3, shape)
        field = restate_field(sim, sorted_state(sim), "density", (origin, (spacing,) * 3, shape))
        assert_same_bits(sampled, field, f"{name} {sweep}: the sampled lattice")
        iso = float(field.max()) / 2
        assert iso > 0
        want = restate_mesh(field, origin, spacing, iso)
        assert len(want["triangles"]) > 50 and len(want["vertices"]) > 50
        for plain in ("0", "1"):
            monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
            assert_same_mesh(sim.extract_surface(iso, origin, spacing, shape), want, f"{name} {sweep}, plain={plain}")
        sim.close()


# ---- after a click ----

def click_state():
    """4,096 rows under the click at grid_states.CLICK on the reference grid: x and y within four cells of the click's
    cell (its footprint is five cells square, every z-layer), z from 0.5 to 9.5"""
    rng = np.random.default_rng(31)
    cx, cy = G.click_cell(0.1, 100)
    lo = np.array([(cx - 3.5) * 0.1, (cy - 3.5) * 0.1, 0.5])
    pos = (lo + rng.random((4096, 3)) * np.array([0.8, 0.8, 9.0])).astype(F)
    vel = rng.uniform(-0.5, 0.5, pos.shape).astype(F)
    return pos, vel


@pytest.mark.parametrize("sweep", ["list", "direct"])
def test_an_advect_after_a_click_sees_the_clicked_velocities(sweep, monkeypatch):
    """Three steps, an advect (it builds the next step's grid ahead, and with the list sweep gathers the velocities into
    its interleaved records), a click (which drops that grid), the same seeds again and a second advect: it walks a
    grid rebuilt from the clicked velocities."""
    pos, vel = click_state()
    sim = make(pos, vel, 0.1, 100, sweep)
    for _ in range(3):
        sim.simulate()
    seeds = TS.scatter_in(sim.download_state()["pos"], 0.1, m=512)
    first = advected(sim, seeds, sim.settings.timestep, "0", monkeypatch)
    before = sim.download_state()["vel"]
    sim.moveParticles(G.CLICK)
    assert (bits(sim.download_state()["vel"]) != bits(before)).any(axis=1).sum() > 500, "premise: the click pushed rows"
    second = advected(sim, seeds, sim.settings.timestep, "0", monkeypatch)
    grid = sorted_state(sim)
    assert_same_tracers(second, restate_tracers(sim, grid, seeds, sim.settings.timestep), f"{sweep}: the advect after the click")
    changed = int((bits(second["vel"]) != bits(first["vel"])).any(axis=1).sum())
    assert changed > 10 and (second["den"] > 0).sum() > 400, f"{sweep}: {changed} tracers saw the click"
    assert np.array_equal(bits(second["den"]), bits(first["den"]))          # (the click moves no row)
    assert_same_tracers(advected(sim, seeds, sim.settings.timestep, "1", monkeypatch), second, f"{sweep}: the check path after the click")
    cx, cy = G.click_cell(0.1, 100)
    lattice = (((cx - 4) * 0.1, (cy - 1) * 0.1, 4.0), (0.1 / 13, 0.1, 0.1), (3, 3, 130))
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_SAMPLE_PLAIN", plain)
        got = sim.sample_field("speed", *lattice)
        assert_same_bits(got, restate_field(sim, grid, "speed", lattice), f"{sweep}: speed under the click, plain={plain}")
    assert (got > 0).sum() > 100
    sim.close()


# ---- fast-math handles ----

@pytest.mark.parametrize("sweep", ["list", "lds"])
def test_the_analysis_passes_do_not_depend_on_the_math_mode(sweep, monkeypatch):
    """SPH_MATH_FAST changes the step's sweeps and nothing else: tracers, field sample and surface of a fast handle
    equal their restatements (strict fp32, operation by operation) fed by that handle's own grid and state."""
    data = np.load(os.path.join(GOLD, "dense4096.npz"))
    pos, vel = np.ascontiguousarray(data["pos_1"], dtype=F), np.ascontiguousarray(data["vel_1"], dtype=F)
    sim = sph.Simulator(sph.default_settings(len(pos), True), sweep=sweep, math="fast")
    sim.upload_state(pos, vel)
    for _ in range(3):
        sim.simulate()
    st = sim.download_state()
    assert (st["prs"] > 0).any()
    h, D = sim.settings.h, int(sim.settings.numCellsPerDim)
    sets = {"A": TS.blob_in(TS.crowded_cell(st["pos"], h, D), h), "C": TS.scatter_in(st["pos"], h)}
    hits, moved, _ = check_tracers([sim], sets, f"fast {sweep}", monkeypatch)
    assert hits >= 300 and moved >= 300
    a = W.anchor(st["pos"], h, D)
    q = float(F(h) / F(4))
    lattices = {"fine": W.lattices("", st["pos"], h, D)["fine"], "cube": (tuple(v - 8 * q for v in a), (q, q, q), (17, 17, 17))}
    nonzero = check_fields([sim], lattices, FS.FIELDS, f"fast {sweep}", monkeypatch)
    assert min(nonzero.values()) >= 200, nonzero                        # (some sampled pressure is positive)
    origin, spacing, shape = lattices["cube"]
    field = restate_field(sim, sorted_state(sim), "density", lattices["cube"])
    iso = float(field.max()) / 2
    want = restate_mesh(field, origin, spacing, iso)
    assert len(want["triangles"]) > 50
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
        assert_same_mesh(sim.extract_surface(iso, origin, spacing, shape), want, f"fast {sweep}: surface, plain={plain}")
    sim.close()
