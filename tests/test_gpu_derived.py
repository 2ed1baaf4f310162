"""The derived per-particle fields on the GPU (sph_derive): both paths against the numpy
restatement (tests/derived_restatement.py) fed by sph_download_grid + sph_download_state, against the density and the
hit count the next step produces, what the kernel counted, and the call's absence from the run's results.  Every
comparison is of 32-bit words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import derived_restatement as DR
import grid_states as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SPH_ESTATE = -4
EPS_F = F(1e-4)
SLICE = 320          # derived.hip's kDeriveSlice: the longest run the default path stages
KEYS = ("vorticity", "divergence", "grad_rho", "rho", "neighbours")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_fields(got, want, what):
    for k in KEYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = words(a) != words(b)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} words of {k} differ, first at {np.argwhere(bad)[0]}: " \
                              f"{a[tuple(np.argwhere(bad)[0])]!r} vs {b[tuple(np.argwhere(bad)[0])]!r}"


def golden(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    return np.ascontiguousarray(data["pos_1"], dtype=F), np.ascontiguousarray(data["vel_1"], dtype=F)


def simulator(pos, vel, h=0.1, cells=100, **kw):
    s = sph.default_settings(len(pos), True) if (h, cells) == (0.1, 100) else G.settings_for(len(pos), h, cells, factory=sph.default_settings)
    sim = sph.Simulator(s, **kw)
    sim.upload_state(pos, vel)
    return sim


def restate(sim):
    """the restatement over the grid the sweep walked (call after derive()), its rows put back in particle-id order"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    s = sim.settings
    rows = DR.derive(st["pos"][ids], st["vel"][ids], g["cells"], s.h, s.d_kernel_coeff, int(s.numCellsPerDim))
    out = {}
    for k in KEYS:
        out[k] = np.empty_like(rows[k])
        out[k][ids] = rows[k]
    return out


def both_paths(sim, monkeypatch, what):
    """derive() on the default and on the check path, both equal to the restatement -> (fields, the default path's stats)"""
    monkeypatch.setenv("SPH_DERIVE_PLAIN", "0")
    sim.derive_stats(reset=True)
    got = sim.derive()
    st = sim.derive_stats(reset=True)
    want = restate(sim)
    assert_same_fields(got, want, what + ", default path")
    monkeypatch.setenv("SPH_DERIVE_PLAIN", "1")
    assert_same_fields(sim.derive(), want, what + ", check path")
    plain = sim.derive_stats(reset=True)
    assert (plain["calls"], plain["runs_staged"], plain["runs_direct"]) == (1, 0, 0), plain
    monkeypatch.setenv("SPH_DERIVE_PLAIN", "0")
    assert st["calls"] == 1 and 0.0 < st["seconds"] < 1.0, st
    return got, st


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("random4096", 0), ("dense4096", 5)])
def test_all_five_outputs_are_the_restatement_on_both_paths(name, steps, monkeypatch):
    pos, vel = golden(name)
    sim = simulator(pos, vel)
    for _ in range(steps):
        sim.simulate()
    got, st = both_paths(sim, monkeypatch, f"{name} + {steps} steps")
    assert st["runs_staged"] > 0
    assert (got["neighbours"] >= 1).all() and int(got["neighbours"].sum()) > len(pos)
    if name == "dense4096":
        assert (got["vorticity"] != 0).any() and (got["divergence"] != 0).any()
    else:   # one velocity for every particle: a uniform translation
        assert (words(got["vorticity"]) == 0).all() and (words(got["divergence"]) == 0).all()
    sim.close()
    # the sweeps that keep separate sorted position and velocity streams read the same words
    for sweep in ("lds", "direct"):
        other = simulator(pos, vel, sweep=sweep)
        for _ in range(steps):
            other.simulate()
        assert_same_fields(other.derive(), got, f"{name} + {steps} steps, sweep {sweep}")
        other.close()


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("dense4096", 3), ("random4096", 0)])
def test_rho_and_neighbours_are_what_the_next_step_computes(name, steps):
    pos, vel = golden(name)
    sim = simulator(pos, vel, flags=_lib.SPH_FLAG_COUNT_PAIRS)
    assert sim.settings.h == F(0.1)
    for _ in range(steps):
        sim.simulate()
    got = sim.derive()
    sim.kernel_times(reset=True)
    sim.simulate()
    rho = sim.download_state()["rho"]
    assert (got["rho"] > EPS_F).all()
    assert np.array_equal(words(got["rho"]), words(rho)), "rho differs from the next step's density sweep"
    dbg = sim.debug_counters()
    assert int(got["neighbours"].sum()) == int(dbg[15]) > len(pos), (int(got["neighbours"].sum()), dbg[15])
    sim.close()


def run(timed, deriving, steps=10):
    pos, vel = golden("dense4096")
    sim = simulator(pos, vel)
    times = sph.Times()
    fields = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if deriving:
            fields.append(sim.derive())
    st = sim.download_state()
    st["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return st, fields


@pytest.mark.parametrize("timed", [False, True])
def test_a_derive_between_every_two_steps_leaves_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_DERIVE_PLAIN", "0")
    with_, fields = run(timed, True)
    without, _ = run(timed, False)
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(words(with_[k]), words(without[k])), f"timed={timed}: {k} differs after 10 steps"
    assert len(fields) == 10 and not np.array_equal(words(fields[0]["rho"]), words(fields[-1]["rho"]))


# ---- the smallest shapes that can go wrong ----

def cluster(n, seed, lo=(0.5, 0.5, 0.5), side=0.25):
    """n particles in a cube of `side` at `lo` (a few cells), velocities of order one"""
    rng = np.random.default_rng(seed)
    pos = (np.asarray(lo) + rng.uniform(0, side, (n, 3))).astype(F)
    vel = rng.uniform(-1, 1, (n, 3)).astype(F)
    return pos, vel


def one_cell(n, seed, cell):
    """n particles inside one cell of the 100^3 grid, away from its faces"""
    rng = np.random.default_rng(seed)
    pos = ((np.asarray(cell) + rng.uniform(0.1, 0.9, (n, 3))) * 0.1).astype(F)
    assert (DR.row_cells(pos, 0.1, 100) == np.asarray(cell)).all()
    return pos, rng.uniform(-1, 1, (n, 3)).astype(F)


def on_the_walls(name):
    """a grid_states state with rows moved onto the wall planes: coordinates 0 and the largest float below the box"""
    pos, vel, g = G.grid_state(name)
    top = np.nextafter(G.box_of(g["h"], g["cells"]), F(0))
    k = min(len(pos) // 4, 24)
    for i in range(k):
        pos[i, i % 3] = F(0) if (i // 3) % 2 == 0 else top
    pos[k] = (F(0), F(0), F(0))
    pos[k + 1] = (top, top, top)
    G.assert_inside(pos, g["h"], g["cells"], name)
    return pos, vel, g


def test_one_particle(monkeypatch):
    pos, vel = np.array([[5.05, 5.05, 5.05]], F), np.array([[1, -2, 3]], F)
    sim = simulator(pos, vel)
    got, st = both_paths(sim, monkeypatch, "n = 1")
    s = sim.settings
    h2 = F(s.h) * F(s.h)
    self_term = F(0) + F(0.02) * (((F(s.d_kernel_coeff) * h2) * h2) * h2)
    assert words(got["rho"]).item() == words(self_term).item() and got["neighbours"].tolist() == [1]
    for k in ("vorticity", "divergence", "grad_rho"):
        assert (words(got[k]) == 0).all(), k
    assert (st["runs_staged"], st["runs_direct"]) == (1, 0)
    sim.close()


def test_wave_tails_grids_of_a_few_cells_and_runs_about_the_slice(monkeypatch):
    staged = direct = 0
    for n in (63, 64, 65, 129):
        sim = simulator(*cluster(n, n))
        got, st = both_paths(sim, monkeypatch, f"n = {n}")
        assert got["neighbours"].max() > 1
        staged, direct = staged + st["runs_staged"], direct + st["runs_direct"]
        sim.close()
    for name in ("D1", "D2", "D3"):
        pos, vel, g = on_the_walls(name)
        sim = simulator(pos, vel, g["h"], g["cells"])
        got, st = both_paths(sim, monkeypatch, name)
        staged, direct = staged + st["runs_staged"], direct + st["runs_direct"]
        sim.close()
    # about 1,500 rows in one cell: every wave's only run is longer than any slice
    sim = simulator(*one_cell(1500, 5, (50, 50, 50)))
    got, st = both_paths(sim, monkeypatch, "1500 in one cell")
    assert (got["neighbours"] > 100).all()
    assert (st["runs_staged"], st["runs_direct"]) == (0, -(-1500 // 64)), st
    staged, direct = staged + st["runs_staged"], direct + st["runs_direct"]
    sim.close()
    # a run of exactly the slice (rows 0 .. SLICE - 1: whole waves) is staged, a run of one more is not
    a, b = one_cell(SLICE, 6, (20, 20, 20)), one_cell(SLICE + 1, 7, (60, 60, 60))
    sim = simulator(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
    got, st = both_paths(sim, monkeypatch, "runs of SLICE and SLICE + 1")
    assert (st["runs_staged"], st["runs_direct"]) == (SLICE // 64, -(-(SLICE + 1) // 64)), st
    staged, direct = staged + st["runs_staged"], direct + st["runs_direct"]
    sim.close()
    assert staged > 0 and direct > 0


def test_state_rules_error_codes_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_DERIVE_PLAIN", "0")
    pos, vel = golden("dense4096")
    sim = sph.Simulator(sph.default_settings(len(pos), True))
    L, h = sim._L, sim._h
    outs = (C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.c_int(-1))
    host = lambda: L.sph_derived_host(h, C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]))
    # before any state, and the results before the first derive
    assert L.sph_derive(h) == SPH_ESTATE
    assert host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    assert host() == SPH_ESTATE
    first = sim.derive()
    assert host() == 0 and outs[3].value == len(pos)
    assert L.sph_derived_host(h, None, None, None, None) == 0
    # a derive, an upload, a derive again: the new state's fields
    moved = pos[::-1].copy()
    sim.upload_state(moved, vel)
    second = sim.derive()
    assert_same_fields(second, restate(sim), "after a second upload")
    assert not np.array_equal(words(second["rho"]), words(first["rho"]))
    # the stats sum over calls and reset
    st = sim.derive_stats()
    assert st["calls"] == 2 and st["runs_staged"] > 0 and st["seconds"] > 0
    assert sim.derive_stats(reset=True) == st
    assert sim.derive_stats() == dict(calls=0, runs_staged=0, runs_direct=0, seconds=0.0)
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    assert_same_fields(sim.derive(), second, "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_derive(h) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_derive(h) == SPH_ESTATE
    sim.phase("readback")
    assert_same_fields(sim.derive(), restate(sim), "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_derive(other._h) == SPH_ESTATE, kw
        other.close()
    # no particles: SPH_OK and n = 0
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    got = empty.derive()
    assert [got[k].shape for k in KEYS] == [(0, 3), (0,), (0, 3), (0,), (0,)] and got["neighbours"].dtype == np.uint32
    empty.close()


def read_ply(path):
    blob = open(path, "rb").read()
    head, _, body = blob.partition(b"end_header\n")
    lines = head.decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n = int(lines[2].split()[2])
    assert lines[2] == "element vertex %d" % n
    names = ("x", "y", "z", "vx", "vy", "vz", "rho", "wx", "wy", "wz", "divergence", "gx", "gy", "gz")
    assert lines[3:17] == ["property float " + k for k in names] and lines[17:] == ["property uint neighbours", ""]
    assert len(body) == n * 60
    return np.frombuffer(body, "<u4").reshape(n, 15)


def test_cli_free_particles(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_DERIVE_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_PARTICLES": "1", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["frame_%04d.ppm" % f for f in range(2)] + ["particles_%04d.ply" % f for f in range(2)]
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    for f in range(2):
        sim.simulate()
        d = sim.derive()
        rows = read_ply(tmp_path / ("particles_%04d.ply" % f))
        want = np.concatenate([np.array(sim.getPosition(), copy=True), sim.download_state()["vel"], d["rho"][:, None],
                               d["vorticity"], d["divergence"][:, None], d["grad_rho"]], axis=1)
        assert np.array_equal(rows[:, :14], words(want)), f
        assert np.array_equal(rows[:, 14], d["neighbours"]), f
    assert (d["neighbours"] > 1).any()
    sim.close()
    # a bad value prints one line and writes no particle files
    bad = tmp_path / "bad"
    bad.mkdir()
    env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_PARTICLES": "yes", "SPH_FREE_FRAMES_DIR": str(bad)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "SPH_FREE_PARTICLES=yes" in r.stderr and sorted(os.listdir(bad)) == ["frame_0000.ppm"]
