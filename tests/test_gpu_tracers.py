"""Passive tracers on the GPU (sph_tracers_*): the default path against the numpy restatement
(tests/tracer_restatement.py) fed by sph_download_grid + sph_download_state, the check path against the default path,
what the walk kernel counted, and the tracers' absence from the run's results.  Every comparison is of fp32 words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import tracer_restatement as TR
import tracer_sets as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SWEEPS = ("list", "lds", "direct")
SPH_EINVAL, SPH_ESTATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_tracers(got, want, what):
    for k in ("pos", "den", "vel"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype == F, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = bits(a) != bits(b)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} words of {k} differ, first at {np.argwhere(bad)[0]}: " \
                              f"{a[tuple(np.argwhere(bad)[0])]!r} vs {b[tuple(np.argwhere(bad)[0])]!r}"


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def golden(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    return np.ascontiguousarray(data["pos_1"], dtype=F), np.ascontiguousarray(data["vel_1"], dtype=F)


def uploaded(name, steps=0, **kw):
    pos, vel = golden(name)
    sim = make(len(pos), **kw)
    sim.upload_state(pos, vel)
    for _ in range(steps):
        sim.simulate()
    return sim


def sorted_state(sim):
    """what the restatement is fed with: the grid the walk read and the state, row by row of the sorted stream"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    return st["pos"][ids], st["vel"][ids], g["cells"]


def restate(sim, grid, tracers, dt):
    s = sim.settings
    return TR.advect(grid[0], grid[1], grid[2], s.h, s.d_kernel_coeff, s.numCellsPerDim, tracers, dt)


def advected(sim, tracers, dt):
    sim.set_tracers(tracers)
    sim.advect_tracers(dt)
    return sim.tracers()


def sets_of(sim):
    s = sim.settings
    return TS.all_sets(sim.download_state()["pos"], s.h, int(s.numCellsPerDim))


@pytest.mark.parametrize("steps", [0, 5])
@pytest.mark.parametrize("name", ["dense4096", "random4096"])
def test_every_set_against_the_restatement_on_every_path_and_sweep(name, steps, monkeypatch):
    sims = [uploaded(name, steps, sweep=sweep) for sweep in SWEEPS]
    sets = sets_of(sims[0])
    grid = None
    hits = moved = 0
    for key, t in sets.items():
        for dt in (sims[0].settings.timestep, 0.0):
            what = f"{name} + {steps} steps, set {key}, dt = {dt}"
            monkeypatch.setenv("SPH_TRACER_PLAIN", "0")
            got = advected(sims[0], t, dt)
            if grid is None:
                grid = sorted_state(sims[0])          # (taken after the call: the grid that was walked)
            assert_same_tracers(got, restate(sims[0], grid, t, dt), what)
            if dt == 0.0:
                assert np.array_equal(bits(got["pos"]), bits(t)), what
            else:
                moved += int((bits(got["pos"]) != bits(t)).any(axis=1).sum())
            hits += int((got["den"] > 0).sum())
            for k, sim in enumerate(sims):
                for plain in ("0", "1"):
                    if k == 0 and plain == "0":
                        continue
                    monkeypatch.setenv("SPH_TRACER_PLAIN", plain)
                    assert_same_tracers(advected(sim, t, dt), got, f"{what}: sweep {SWEEPS[k]}, plain={plain}")
    assert hits > 1000 and moved > 500, f"{name}: the sets miss the fluid ({hits} hits, {moved} moved)"
    for sim in sims:
        sim.close()


def stats_of(sim, tracers, dt=0.0):
    sim.tracer_stats(reset=True)
    advected(sim, tracers, dt)
    return sim.tracer_stats(reset=True)


def test_the_counters_show_that_both_walks_ran(monkeypatch):
    monkeypatch.setenv("SPH_TRACER_PLAIN", "0")
    sim = uploaded("dense4096")
    s = sim.settings
    D = int(s.numCellsPerDim)
    sets = sets_of(sim)
    st = stats_of(sim, sets["A"])
    assert TS.wave_groups(sets["A"], s.h, D) == [1, 1, 1, 1]
    assert (st["calls"], st["waves_shared"], st["waves_direct"], st["groups"]) == (1, 4, 0, 4), st
    assert 0.0 < st["seconds"] < 1.0
    assert sim.tracer_stats() == dict(calls=0, waves_shared=0, waves_direct=0, groups=0, seconds=0.0)
    for key in ("B", "C", "E"):
        want = TS.wave_groups(sets[key], s.h, D)
        st = stats_of(sim, sets[key])
        assert st["groups"] == sum(want) and st["waves_shared"] + st["waves_direct"] == len(want), (key, st, want)
    # D: one wave of 64 tracers from g rows of cells, g = 1 .. 25: few groups walk shared, many walk direct
    shared, direct = [], []
    for g in range(1, 26):
        want = TS.wave_groups(sets["D%d" % g], s.h, D)
        st = stats_of(sim, sets["D%d" % g])
        assert len(want) == 1 and st["groups"] == want[0] >= g, (g, st, want)
        assert st["waves_shared"] + st["waves_direct"] == 1, (g, st)
        (shared if st["waves_shared"] else direct).append(want[0])
    assert shared, f"no wave of D walked shared: group counts {sorted(direct)}"
    assert direct, f"G >= {max(shared)}: no wave of D walked direct, the direct walk of the default path is not covered here"
    assert max(shared) < min(direct), f"the walk does not depend on the group count alone: shared {sorted(shared)}, direct {sorted(direct)}"
    # sums over calls; the check path counts no wave
    sim.tracer_stats(reset=True)
    for _ in range(3):
        advected(sim, sets["A"], 0.0)
    monkeypatch.setenv("SPH_TRACER_PLAIN", "1")
    advected(sim, sets["A"], 0.0)
    st = sim.tracer_stats()
    assert (st["calls"], st["waves_shared"], st["waves_direct"], st["groups"]) == (4, 12, 0, 12), st
    sim.close()
    # the scatter on random4096: every lane a group of its own
    monkeypatch.setenv("SPH_TRACER_PLAIN", "0")
    sim = uploaded("random4096")
    t = TS.scatter(golden("random4096")[0])
    want = TS.wave_groups(t, s.h, D)
    st = stats_of(sim, t)
    assert want == [64, 64, 22] and st["groups"] == 150
    assert st["waves_shared"] == 0 and st["waves_direct"] == 3, f"G >= 22? {st}"
    sim.close()


def test_den_is_the_field_sample_at_the_tracer():
    sim = uploaded("dense4096")
    t = TS.scatter(golden("dense4096")[0])[:32]
    got = advected(sim, t, 0.0)
    assert (got["den"] > 0).all()
    for i, p in enumerate(t):
        want = sim.sample_field("density", tuple(float(v) for v in p), (0.1,) * 3, (1, 1, 1))
        assert bits(got["den"][i]).item() == bits(want).item(), i
    sim.close()


def trajectory(timed, with_tracers, steps=5):
    """`steps` x (step, advect) with set C on dense4096: the state after every step, the tracers after every advect
    and what the restatement makes of the same grid and the tracers before it"""
    sim = uploaded("dense4096")
    times = sph.Times()
    t = TS.scatter(golden("dense4096")[0])
    if with_tracers:
        sim.set_tracers(t)
    states, got, want = [], [], []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if with_tracers:
            sim.advect_tracers()
            got.append(sim.tracers())
            want.append(restate(sim, sorted_state(sim), t, sim.settings.timestep))
            t = want[-1]["pos"]
        states.append(sim.download_state())
    host = np.array(sim.getPosition(), copy=True)
    sim.close()
    return states, got, want, host


@pytest.mark.parametrize("timed", [False, True])
def test_trajectory_and_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_TRACER_PLAIN", "0")
    states, got, want, host = trajectory(timed, True)
    start = TS.scatter(golden("dense4096")[0])
    for k in range(5):
        assert_same_tracers(got[k], want[k], f"timed={timed}, step {k}")
    assert (bits(got[-1]["pos"]) != bits(start)).any(axis=1).sum() > 100
    without, _, _, host0 = trajectory(timed, False)
    for k in range(5):
        for key in ("pos", "vel", "rho"):
            assert np.array_equal(bits(states[k][key]), bits(without[k][key])), f"timed={timed}, step {k}: {key} differs"
    assert np.array_equal(bits(host), bits(host0))


def click_sequence(timed, tracing, order):
    """6 steps, then the calls of `order` ("c" a click, "a" an advect, skipped without tracing), then 2 more steps"""
    sim = make(4096)
    sim.setup()
    if tracing:
        sim.set_tracers(np.array(sim.getPosition(), copy=True)[::40])
    times = sph.Times()
    step = (lambda: sim.simulateAndTime(times)) if timed else sim.simulate
    for _ in range(6):
        step()
    for call in order:
        if call == "c":
            sim.moveParticles((400, 300))
        elif tracing:
            sim.advect_tracers()
    mid = sim.download_state()
    for _ in range(2):
        step()
    out = sim.download_state()
    out["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return mid, out


@pytest.mark.parametrize("timed,pipeline,order", [(True, "1", "caca"), (False, "1", "acac"), (True, "0", "acacac"), (False, "0", "cacac")])
def test_clicks_between_advects_walk_the_last_steps_table(timed, pipeline, order, monkeypatch):
    monkeypatch.setenv("SPH_PIPELINE", pipeline)
    mid1, end1 = click_sequence(timed, True, order)
    mid0, end0 = click_sequence(timed, False, order)
    assert np.array_equal(bits(mid1["vel"]), bits(mid0["vel"])), f"{order}: velocities after the clicks differ"
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(bits(end1[k]), bits(end0[k])), f"timed={timed} SPH_PIPELINE={pipeline} {order}: {k} differs"
    # ... and every click of the sequence did something: one click fewer gives other velocities
    fewer, _ = click_sequence(timed, False, order.replace("c", "", 1))
    assert not np.array_equal(bits(fewer["vel"]), bits(mid0["vel"]))


def test_state_rules_error_codes_and_ownership(monkeypatch):
    monkeypatch.setenv("SPH_TRACER_PLAIN", "0")
    pos, vel = golden("dense4096")
    sim = make(len(pos))
    L, h = sim._L, sim._h
    fp = C.POINTER(C.c_float)
    a = TS.blob()
    # tracers can be set before any state; advecting them cannot
    sim.set_tracers(a)
    assert L.sph_tracers_advect(h, C.c_float(0.0)) == SPH_ESTATE
    before = sim.tracers()
    assert np.array_equal(bits(before["pos"]), bits(a)) and (bits(before["den"]) == 0).all() and (bits(before["vel"]) == 0).all()
    sim.upload_state(pos, vel)
    # SPH_EINVAL
    assert L.sph_tracers_set(h, a.ctypes.data_as(fp), -1) == SPH_EINVAL
    assert L.sph_tracers_set(h, a.ctypes.data_as(fp), (1 << 24) + 1) == SPH_EINVAL
    assert L.sph_tracers_set(h, None, 1) == SPH_EINVAL
    for dt in (float("nan"), float("inf"), float("-inf")):
        assert L.sph_tracers_advect(h, C.c_float(dt)) == SPH_EINVAL
    assert np.array_equal(bits(sim.tracers()["pos"]), bits(a))          # the failed calls changed nothing
    # tracers survive an upload; the advect samples the new state
    sim.advect_tracers(0.0)
    first = sim.tracers()
    assert (first["den"] > 0).all()
    sim.upload_state(pos, vel)
    sim.advect_tracers()
    assert_same_tracers(sim.tracers(), restate(sim, sorted_state(sim), a, sim.settings.timestep), "after a second upload")
    # set replaces, m = 0 clears, an advect without tracers is SPH_OK and does nothing
    b = TS.line()
    sim.set_tracers(b)
    got = sim.tracers()
    assert np.array_equal(bits(got["pos"]), bits(b)) and (bits(got["den"]) == 0).all() and (bits(got["vel"]) == 0).all()
    sim.set_tracers(np.zeros((0, 3), F))
    calls = sim.tracer_stats()["calls"]
    sim.advect_tracers()
    assert sim.tracer_stats()["calls"] == calls
    empty = sim.tracers()
    assert empty["pos"].shape == (0, 3) and empty["den"].shape == (0,) and empty["vel"].shape == (0, 3)
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.set_tracers(a)
    sim.phase("grid")
    sim.advect_tracers(0.0)
    assert_same_tracers(sim.tracers(), {**first, "pos": a}, "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_tracers_advect(h, C.c_float(0.0)) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_tracers_advect(h, C.c_float(0.0)) == SPH_ESTATE
    sim.phase("readback")
    sim.advect_tracers(0.0)
    assert_same_tracers(sim.tracers(), restate(sim, sorted_state(sim), a, 0.0), "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = make(4096, **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
            other.set_tracers(a)
        assert other._L.sph_tracers_advect(other._h, C.c_float(0.0)) == SPH_ESTATE, kw
        other.close()


def test_no_particles_every_tracer_keeps_its_words(monkeypatch):
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_TRACER_PLAIN", plain)
        empty = make(0)
        empty.setup()
        t = TS.specials(golden("dense4096")[0])
        got = advected(empty, t, empty.settings.timestep)
        assert np.array_equal(bits(got["pos"]), bits(t)) and (bits(got["den"]) == 0).all() and (bits(got["vel"]) == 0).all()
        empty.close()


def read_ply(path):
    blob = open(path, "rb").read()
    head, _, body = blob.partition(b"end_header\n")
    lines = head.decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    m = int(lines[2].split()[2])
    assert lines[2] == "element vertex %d" % m
    assert lines[3:10] == ["property float " + k for k in ("x", "y", "z", "vx", "vy", "vz", "density")] and lines[10] == ""
    assert len(body) == m * 28
    return np.frombuffer(body, "<f4").reshape(m, 7)


def test_cli_free_tracers(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_TRACER_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "6", "SPH_FREE_TRACERS": "100", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["frame_%04d.ppm" % f for f in range(6)] + ["tracers_%04d.ply" % f for f in range(6)]
    sim = make(4096, random=False)
    sim.setup()
    seeds = np.array(sim.getPosition(), copy=True)[[k * 4096 // 100 for k in range(100)]]
    sim.set_tracers(seeds)
    moved = 0
    for f in range(6):
        sim.simulate()
        sim.advect_tracers()
        t = sim.tracers()
        rows = read_ply(tmp_path / ("tracers_%04d.ply" % f))
        want = np.concatenate([t["pos"], t["vel"], t["den"][:, None]], axis=1)
        assert np.array_equal(bits(rows), bits(want)), f
        moved += int((t["den"] > 0).sum())
    assert moved > 300
    sim.close()
    # a bad count prints one line and writes no tracers
    bad = tmp_path / "bad"
    bad.mkdir()
    env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_TRACERS": "0", "SPH_FREE_FRAMES_DIR": str(bad)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "SPH_FREE_TRACERS=0" in r.stderr and sorted(os.listdir(bad)) == ["frame_0000.ppm"]
