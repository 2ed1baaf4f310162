"""The pair statistics on the GPU (sph_pair_statistics): the default and the check path against
restatement (a) of tests/pair_restatement.py word for word -- rows, edges and stats --, against what the bodies and the
neighbour lists say about the same state, and the call's absence from the run's results.  Every comparison is of
integer words."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import grid_states as G
import pair_restatement as PR
import pair_states as PS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SPH_EINVAL, SPH_ESTATE = -1, -4
RADII = (0.0, 0.08, 0.025)
BINS = (1, 2, 0, 128)
_prepared = {}


def simulator(name, **kw):
    pos, vel, h, cells = PS.state(name)
    s = sph.default_settings(len(pos), True) if (float(h), cells) == (float(PS.H), 100) else G.settings_for(len(pos), float(h), cells, factory=sph.default_settings)
    sim = sph.Simulator(s, **kw)
    sim.upload_state(pos, vel)
    return sim


def want_of(sim, bins, radius, key=None):
    """restatement (a) of the state the handle holds; `key`: its pairs are found once per process and shared"""
    k = None if key is None else (key, radius)
    if k is None or k not in _prepared:
        st = sim.download_state()
        p = PR.prepared(st["pos"], st["vel"], sim.settings.h, radius)
        if k is None:
            return p.table(PR.edges2(radius, sim.settings.h, bins))
        _prepared[k] = p
    return _prepared[k].table(PR.edges2(radius, sim.settings.h, bins))


def both_paths(sim, monkeypatch, what, bins=0, radius=0.0, key=None):
    """pair_statistics() on the default and on the check path, rows, edges and stats equal to restatement (a)
    -> (the table, the default path's stats)"""
    want = want_of(sim, bins, radius, key)
    total = int(want["pairs"].sum())
    ran = 1 if sim.settings.numParticles else 0
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_PAIRS_PLAIN", plain)
        sim.pair_stats(reset=True)
        got = sim.pair_statistics(bins, radius)
        st = sim.pair_stats(reset=True)
        PR.assert_same_table(got, want, f"{what}, {bins} bins, radius {radius}, plain={plain}")
        assert got["edges2"].dtype == F and got["pairs"].dtype == np.uint64
        assert PR.describe_difference(PR.from_rows(got["rows"], got["edges2"]), want) == []
        assert (st["calls"], st["pairs"]) == (ran, total), (what, st)
        assert (0.0 < st["seconds"] < 1.0) if ran else st["seconds"] == 0.0, st
        if plain == "0":
            result, stats = got, st
        else:
            assert (st["runs_staged"], st["runs_direct"]) == (0, 0), st
    monkeypatch.setenv("SPH_PAIRS_PLAIN", "0")
    return result, stats


# ---- the smallest shapes that can go wrong ----

@pytest.mark.parametrize("name", PS.TAILS)
def test_wave_tails(name, monkeypatch):
    sim = simulator(name)
    n = sim.settings.numParticles
    got, st = both_paths(sim, monkeypatch, name)
    both_paths(sim, monkeypatch, name, 5, 0.03)
    assert got["pairs"].sum() > 0 if n > 2 else got["pairs"].sum() <= 1
    assert st["runs_staged"] >= (n + 63) // 64 and st["runs_direct"] == 0, st
    sim.close()


def test_nobody_near_and_two_coincident_particles(monkeypatch):
    sim = simulator("far_pair")
    got, _ = both_paths(sim, monkeypatch, "two particles far apart")
    assert not got["pairs"].any() and not got["saturated"].any() and not got["words"].any()
    assert len(got["edges2"]) == 32 and got["edges2"][-1] == sim.settings.h * sim.settings.h
    sim.close()
    sim = simulator("coincident")
    for radius in RADII:
        got, _ = both_paths(sim, monkeypatch, "two coincident particles", 0, radius)
        assert got["pairs"].tolist() == [1] + [0] * 31
        assert got["sums"][0, 0] == 0 and got["sums"][0, 3] == 0 and got["sums"][0, 2] == 0 and got["sums"][0, 1] > 0
    sim.close()


def test_pairs_on_and_about_every_edge(monkeypatch):
    pos, edges = PS.on_the_edges()
    PS.assert_edges_straddled(pos, edges)
    sim = simulator("edges")
    got, _ = both_paths(sim, monkeypatch, "edges", PS.EDGE_BINS)
    assert np.array_equal(got["edges2"].view(np.uint32), edges.view(np.uint32)) and (got["pairs"] > 0).all()
    # the same particles through a table whose edges fall elsewhere, and through one bin
    both_paths(sim, monkeypatch, "edges", 7)
    one, _ = both_paths(sim, monkeypatch, "edges", 1)
    assert one["pairs"].tolist() == [int(got["pairs"].sum())]
    sim.close()


def test_bins_and_radii(monkeypatch):
    sim = simulator("dense4096")
    totals = {}
    for radius in RADII:
        for bins in BINS:
            got, st = both_paths(sim, monkeypatch, "dense4096", bins, radius, key=("dense4096", 0))
            assert len(got["pairs"]) == (bins or 32) and st["runs_staged"] > 0
            totals.setdefault(radius, set()).add(int(got["pairs"].sum()))
    assert all(len(t) == 1 for t in totals.values()) and min(totals[0.0]) > min(totals[0.08]) > min(totals[0.025]) > 0
    sim.close()


def test_runs_of_exactly_the_slice_and_one_more(monkeypatch):
    # a ball of SLICE rows in one cell (whole waves, a union of exactly the slice: staged) and one of SLICE + 1 (direct)
    sim = simulator("slice")
    got, st = both_paths(sim, monkeypatch, "balls of SLICE and SLICE + 1")
    assert (st["runs_staged"], st["runs_direct"]) == (PS.SLICE // 64, -(-(PS.SLICE + 1) // 64)), st
    assert int(got["pairs"].sum()) == PS.SLICE * (PS.SLICE - 1) // 2 + (PS.SLICE + 1) * PS.SLICE // 2
    both_paths(sim, monkeypatch, "balls of SLICE and SLICE + 1", 128, 0.04)
    sim.close()


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("dense4096", 5), ("random4096", 0), ("random4096", 5)])
def test_several_tiles_per_workgroup_every_sweep_and_fast_math(name, steps, monkeypatch):
    sim = simulator(name)
    for _ in range(steps):
        sim.simulate()
    key = (name, steps)
    results = {}
    for bins, radius in ((0, 0.0), (16, 0.08)):
        results[bins, radius], st = both_paths(sim, monkeypatch, f"{name} + {steps} steps", bins, radius, key=key)
        assert st["runs_staged"] > 64      # 64 tiles of several runs each (one tile per workgroup: the launch holds 64)
    state = sim.download_state()
    sim.close()
    # the sweeps that keep a sorted stream of their own, and a fast-math handle: the same words of the same state
    for kw in (dict(sweep="lds"), dict(sweep="direct"), dict(math="fast")):
        other = simulator(name, **kw)
        for _ in range(steps):
            other.simulate()
        mine = other.download_state()
        same = all(np.array_equal(mine[k].view(np.uint32), state[k].view(np.uint32)) for k in ("pos", "vel"))
        assert same or (steps > 0 and "math" in kw), kw
        for (bins, radius), want in results.items():
            got = other.pair_statistics(bins, radius)
            PR.assert_same_table(got, want if same else want_of(other, bins, radius), f"{name} + {steps} steps, {kw}")
        other.close()


@pytest.mark.parametrize("name", ["dense4096", "random4096"])
def test_a_workgroup_keeps_its_table_across_its_tiles(name, monkeypatch):
    """The default launch holds a workgroup per tile for states of this size; SPH_PAIRS_WORKGROUPS makes 1, 3 and 5
    workgroups pull the 64 tiles from the counter, so each accumulates on top of a table it has already carried."""
    sim = simulator(name)
    tiles = -(-sim.settings.numParticles // 64)
    counted = {}
    for workgroups in (1, 3, 5, 0):
        assert workgroups < tiles == 64
        monkeypatch.setenv("SPH_PAIRS_WORKGROUPS", str(workgroups))
        for bins, radius in ((0, 0.0), (16, 0.08), (128, 0.025)):
            _, st = both_paths(sim, monkeypatch, f"{name}, {workgroups} workgroups", bins, radius, key=(name, 0))
            # the runs are a property of the tiles, whoever walks them
            assert counted.setdefault((bins, radius), (st["runs_staged"], st["runs_direct"])) == (st["runs_staged"], st["runs_direct"])
    sim.close()


@pytest.mark.parametrize("workgroups", [1, 2, 0])
def test_high_words_shed_into_top_words_between_tiles(workgroups, monkeypatch):
    """Five tiles whose clamped terms, 2^31 high units each and of either sign, pass 2^34 high units per bin: with the
    shedding threshold lowered to 2^33 (SPH_PAIRS_SHED_BITS) a high word sheds into its top word at the end of a tile,
    is added to again, and the join folds lo, hi and top of every partial row into the restatement's words."""
    sim = simulator("saturating_tiles")
    assert -(-sim.settings.numParticles // 64) == 5
    monkeypatch.setenv("SPH_PAIRS_WORKGROUPS", str(workgroups))
    for shed in ("33", "40", "62"):
        monkeypatch.setenv("SPH_PAIRS_SHED_BITS", shed)
        for bins in (4, 1, 0):
            got, _ = both_paths(sim, monkeypatch, f"saturating tiles, {workgroups} workgroups, shed {shed}", bins, key=("saturating_tiles", 0))
            if bins == 1:
                assert int(got["sums"][0, 1]) >= 1 << 66 and int(got["saturated"][0]) > 64
    four = want_of(sim, 4, 0.0, key=("saturating_tiles", 0))
    assert max(int(s) for s in four["sums"][:, 1]) >= 1 << 66
    # terms clamped at the bottom too: a bin's e.dv sum is the sum of its terms, of which some are INT64_MIN
    clamped = _prepared[("saturating_tiles", 0), 0.0].q[2].tolist()
    assert PR.INT64_MIN in clamped and PR.INT64_MAX in clamped
    sim.close()


def test_more_than_two_to_the_24_particles(monkeypatch):
    """The default path refuses an n beyond the bound up to which none of its accumulators can wrap; the check path,
    whose atomics carry their own wraps, takes it, and counts what the neighbour lists count."""
    n = (1 << 24) + 1
    s = sph.default_settings(n, True)
    pos = (np.random.default_rng(24).random((n, 3), dtype=F) * F(s.boxDim) * F(0.999)).astype(F)
    sim = sph.Simulator(s, flags=_lib.SPH_FLAG_NO_READBACK)
    sim.upload_state(pos, np.zeros((n, 3), F))
    monkeypatch.setenv("SPH_PAIRS_PLAIN", "0")
    with pytest.raises(sph.SphError) as err:
        sim.pair_statistics(8, 0.01)
    assert f"({SPH_EINVAL})" in str(err.value) and str(n) in str(err.value) and str(1 << 24) in str(err.value)
    assert sim._L.sph_pair_statistics_host(sim._h, None, None, None) == SPH_ESTATE
    monkeypatch.setenv("SPH_PAIRS_PLAIN", "1")
    got = sim.pair_statistics(8, 0.01)
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    entries = len(sim.neighbour_lists(0.01, walk_order=True)["neighbours"])
    assert 2 * int(got["pairs"].sum()) == entries > 0 and not got["saturated"].any()
    sim.close()


@pytest.mark.parametrize("name", ["D1", "D2", "D3", "D10h025"])
def test_grids_of_a_few_cells_with_rows_on_the_walls(name, monkeypatch):
    sim = simulator(name)
    h = float(sim.settings.h)
    for bins, radius in ((0, 0.0), (9, 0.5 * h)):
        got, _ = both_paths(sim, monkeypatch, name, bins, radius, key=(name, 0))
        assert got["pairs"].sum() > 0
    sim.close()


def test_saturation_and_nan(monkeypatch):
    sim = simulator("saturating")
    for bins in (0, 4, 1):
        got, _ = both_paths(sim, monkeypatch, "saturating", bins, key=("saturating", 0))
        assert got["saturated"].sum() > 40
        assert max(int(s) for s in got["sums"][:, 1]) >= PR.INT64_MAX      # a clamped |dv|^2, and more on top of it
    # a radius so small that its square is 0 and every edge of the table with it: the coincident pair alone, in bin 0
    tiny, _ = both_paths(sim, monkeypatch, "saturating", 128, 1e-30)
    assert not tiny["edges2"].any() and tiny["pairs"].tolist() == [1] + [0] * 127
    # a denormal radius: bins / radius is inf, and the search's first guess must still be a bin
    tiny, _ = both_paths(sim, monkeypatch, "saturating", 32, 1e-40)
    assert not tiny["edges2"].any() and tiny["pairs"].tolist() == [1] + [0] * 31
    sim.close()


@pytest.mark.parametrize("name,steps", [("dense4096", 3), ("random4096", 0)])
def test_pins_to_the_bodies_and_the_neighbour_lists(name, steps, monkeypatch):
    for env in ("SPH_PAIRS_PLAIN", "SPH_NEIGHBOURS_PLAIN", "SPH_BODIES_PLAIN"):
        monkeypatch.setenv(env, "0")
    sim = simulator(name)
    for _ in range(steps):
        sim.simulate()
    for radius in RADII:
        pairs = int(sim.pair_statistics(7, radius)["pairs"].sum())
        sim.body_stats(reset=True)
        sim.label_bodies(radius)
        entries = len(sim.neighbour_lists(radius)["neighbours"])
        assert pairs == sim.body_stats()["links"] and 2 * pairs == entries and (pairs > 0 or radius == 0.025), radius
    sim.close()


def run(timed, calling, steps=8):
    sim = simulator("dense4096")
    times = sph.Times()
    totals = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if calling:
            totals.append(int(sim.pair_statistics(16, 0.08)["pairs"].sum()))
    digest = hashlib.sha256(np.array(sim.getPosition(), copy=True).tobytes() + sim.download_state()["vel"].tobytes()).hexdigest()
    sim.close()
    return digest, totals


@pytest.mark.parametrize("timed", [False, True])
def test_calls_between_every_two_steps_leave_the_run_untouched(timed, monkeypatch):
    monkeypatch.setenv("SPH_PAIRS_PLAIN", "0")
    with_, totals = run(timed, True)
    without, _ = run(timed, False)
    assert with_ == without, f"timed={timed}: the state after 8 steps differs"
    assert len(totals) == 8 and min(totals) > 0 and len(set(totals)) > 1


def test_state_rules_refusals_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_PAIRS_PLAIN", "0")
    pos, vel, _, _ = PS.state("dense4096")
    sim = sph.Simulator(sph.default_settings(len(pos), True))
    L, h = sim._L, sim._h
    host = lambda: L.sph_pair_statistics_host(h, None, None, None)

    def opt(radius=0.0, bins=0, flags=0, pad=0, size=C.sizeof(_lib.SphPairOptions)):
        return C.byref(_lib.SphPairOptions(size, flags, radius, bins, pad))

    # before any state, and the results before the first call
    assert L.sph_pair_statistics(h, None) == SPH_ESTATE
    assert host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    assert host() == SPH_ESTATE
    # the options
    assert L.sph_pair_statistics(h, opt(0.05, size=0)) == SPH_EINVAL
    for bad in (float("nan"), float("inf"), -1.0, 1.5 * float(sim.settings.h), float(np.nextafter(F(sim.settings.h), F(1)))):
        assert L.sph_pair_statistics(h, opt(bad)) == SPH_EINVAL, bad
    for flags in (1, 2, 1 << 30, -1):
        assert L.sph_pair_statistics(h, opt(flags=flags)) == SPH_EINVAL, flags
    assert L.sph_pair_statistics(h, opt(pad=1)) == SPH_EINVAL
    for bins in (-1, 129, 1 << 20):
        assert L.sph_pair_statistics(h, opt(bins=bins)) == SPH_EINVAL, bins
    assert sim._L.sph_last_error(h)
    assert host() == SPH_ESTATE
    assert L.sph_pair_statistics(h, None) == 0          # NULL: every default
    assert host() == 0
    rows, edges, bins = C.POINTER(_lib.SphPairBinRaw)(), C.POINTER(C.c_float)(), C.c_int(-1)
    assert L.sph_pair_statistics_host(h, C.byref(rows), C.byref(edges), C.byref(bins)) == 0 and bins.value == 32
    first = sim.pair_statistics()
    PR.assert_same_table(first, want_of(sim, 0, 0.0, key=("dense4096", 0)), "every default")
    PR.assert_same_table(sim.pair_statistics(32, float(sim.settings.h)), first, "32 bins up to h against the defaults")
    # a refused call and a later step leave the result alone; a new call replaces it
    assert L.sph_pair_statistics(h, opt(bins=129)) == SPH_EINVAL
    sim.simulate()
    assert L.sph_pair_statistics_host(h, C.byref(rows), C.byref(edges), C.byref(bins)) == 0 and bins.value == 32
    assert [rows[k].pairs for k in range(32)] == first["pairs"].tolist()
    second = sim.pair_statistics(8, 0.05)
    PR.assert_same_table(second, want_of(sim, 8, 0.05), "after a step")
    assert L.sph_pair_statistics_host(h, C.byref(rows), C.byref(edges), C.byref(bins)) == 0 and bins.value == 8
    assert [rows[k].pairs for k in range(8)] == second["pairs"].tolist()
    # the values are the restatement's, bit for bit
    got, want = sim.pair_values(second), PR.values(second, sim.settings.boxDim, len(pos))
    for k in range(8):
        for name in PR.VALUE_FIELDS[:-1]:
            assert np.float64(got[name][k]).view(np.uint64) == np.float64(want[k][name]).view(np.uint64), (k, name)
    assert got["g"][-1] > 0 and (np.diff(got["r_hi"]) > 0).all()
    # the stats sum over calls and reset
    sim.pair_stats(reset=True)
    sim.pair_statistics(8, 0.05)
    sim.pair_statistics(3, 0.05)
    st = sim.pair_stats()
    assert (st["calls"], st["pairs"]) == (2, 2 * int(second["pairs"].sum())) and st["seconds"] > 0 and st["runs_staged"] > 0
    assert sim.pair_stats(reset=True) == st
    assert sim.pair_stats() == dict(calls=0, pairs=0, runs_staged=0, runs_direct=0, seconds=0.0)
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    PR.assert_same_table(sim.pair_statistics(8, 0.05), second, "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_pair_statistics(h, None) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_pair_statistics(h, None) == SPH_ESTATE
    sim.phase("readback")
    assert L.sph_pair_statistics(h, None) == 0
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_pair_statistics(other._h, None) == SPH_ESTATE, kw
        assert other._L.sph_last_error(other._h), kw
        other.close()
    # no particles: SPH_OK and an all-zero table with its edges
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_PAIRS_PLAIN", plain)
        got = empty.pair_statistics(6)
        assert len(got["pairs"]) == 6 and not got["rows"].view(np.uint64).any()
        assert np.array_equal(got["edges2"].view(np.uint32), PR.edges2(0.0, empty.settings.h, 6).view(np.uint32))
    assert empty.pair_stats()["calls"] == 0
    empty.close()


def test_cli_free_pair_stats(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_PAIRS_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_PAIR_STATS": "16", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["frame_%04d.ppm" % f for f in range(2)] + ["pair_stats_%04d.jsonl" % f for f in range(2)]
    said = [l.split() for l in r.stderr.splitlines() if l.startswith("pairs ")]
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    for f in range(2):
        sim.simulate()
        stats = sim.pair_statistics(16)
        want = sim.pair_values(stats)
        lines = [json.loads(l) for l in open(tmp_path / ("pair_stats_%04d.jsonl" % f))]
        assert [l["bin"] for l in lines] == list(range(16))
        for k, l in enumerate(lines):
            for name in PR.VALUE_FIELDS:
                assert l[name] == want[name][k], (f, k, name)
        assert said[f] == ["pairs", str(f), str(int(stats["pairs"].sum())), str(int(stats["saturated"].sum()))], said
        assert stats["pairs"].sum() > 0
    sim.close()
    # a bad value prints one line and writes no pair statistics
    for value in ("yes", "0", "129", "1.5"):
        bad = tmp_path / ("bad" + value)
        bad.mkdir()
        env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_PAIR_STATS": value, "SPH_FREE_FRAMES_DIR": str(bad)})
        r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and ("SPH_FREE_PAIR_STATS=" + value) in r.stderr and sorted(os.listdir(bad)) == ["frame_0000.ppm"], value
