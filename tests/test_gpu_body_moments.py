"""Per-body moments on the GPU (sph_measure_bodies): the default path (wave groups, the LDS
fold of a block's first body) and the check path (one atomic per word) against the restatement
(tests/body_moments_restatement.py) fed by sph_download_grid + sph_download_state after the call, byte for byte; the
labelling, the table and the diagnostics of the same state on the device; the call's absence from the run's results;
the state rules; the command-line front end."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import body_moments_restatement as M
import body_states as BS
import grid_states as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
U = np.uint32
SPH_EINVAL, SPH_ESTATE, SPH_ENOMEM = -1, -4, -3


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def simulator(pos, vel=None, h=0.1, cells=100, **kw):
    vel = np.zeros_like(pos) if vel is None else vel
    s = sph.default_settings(len(pos), True) if (h, cells) == (0.1, 100) else G.settings_for(len(pos), h, cells, factory=sph.default_settings)
    sim = sph.Simulator(s, **kw)
    sim.upload_state(pos, vel)
    return sim


def velocities(n, seed, nan=False):
    """test_gpu_diagnostics.small_state's: both signs, some at 2^-30, one row at 1e6 (its v2 saturates), terms below a
    unit of Q32.32 and a denormal; nan: NaN and infinite ones too"""
    rng = np.random.default_rng(seed)
    vel = (rng.uniform(-3, 3, (n, 3)) * rng.choice([1.0, 2.0**-30], (n, 1))).astype(F)
    vel[n // 2] = (1e6, -0.75, 2.0**-30)
    if n >= 3:
        vel[n // 2 + 1] = (-(2.0**-40), 2.0**-40, -0.0)
        vel[n // 2 - 1] = (-(2.0**-33), -1e-40, 1e-40)
    if nan:
        vel[n // 3, 1] = np.nan
        vel[(2 * n) // 3] = np.nan
        vel[n // 4] = (-(2.0**31), np.inf, -np.inf)
    return vel


_bodies = {}  # the bodies' restatement of a shared state as uploaded, by (name, link): computed once, never written to


def restate(sim, link, shared=None):
    """(the bodies' restatement over the grid the sweep walked, the moments' restatement over its labels, the state):
    call after measure_bodies().  shared: the name of a body_states.big state the simulator holds as uploaded (the
    bodies depend on the positions and the grid alone, and both are checked to be the ones restated before)"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    s = sim.settings
    if shared is None or (shared, link) not in _bodies:
        b = BR.bodies(st["pos"][ids], ids, g["cells"], s.h, int(s.numCellsPerDim), link)
        if shared is not None:
            _bodies[shared, link] = (b, st["pos"].copy(), ids.copy())
    else:
        b, pos, order = _bodies[shared, link]
        assert np.array_equal(words(pos), words(st["pos"])) and np.array_equal(order, ids)
    return b, M.restate(st["pos"], st["vel"], st["rho"], b["labels"]), st


def assert_same_bodies(got, want, what):
    assert got["num_bodies"] == want["num_bodies"], f"{what}: {got['num_bodies']} bodies, not {want['num_bodies']}"
    for k in ("labels", "table"):
        assert got[k].dtype == want[k].dtype == U and np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    assert got["largest"] == want["largest"], what


def assert_same_moments(got, bodies, what):
    M.assert_same_rows(got["moments"], M.to_rows(bodies), what)
    assert got["size_hist"].dtype == U and np.array_equal(got["size_hist"], M.size_hist(bodies)), f"{what}: size_hist"
    assert np.array_equal(got["moments"]["count"], got["table"][:, 1]) and np.array_equal(got["moments"]["label"], got["table"][:, 0]), what


def both_paths(sim, monkeypatch, what, link=0.0, shared=None):
    """measure_bodies() on the default and on the check path, both equal to the restatements byte for byte
    -> (the default path's result, the restated bodies of the moments)"""
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    sim.body_measure_stats(reset=True)
    got = sim.measure_bodies(link)
    want, bodies, _ = restate(sim, link, shared)
    assert_same_bodies(got, want, what + ", default path")
    assert_same_moments(got, bodies, what + ", default path")
    monkeypatch.setenv("SPH_BODIES_PLAIN", "1")
    plain = sim.measure_bodies(link)
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    assert_same_bodies(plain, want, what + ", check path")
    assert_same_moments(plain, bodies, what + ", check path")
    st = sim.body_measure_stats(reset=True)
    assert st["calls"] == 2 and 0.0 < st["seconds"] < 1.0, (what, st)
    return got, bodies


def total(rows, k):
    """sum k over all bodies as a Python int"""
    return sum(b["sums"][M.SUMS[k]] for b in M.from_rows(rows))


def assert_pins_on_the_device(sim, got, link, what, saturated_too):
    """the labelling is label_bodies's, and the first nine sums over the bodies are sph_diagnose's"""
    assert_same_bodies(got, sim.label_bodies(link), what + ": measure_bodies against label_bodies")
    sim.diagnose()
    raw = sim.diagnostics_raw()
    for k in range(9):
        S = (raw.sum[k].hi << 64) | raw.sum[k].lo
        assert total(got["moments"], k) == S, f"{what}: sum {M.SUMS[k]} over the bodies against sph_diagnose"
    if saturated_too:  # (no special term among the moments' own nine)
        assert int(got["moments"]["saturated"].sum()) == raw.saturated, what


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("random4096", 0), ("uniform4096", 0),
                                        ("dense4096", 5), ("random4096", 5), ("uniform4096", 5)])
def test_moments_are_the_restatement_on_both_paths_and_every_sweep(name, steps, monkeypatch):
    pos, vel = BS.big(name)
    links = [l for s, l in BS.BIG if s == name]
    sim = simulator(pos, vel)
    for _ in range(steps):
        sim.simulate()
    results = {}
    for link in links:
        results[link], _ = both_paths(sim, monkeypatch, f"{name} + {steps} steps, link {link}", link, name if steps == 0 else None)
    assert_pins_on_the_device(sim, results[links[0]], links[0], f"{name} + {steps} steps", True)
    if (name, steps) == ("uniform4096", 0):  # (the shapes tests/test_body_moments_cpu.py found in this state)
        assert results[0.0]["num_bodies"] == 89 and results[0.08]["num_bodies"] == 785
        assert int((results[0.08]["size_hist"] > 0).sum()) == 8
    sim.close()
    # the sweeps that keep a sorted position stream of their own read the same words
    for sweep in ("lds", "direct"):
        other = simulator(pos, vel, sweep=sweep)
        for _ in range(steps):
            other.simulate()
        for link in links:
            got = other.measure_bodies(link)
            what = f"{name} + {steps} steps, link {link}, sweep {sweep}"
            assert_same_bodies(got, results[link], what)
            st = other.download_state()
            assert_same_moments(got, M.restate(st["pos"], st["vel"], st["rho"], got["labels"]), what)
        other.close()


@pytest.mark.parametrize("name,link", BS.BIG)
def test_tiny_huge_nan_and_infinite_velocities(name, link, monkeypatch):
    pos, _ = BS.big(name)
    n = len(pos)
    for nan in (False, True):
        sim = simulator(pos, velocities(n, 5, nan))
        got, bodies = both_paths(sim, monkeypatch, f"{name}, link {link}, nan {nan}", link, name)
        sat = {b["label"]: b["saturated"] for b in bodies}
        lab = got["labels"]
        # the row at 1e6: its v2 saturates, nothing else of it; with nan the NaN and infinite rows' terms on top
        assert sat[int(lab[n // 2])] >= 1 and (nan or sum(sat.values()) == 1)
        if nan:
            for row in (n // 3, (2 * n) // 3, n // 4):
                assert sat[int(lab[row])] >= 2, row
            assert sum(sat.values()) > 10
        assert got["moments"]["saturated"].tolist() == [b["saturated"] for b in bodies]
        st = sim.download_state()
        assert np.isfinite(st["pos"]).all() and (st["pos"] >= 0).all() and (st["pos"] < 10).all()
        assert_pins_on_the_device(sim, got, link, f"{name}, nan {nan}", saturated_too=not nan)
        sim.close()


# ---- the smallest shapes that can go wrong ----

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
    sim = simulator(np.array([[5.0625, 5.125, 5.25]], F), np.array([[0.5, -2.0, 4.0]], F))
    got, bodies = both_paths(sim, monkeypatch, "n = 1")
    (b,) = bodies
    assert (b["label"], b["count"], b["saturated"]) == (0, 1, 0) and got["size_hist"].tolist() == [1] + [0] * 31
    assert b["sums"]["x"] == int(5.0625 * 2**32) and b["sums"]["ly"] == int((5.25 * 0.5 - 5.0625 * 4.0) * 2**32)
    v = sim.body_values(got["moments"])[0]
    assert v["velocity"].tolist() == [0.5, -2.0, 4.0] and v["kinetic_internal"] == 0.0 and v["angular"].tolist() == [0.0, 0.0, 0.0]
    sim.close()


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_tails(n, monkeypatch):
    sim = simulator(BS.cluster(n, n), velocities(n, n))
    got, _ = both_paths(sim, monkeypatch, f"n = {n}")
    assert got["table"][:, 1].max() > 1
    sim.close()


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_a_giant_across_blocks_and_a_last_block_of_one_row(n, monkeypatch):
    sim = simulator(BS.cluster(n, n), velocities(n, n))
    got, _ = both_paths(sim, monkeypatch, f"cluster of {n}")
    if n > 2048:
        assert got["table"][:, 1].max() > 2048
    assert got["table"][:, 1].max() > n // 2
    sim.close()


def test_one_cell_chains_and_grids_of_a_few_cells(monkeypatch):
    sim = simulator(BS.one_cell(1500, 5, (50, 50, 50)), velocities(1500, 1))
    got, _ = both_paths(sim, monkeypatch, "1500 in one cell")
    assert got["num_bodies"] == 1 and got["moments"]["count"].tolist() == [1500]
    sim.close()
    for cut in (False, True):
        pos, _ = BS.chain(without_middle=cut)
        sim = simulator(pos, velocities(len(pos), 2))
        got, _ = both_paths(sim, monkeypatch, f"chain, cut {cut}")
        assert got["moments"]["count"].tolist() == ([128, 128] if cut else [257])
        sim.close()
    for name in ("D1", "D2", "D3"):
        pos, vel, g = on_the_walls(name)
        sim = simulator(pos, vel, g["h"], g["cells"])
        for link in (0.0, 0.5 * float(g["h"])):
            both_paths(sim, monkeypatch, f"{name}, link {link}", link)
        sim.close()


# ---- no footprint ----

def run(timed, measuring, steps=10):
    pos, vel = BS.big("dense4096")
    sim = simulator(pos, vel)
    times = sph.Times()
    counts = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if measuring:
            counts.append(sim.measure_bodies(0.025)["num_bodies"])
    st = sim.download_state()
    st["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return st, counts


@pytest.mark.parametrize("timed", [False, True])
def test_a_measurement_between_every_two_steps_leaves_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    with_, counts = run(timed, True)
    without, _ = run(timed, False)
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(words(with_[k]), words(without[k])), f"timed={timed}: {k} differs after 10 steps"
    assert len(counts) == 10 and min(counts) > 1


# ---- state rules, options, stats ----

def test_state_rules_error_codes_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    pos, vel = BS.big("dense4096")
    sim = sph.Simulator(sph.default_settings(len(pos), True))
    L, h = sim._L, sim._h
    outs = (C.POINTER(_lib.SphBodyMomentsRaw)(), C.c_int(-1), C.POINTER(C.c_uint32)())
    host = lambda: L.sph_body_moments_host(h, *[C.byref(o) for o in outs])
    opt = lambda link, cap=0, size=C.sizeof(_lib.SphBodyMeasureOptions), pad=0: C.byref(_lib.SphBodyMeasureOptions(size, link, cap, pad))
    # before any state, and the results before the first call
    assert L.sph_measure_bodies(h, None) == SPH_ESTATE
    assert host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    assert host() == SPH_ESTATE
    sim.label_bodies()
    assert host() == SPH_ESTATE, "a labelling alone leaves no moments"
    # the options
    assert L.sph_measure_bodies(h, opt(0.05, size=0)) == SPH_EINVAL
    assert L.sph_measure_bodies(h, opt(0.05, pad=1)) == SPH_EINVAL
    for bad in (float("nan"), float("inf"), -0.05, float(np.nextafter(F(sim.settings.h), F(1)))):
        assert L.sph_measure_bodies(h, opt(bad)) == SPH_EINVAL, bad
    assert host() == SPH_ESTATE
    assert L.sph_measure_bodies(h, None) == 0          # NULL: link = h, no cap
    assert host() == 0 and outs[1].value == 1 and outs[0][0].count == len(pos) and outs[2][12] == 1
    assert L.sph_body_moments_host(h, None, None, None) == 0
    first = sim.measure_bodies(0.0)
    M.assert_same_rows(sim.measure_bodies(float(sim.settings.h))["moments"], first["moments"], "link = h against link = 0")
    # max_bodies: at the count it passes, below it SPH_ENOMEM names both numbers, the labelling stands, the moments are gone
    sim.body_stats(reset=True)
    sim.body_measure_stats(reset=True)
    many = sim.measure_bodies(0.025)
    k = many["num_bodies"]
    assert k > 1 and sim.measure_bodies(0.025, max_bodies=k)["num_bodies"] == k
    assert L.sph_measure_bodies(h, opt(0.025, k - 1)) == SPH_ENOMEM
    msg = L.sph_last_error(h).decode()
    assert str(k) in msg and str(k - 1) in msg, msg
    assert host() == SPH_ESTATE
    assert_same_bodies(bodies_host(sim), many, "the refused call's labelling")
    # the stats: the labelling's in SphBodyStats (three calls), the moments' own (two), and their reset
    assert sim.body_stats()["calls"] == 3
    st = sim.body_measure_stats()
    assert st["calls"] == 2 and st["seconds"] > 0
    assert sim.body_measure_stats(reset=True) == st and sim.body_measure_stats() == dict(calls=0, seconds=0.0)
    # an upload, a measurement again: the new state's bodies
    sim.upload_state(pos[::-1].copy(), vel)
    got = sim.measure_bodies(0.025)
    want, bodies, _ = restate(sim, 0.025)
    assert_same_bodies(got, want, "after a second upload")
    assert_same_moments(got, bodies, "after a second upload")
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    M.assert_same_rows(sim.measure_bodies(0.025)["moments"], got["moments"], "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_measure_bodies(h, None) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_measure_bodies(h, None) == SPH_ESTATE
    sim.phase("readback")
    got = sim.measure_bodies(0.025)
    assert_same_moments(got, restate(sim, 0.025)[1], "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_measure_bodies(other._h, None) == SPH_ESTATE, kw
        other.close()
    # no particles: SPH_OK and no bodies
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    got = empty.measure_bodies()
    assert got["moments"].shape == (0,) and got["moments"].dtype == M.ROW_DTYPE and got["num_bodies"] == 0
    assert got["size_hist"].tolist() == [0] * 32 and got["labels"].shape == (0,) and got["table"].shape == (0, 8)
    assert len(empty.body_values(got["moments"])) == 0
    empty.close()


def bodies_host(sim):
    """what sph_bodies_host serves now, as label_bodies() returns it"""
    lab, tab, n, k, big = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_int(0), C.c_uint32(0)
    assert sim._L.sph_bodies_host(sim._h, C.byref(lab), C.byref(n), C.byref(tab), C.byref(k), C.byref(big)) == 0
    as_array = lambda p, shape: np.array(np.ctypeslib.as_array(p, shape=shape), copy=True)
    return dict(labels=as_array(lab, (n.value,)), table=as_array(tab, (k.value, 8)), num_bodies=k.value, largest=big.value)


# ---- the command-line front end ----

def test_cli_free_body_table(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_BODIES_PLAIN", "SPH_FREE_BODIES"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_BODY_TABLE": "1", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["body_table_%04d.jsonl" % f for f in range(2)] + ["frame_%04d.ppm" % f for f in range(2)]
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    for f in range(2):
        sim.simulate()
        got = sim.measure_bodies(float(sim.settings.h))
        values = sim.body_values(got["moments"])
        lines = [json.loads(l) for l in open(tmp_path / ("body_table_%04d.jsonl" % f))]
        assert len(lines) == got["num_bodies"] >= 1
        for line, row, v in zip(lines, got["moments"], values):
            assert set(line) == {"label", "count"} | set(M.VALUE_FIELDS)
            assert (line["label"], line["count"]) == (int(row["label"]), int(row["count"]))
            for name in M.VALUE_FIELDS:
                assert line[name] == v[name].tolist(), (f, name, line[name], v[name])
    sim.close()
    # a bad value prints one line and writes no table files
    for value in ("yes", "0", "1.5"):
        bad = tmp_path / ("bad" + value)
        bad.mkdir()
        env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_BODY_TABLE": value, "SPH_FREE_FRAMES_DIR": str(bad)})
        r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        said = [l for l in r.stderr.splitlines() if "SPH_FREE_BODY_TABLE" in l]
        assert r.returncode == 0 and said == [l for l in said if ("SPH_FREE_BODY_TABLE=" + value) in l] and len(said) == 1, r.stderr
        assert sorted(os.listdir(bad)) == ["frame_0000.ppm"], value
