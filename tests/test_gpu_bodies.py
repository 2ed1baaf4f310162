"""The bodies on the GPU (sph_label_bodies): the union-find of the default path and the label
propagation of the check path against the numpy restatement (tests/bodies_restatement.py) fed by sph_download_grid +
sph_download_state, what the call counted, the derived fields' neighbour counts, and the call's absence from the run's
results.  Every comparison is of 32-bit words; gave_up is 0 everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import body_states as BS
import grid_states as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
U = np.uint32
SPH_EINVAL, SPH_ESTATE = -1, -4
KEYS = ("labels", "table", "num_bodies", "largest")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bodies(got, want, what):
    assert got["num_bodies"] == want["num_bodies"], f"{what}: {got['num_bodies']} bodies, not {want['num_bodies']}"
    for k in ("labels", "table"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype == U, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} words of {k} differ, first at {np.argwhere(bad)[0]}"
    assert got["largest"] == want["largest"], f"{what}: largest {got['largest']}, not {want['largest']}"


def simulator(pos, vel=None, h=0.1, cells=100, **kw):
    vel = np.zeros_like(pos) if vel is None else vel
    s = sph.default_settings(len(pos), True) if (h, cells) == (0.1, 100) else G.settings_for(len(pos), h, cells, factory=sph.default_settings)
    sim = sph.Simulator(s, **kw)
    sim.upload_state(pos, vel)
    return sim


def restate(sim, link):
    """the restatement over the grid the sweep walked (call after label_bodies())"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    s = sim.settings
    return BR.bodies(st["pos"][ids], ids, g["cells"], s.h, int(s.numCellsPerDim), link)


def assert_sound(got, n):
    t = got["table"]
    assert int(t[:, 1].sum(dtype=np.int64)) == n and (np.diff(t[:, 0].astype(np.int64)) > 0).all()
    assert np.array_equal(got["labels"][t[:, 0]], t[:, 0])


def both_paths(sim, monkeypatch, what, link=0.0):
    """label_bodies() on the default and on the check path, both equal to the restatement and counted right
    -> (bodies, the restatement, the check path's rounds)"""
    n = sim.settings.numParticles
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    sim.body_stats(reset=True)
    got = sim.label_bodies(link)
    st = sim.body_stats(reset=True)
    want = restate(sim, link)
    assert st["gave_up"] == 0
    assert_same_bodies(got, want, what + ", default path")
    assert_sound(got, n)
    assert (st["calls"], st["links"], st["unions"], st["rounds"]) == (1, want["links"], n - want["num_bodies"], 0), (what, st)
    assert 0.0 < st["seconds"] < 1.0, st
    monkeypatch.setenv("SPH_BODIES_PLAIN", "1")
    plain = sim.label_bodies(link)
    ps = sim.body_stats(reset=True)
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    assert_same_bodies(plain, want, what + ", check path")
    assert (ps["calls"], ps["links"], ps["unions"], ps["gave_up"]) == (1, want["links"], n - want["num_bodies"], 0), (what, ps)
    assert 1 <= ps["rounds"] <= n, (what, ps)
    return got, want, ps["rounds"]


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("random4096", 0), ("uniform4096", 0),
                                        ("dense4096", 5), ("random4096", 5), ("uniform4096", 5)])
def test_labels_table_and_counters_are_the_restatement_on_both_paths(name, steps, monkeypatch):
    pos, vel = BS.big(name)
    links = [l for s, l in BS.BIG if s == name]
    sim = simulator(pos, vel)
    for _ in range(steps):
        sim.simulate()
    results = {}
    for link in links:
        results[link], want, _ = both_paths(sim, monkeypatch, f"{name} + {steps} steps, link {link}", link)
    if steps == 0:
        several = {"dense4096": 0.025, "random4096": 0.0, "uniform4096": 0.08}[name]
        assert results[several]["num_bodies"] > 1
    # the cross-check with sph_derive on the device: links, and who is alone
    d = sim.derive()["neighbours"].astype(np.int64)
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    sim.body_stats(reset=True)
    got = sim.label_bodies(0.0)
    assert 2 * sim.body_stats()["links"] == int(d.sum()) - len(pos)
    alone = np.zeros(len(pos), bool)
    alone[got["table"][got["table"][:, 1] == 1, 0]] = True
    assert np.array_equal(alone, d == 1)
    sim.close()
    # the sweeps that keep a sorted position stream of their own read the same words
    for sweep in ("lds", "direct"):
        other = simulator(pos, vel, sweep=sweep)
        for _ in range(steps):
            other.simulate()
        for link in links:
            assert_same_bodies(other.label_bodies(link), results[link], f"{name} + {steps} steps, link {link}, sweep {sweep}")
        assert other.body_stats()["gave_up"] == 0
        other.close()


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


def test_one_particle_and_the_pairs_at_the_link_length(monkeypatch):
    sim = simulator(np.array([[5.05, 5.05, 5.05]], F))
    got, _, rounds = both_paths(sim, monkeypatch, "n = 1")
    p = np.array([5.05, 5.05, 5.05], F).view(U)
    assert got["labels"].tolist() == [0] and got["table"].tolist() == [[0, 1, *p, *p]] and got["largest"] == 0 and rounds == 1
    sim.close()
    pos, (near, far), r2 = BS.boundary_pairs()
    assert near == r2 and far > r2
    sim = simulator(pos)
    got, _, _ = both_paths(sim, monkeypatch, "boundary pairs")
    assert got["labels"].tolist() == [0, 0, 2, 3] and got["table"][:, :2].tolist() == [[0, 2], [2, 1], [3, 1]]
    sim.close()


def test_wave_tails_and_grids_of_a_few_cells(monkeypatch):
    for n in (63, 64, 65, 129):
        sim = simulator(BS.cluster(n, n))
        got, _, _ = both_paths(sim, monkeypatch, f"n = {n}")
        assert got["table"][:, 1].max() > 1
        sim.close()
    for name in ("D1", "D2", "D3"):
        pos, vel, g = on_the_walls(name)
        sim = simulator(pos, vel, g["h"], g["cells"])
        for link in (0.0, 0.5 * float(g["h"])):
            both_paths(sim, monkeypatch, f"{name}, link {link}", link)
        sim.close()


def test_every_merge_on_one_root(monkeypatch):
    sim = simulator(BS.one_cell(1500, 5, (50, 50, 50)))
    got, _, _ = both_paths(sim, monkeypatch, "1500 in one cell")
    assert got["num_bodies"] == 1 and got["table"][0, :2].tolist() == [0, 1500]
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    sim.body_stats(reset=True)
    sim.label_bodies()
    assert sim.body_stats()["unions"] == 1499
    sim.close()


def test_long_bodies_chain_lattice_and_bridge(monkeypatch):
    pos, where = BS.chain()
    sim = simulator(pos)
    got, _, rounds = both_paths(sim, monkeypatch, "chain of 257")
    assert got["num_bodies"] == 1 and (got["labels"] == 0).all() and rounds > 1
    sim.close()
    pos, where = BS.chain(without_middle=True)
    sim = simulator(pos)
    got, _, _ = both_paths(sim, monkeypatch, "chain without its middle")
    head = where < 128
    assert got["table"][:, :2].tolist() == [[0, 128], [int(np.flatnonzero(head if not head[0] else ~head).min()), 128]]
    sim.close()
    # the lattice of `-i grid`: one body whose graph is tens of links across
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    got, _, rounds = both_paths(sim, monkeypatch, "-i grid")
    assert got["num_bodies"] == 1 and 1 < rounds <= 4096
    sim.close()
    for bridge, bodies in ((True, 1), (False, 2)):
        pos, order = BS.blobs(bridge)
        sim = simulator(pos)
        got, _, _ = both_paths(sim, monkeypatch, f"blobs, bridge {bridge}")
        assert got["num_bodies"] == bodies and got["table"][:, 1].tolist() == ([401] if bridge else [200, 200])
        sim.close()


def run(timed, labelling, steps=10):
    pos, vel = BS.big("dense4096")
    sim = simulator(pos, vel)
    times = sph.Times()
    counts = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if labelling:
            counts.append(sim.label_bodies(0.025)["num_bodies"])
    st = sim.download_state()
    st["host"] = np.array(sim.getPosition(), copy=True)
    gave_up = sim.body_stats()["gave_up"]
    sim.close()
    return st, counts, gave_up


@pytest.mark.parametrize("timed", [False, True])
def test_a_labelling_between_every_two_steps_leaves_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    with_, counts, gave_up = run(timed, True)
    without, _, _ = run(timed, False)
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(words(with_[k]), words(without[k])), f"timed={timed}: {k} differs after 10 steps"
    assert len(counts) == 10 and min(counts) > 1 and gave_up == 0


def test_state_rules_error_codes_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    pos, vel = BS.big("dense4096")
    sim = sph.Simulator(sph.default_settings(len(pos), True))
    L, h = sim._L, sim._h
    outs = (C.POINTER(C.c_uint32)(), C.c_int(-1), C.POINTER(C.c_uint32)(), C.c_int(-1), C.c_uint32(7))
    host = lambda: L.sph_bodies_host(h, *[C.byref(o) for o in outs])
    opt = lambda link, size=C.sizeof(_lib.SphBodyOptions): C.byref(_lib.SphBodyOptions(size, link))
    # before any state, and the results before the first labelling
    assert L.sph_label_bodies(h, None) == SPH_ESTATE
    assert host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    assert host() == SPH_ESTATE
    # the options
    assert L.sph_label_bodies(h, opt(0.05, 0)) == SPH_EINVAL
    for bad in (float("nan"), float("inf"), -0.05, float(np.nextafter(F(sim.settings.h), F(1)))):
        assert L.sph_label_bodies(h, opt(bad)) == SPH_EINVAL, bad
    assert host() == SPH_ESTATE
    assert L.sph_label_bodies(h, None) == 0          # NULL: link = h
    assert host() == 0 and outs[1].value == len(pos) and outs[3].value == 1 and outs[4].value == 0
    assert L.sph_bodies_host(h, None, None, None, None, None) == 0
    first = sim.label_bodies(0.0)
    assert_same_bodies(sim.label_bodies(float(sim.settings.h)), first, "link = h against link = 0")
    # an upload, a labelling again: the new state's bodies
    sim.upload_state(pos[::-1].copy(), vel)
    sim.body_stats(reset=True)
    second = sim.label_bodies(0.025)
    assert_same_bodies(second, restate(sim, 0.025), "after a second upload")
    assert second["num_bodies"] > 1
    third = sim.label_bodies(0.025)
    assert_same_bodies(third, second, "again")
    # the stats sum over calls and reset
    st = sim.body_stats()
    n = len(pos)
    assert st["calls"] == 2 and st["unions"] == 2 * (n - second["num_bodies"]) and st["links"] % 2 == 0 and st["links"] > 0
    assert st["seconds"] > 0 and st["rounds"] == 0 and st["gave_up"] == 0
    assert sim.body_stats(reset=True) == st
    assert sim.body_stats() == dict(calls=0, links=0, unions=0, rounds=0, gave_up=0, seconds=0.0)
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    assert_same_bodies(sim.label_bodies(0.025), second, "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_label_bodies(h, None) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_label_bodies(h, None) == SPH_ESTATE
    sim.phase("readback")
    assert_same_bodies(sim.label_bodies(0.025), restate(sim, 0.025), "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_label_bodies(other._h, None) == SPH_ESTATE, kw
        other.close()
    # no particles: SPH_OK and no bodies
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    got = empty.label_bodies()
    assert got["labels"].shape == (0,) and got["table"].shape == (0, 8) and (got["num_bodies"], got["largest"]) == (0, 0)
    assert got["labels"].dtype == got["table"].dtype == U
    empty.close()


def read_ply(path):
    blob = open(path, "rb").read()
    head, _, body = blob.partition(b"end_header\n")
    lines = head.decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n = int(lines[2].split()[2])
    assert lines[2:] == ["element vertex %d" % n, "property float x", "property float y", "property float z",
                         "property uint label", "property uint body_count", ""]
    assert len(body) == n * 20
    return np.frombuffer(body, "<u4").reshape(n, 5)


def test_cli_free_bodies(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_BODIES_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_BODIES": "1", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bodies_%04d.ply" % f for f in range(2)] + ["frame_%04d.ppm" % f for f in range(2)]
    said = [l.split() for l in r.stderr.splitlines() if l.startswith("bodies ")]
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    for f in range(2):
        sim.simulate()
        b = sim.label_bodies(float(sim.settings.h))
        rows = read_ply(tmp_path / ("bodies_%04d.ply" % f))
        count_of = np.zeros(4096, U)
        count_of[b["table"][:, 0]] = b["table"][:, 1]
        assert np.array_equal(rows[:, :3], words(np.array(sim.getPosition(), copy=True))), f
        assert np.array_equal(rows[:, 3], b["labels"]) and np.array_equal(rows[:, 4], count_of[b["labels"]]), f
        assert said[f] == ["bodies", str(f), str(b["num_bodies"]), str(int(count_of[b["largest"]]))], said
    sim.close()
    # a bad value prints one line and writes no body files
    for value in ("yes", "0", "1.5"):
        bad = tmp_path / ("bad" + value)
        bad.mkdir()
        env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_BODIES": value, "SPH_FREE_FRAMES_DIR": str(bad)})
        r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and ("SPH_FREE_BODIES=" + value) in r.stderr and sorted(os.listdir(bad)) == ["frame_0000.ppm"], value
