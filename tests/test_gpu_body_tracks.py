"""Body tracks on the GPU (sph_track_bodies): the default path (the fold, the sorted partial
edges, integer atomics) and the check path (every particle id a partial, run lengths, one thread per body) against the
restatement (tests/body_tracks_restatement.py) fed with the labels of the two calls, byte for byte; the sums the edges
must keep; the labelling and the moments of the same state; the call's absence from the run's results; the rules; the
command-line front end."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import body_states as BS
import body_tracks_restatement as T
import grid_states as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
U = np.uint32
SPH_EINVAL, SPH_ESTATE, SPH_ENOMEM = -1, -4, -3


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def settings_of(n, h=0.1, cells=100):
    return sph.default_settings(n, True) if (h, cells) == (0.1, 100) else G.settings_for(n, h, cells, factory=sph.default_settings)


def jitter(pos, sigma, seed=7):
    return (pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)).astype(F)


def assert_sums(got, n, what):
    """what the edges must keep, and the flags' agreement with the per-body rows"""
    e, t, p, s = got["edges"], got["tracks"], got["previous"], got["summary"]
    assert (s["bodies"], s["previous_bodies"], s["edges"]) == (len(t), len(p), len(e)) and len(t) == got["num_bodies"], what
    assert s["continued"] + s["born"] == s["bodies"] and s["continued"] + s["ended"] == s["previous_bodies"], what
    assert s["merges"] == int((t["parents"] >= 2).sum()) and s["splits"] == int((p["children"] >= 2).sum()), what
    if len(p) == 0:
        assert len(e) == 0 and (t["parents"] == 0).all() and (t["main_parent"] == T.NONE).all() and (t["flags"] == T.TRACK_BORN).all(), what
        return
    assert int(e["count"].sum()) == n, what
    assert np.array_equal(np.bincount(e["cur"], weights=e["count"], minlength=len(t)).astype(U), got["table"][:, 1]), what
    assert np.array_equal(np.bincount(e["prev"], weights=e["count"], minlength=len(p)).astype(U), p["count"]), what
    order = np.lexsort((e["prev"], e["cur"]))
    assert np.array_equal(order, np.arange(len(e))), f"{what}: the edges are not in (cur, prev) order"
    mp = (e["flags"] & T.EDGE_MAIN_PARENT) != 0
    mc = (e["flags"] & T.EDGE_MAIN_CHILD) != 0
    assert int(mp.sum()) == len(t) and int(mc.sum()) == len(p), what
    assert np.array_equal(e["prev"][mp], t["main_parent"]) and np.array_equal(e["count"][mp], t["main_overlap"]), what
    by_prev = np.argsort(e["prev"][mc], kind="stable")
    assert np.array_equal(e["cur"][mc][by_prev], p["main_child"]) and np.array_equal(e["count"][mc][by_prev], p["main_overlap"]), what


class Pair:
    """Two simulators of the same state, one tracked on the default path and one on the check path, and the
    restatement's tracker beside them: every call is held to it byte for byte on both."""

    def __init__(self, pos, vel=None, h=0.1, cells=100, monkeypatch=None, **kw):
        self.mp = monkeypatch
        self.n = len(pos)
        self.sims = [sph.Simulator(settings_of(len(pos), h, cells), **kw) for _ in range(2)]
        self.tracker = T.Tracker()
        self.upload(pos, vel)

    def upload(self, pos, vel=None):
        for s in self.sims:
            s.upload_state(pos, np.zeros_like(pos) if vel is None else vel)

    def simulate(self, steps):
        for s in self.sims:
            for _ in range(steps):
                s.simulate()

    def reset(self):
        for s in self.sims:
            s.track_reset()
        self.tracker.reset()

    def call(self, what, link=0.0, pin=False, **kw):
        """-> (the default path's result, the restatement's)"""
        self.mp.setenv("SPH_BODIES_PLAIN", "0")
        got = self.sims[0].track_bodies(link, **kw)
        self.mp.setenv("SPH_BODIES_PLAIN", "1")
        plain = self.sims[1].track_bodies(link, **kw)
        self.mp.setenv("SPH_BODIES_PLAIN", "0")
        want = self.tracker.call(got["labels"])
        T.assert_same(got, want, what + ", default path")
        assert np.array_equal(plain["labels"], got["labels"]) and np.array_equal(plain["table"], got["table"]), what
        T.assert_same(plain, want, what + ", check path")
        assert np.array_equal(got["table"][:, 0], want["labels"]) and np.array_equal(got["table"][:, 1], want["counts"]), what
        assert_sums(got, self.n, what)
        if pin:  # the labelling is label_bodies's
            alone = self.sims[0].label_bodies(link)
            for k in ("labels", "table"):
                assert np.array_equal(alone[k], got[k]), f"{what}: {k} against label_bodies"
            assert (alone["num_bodies"], alone["largest"]) == (got["num_bodies"], got["largest"]), what
        return got, want

    def close(self):
        for s in self.sims:
            s.close()


# ---- the shared states, both paths, every sweep ----

@pytest.mark.parametrize("sweep", ["list", "lds", "direct"])
@pytest.mark.parametrize("name,link,then", [("uniform4096", 0.06, "jitter"), ("uniform4096", 0.08, "jitter"),
                                            ("dense4096", 0.025, "steps"), ("random4096", 0.08, "steps")])
def test_tracks_are_the_restatement_on_both_paths_and_every_sweep(name, link, then, sweep, monkeypatch):
    pos, vel = BS.big(name)
    pair = Pair(pos, vel, monkeypatch=monkeypatch, sweep=sweep)
    what = f"{name}, link {link}, sweep {sweep}"
    first, _ = pair.call(what + ", first call", link)
    assert first["summary"]["born"] == first["num_bodies"] and first["summary"]["sequence"] == 1
    if then == "jitter":
        pair.upload(jitter(pos, 0.02))
    else:
        pair.simulate(5)
    got, want = pair.call(what + ", second call", link, pin=True)
    s = got["summary"]
    assert s["previous_bodies"] == first["num_bodies"] and s["sequence"] == 2
    if (name, link) == ("uniform4096", 0.06):  # (the events tests/test_body_tracks_cpu.py found in this pair)
        assert s["merges"] >= 100 and s["splits"] >= 100 and want["parent_ties"] >= 50 and want["child_ties"] >= 50
        assert got["tracks"]["parents"].max() >= 5
    if (name, link) == ("uniform4096", 0.08):
        assert got["tracks"]["parents"].max() >= 20
    pair.close()


def test_a_body_of_a_thousand_parents(monkeypatch):
    pos, vel = BS.big("dense4096")
    pair = Pair(pos, vel, monkeypatch=monkeypatch)
    pair.call("dense4096", 0.025)
    pair.upload(jitter(pos, 0.01))
    got, _ = pair.call("dense4096 jittered", 0.025)
    assert got["tracks"]["parents"].max() > 1000
    pair.close()


def test_a_sequence_of_four_calls(monkeypatch):
    pos, vel = BS.big("uniform4096")
    pair = Pair(pos, vel, monkeypatch=monkeypatch)
    a, _ = pair.call("upload", 0.06)
    pair.upload(jitter(pos, 0.02))
    b, _ = pair.call("jitter", 0.06)
    pair.simulate(3)
    c, _ = pair.call("3 steps", 0.06)
    pair.upload(pos)
    d, _ = pair.call("jitter back", 0.06)
    assert np.array_equal(d["labels"], a["labels"])
    results = [a, b, c, d]
    assert [r["summary"]["sequence"] for r in results] == [1, 2, 3, 4]
    nxt = [r["summary"]["next_track"] for r in results]
    assert nxt[0] == a["num_bodies"] and all(nxt[k + 1] == nxt[k] + results[k + 1]["summary"]["born"] for k in range(3))
    # tracks persist: a continued track is its main parent's, a born one is new, and some last through all four calls
    assert len(set.intersection(*[set(r["tracks"]["track"].tolist()) for r in results])) > 100
    for before, after in zip(results, results[1:]):
        t = after["tracks"]
        kept = (t["flags"] & T.TRACK_CONTINUES) != 0
        assert kept.sum() > 100 and np.array_equal(t["track"][kept], before["tracks"]["track"][t["main_parent"][kept]])
        assert len(set(t["track"].tolist())) == len(t), "a track inherited twice"
        assert (t["track"][~kept] >= before["summary"]["next_track"]).all()
    pair.close()


# ---- small and awkward sizes ----

def moved(pos, row, to=(8.05, 8.05, 8.05)):
    out = pos.copy()
    out[row] = to
    return out


def test_one_particle(monkeypatch):
    pair = Pair(np.array([[5.0625, 5.125, 5.25]], F), monkeypatch=monkeypatch)
    a, _ = pair.call("n = 1")
    assert a["tracks"].tolist() == [(0, 0, T.NONE, 0, T.TRACK_BORN)]
    b, _ = pair.call("n = 1 again")
    assert b["tracks"].tolist() == [(0, 1, 0, 1, T.TRACK_CONTINUES)] and b["edges"].tolist() == [(0, 0, 1, 3)]
    assert b["previous"].tolist() == [(0, 0, 1, 1, 0, 1, T.FATE_CONTINUES)]
    pair.close()


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_tails(n, monkeypatch):
    pos = BS.cluster(n, n)
    pair = Pair(pos, monkeypatch=monkeypatch)
    pair.call(f"n = {n}", 0.05)
    pair.upload(jitter(pos, 0.02))
    got, _ = pair.call(f"n = {n} jittered", 0.05)
    assert got["summary"]["edges"] > 1
    pair.close()


def test_a_giant_across_blocks_and_a_last_block_of_one_row(monkeypatch):
    pos = BS.one_cell(2049, 5, (50, 50, 50))
    pair = Pair(pos, monkeypatch=monkeypatch)
    a, _ = pair.call("2049 of one body")
    assert a["table"][:, 1].tolist() == [2049]
    pair.upload(moved(pos, 1000))
    b, _ = pair.call("one particle moved away")
    assert sorted(b["table"][:, 1].tolist()) == [1, 2048] and b["summary"]["splits"] == 1 and b["summary"]["born"] == 1
    assert int(b["tracks"]["track"][np.argmax(b["table"][:, 1])]) == 0
    pair.close()


def test_one_cell_and_grids_of_a_few_cells(monkeypatch):
    pos = BS.one_cell(1500, 5, (50, 50, 50))
    pair = Pair(pos, monkeypatch=monkeypatch)
    pair.call("1500 in one cell")
    pair.upload(moved(pos, 3))
    got, _ = pair.call("1500 in one cell, one moved away")
    assert sorted(got["table"][:, 1].tolist()) == [1, 1499]
    pair.close()
    for name in ("D1", "D2", "D3"):
        pos, vel, g = G.grid_state(name)
        top = np.nextafter(G.box_of(g["h"], g["cells"]), F(0))
        k = min(len(pos) // 4, 24)
        for i in range(k):  # rows on the wall planes
            pos[i, i % 3] = F(0) if (i // 3) % 2 == 0 else top
        pos[k], pos[k + 1] = (F(0), F(0), F(0)), (top, top, top)
        G.assert_inside(pos, g["h"], g["cells"], name)
        pair = Pair(pos, vel, g["h"], g["cells"], monkeypatch=monkeypatch)
        link = 0.5 * float(g["h"])
        pair.call(name, link)
        pair.simulate(2)
        pair.call(name + " after 2 steps", link)
        pair.call(name + " at link h", 0.0)
        pair.close()


def test_singletons_in_both_labellings_make_n_partials(monkeypatch):
    k = np.arange(8)
    pos = (F(1) + F(0.25) * np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)).astype(F)
    pos = pos[np.random.default_rng(3).permutation(len(pos))]
    n = len(pos)
    pair = Pair(pos, monkeypatch=monkeypatch)
    a, _ = pair.call("a lattice of singletons")
    assert a["num_bodies"] == n
    pair.sims[0].body_track_stats(reset=True)
    b, _ = pair.call("a lattice of singletons again")
    assert b["summary"]["edges"] == n and b["summary"]["continued"] == n and np.array_equal(b["tracks"]["track"], a["tracks"]["track"])
    st = pair.sims[0].body_track_stats()
    assert (st["calls"], st["partials"], st["edges"]) == (1, n, n), st
    pair.close()


def test_one_body_in_both_labellings_makes_one_edge_of_a_partial_per_block(monkeypatch):
    pos = BS.one_cell(4096, 9, (50, 50, 50))
    pair = Pair(pos, monkeypatch=monkeypatch)
    pair.call("4096 of one body")
    for s in pair.sims:
        s.body_track_stats(reset=True)
    got, _ = pair.call("4096 of one body again")
    assert got["edges"].tolist() == [(0, 0, 4096, 3)]
    st = [s.body_track_stats() for s in pair.sims]
    assert 1 <= st[0]["partials"] <= 2, "the 2,048-row blocks of the default path"
    assert st[1]["partials"] == 4096, "the check path: every particle id"
    pair.close()


# ---- hand answers on the device ----

def test_blobs_and_the_cut_chain(monkeypatch):
    pos, order = BS.blobs()
    bridge = int(np.flatnonzero(order == 400)[0])
    pair = Pair(pos, monkeypatch=monkeypatch)
    a, _ = pair.call("blobs with the bridge")
    assert a["table"][:, 1].tolist() == [401]
    pair.upload(moved(pos, bridge))
    b, wb = pair.call("the bridge moved away")
    assert sorted(b["table"][:, 1].tolist()) == [1, 200, 200] and wb["child_ties"] == 1
    halves = np.flatnonzero(b["table"][:, 1] == 200)
    assert b["previous"]["main_child"].tolist() == [halves[0]], "the tie goes to the smaller label"
    assert b["tracks"]["track"][halves[0]] == 0 and sorted(b["tracks"]["track"].tolist()) == [0, 1, 2]
    assert {k: b["summary"][k] for k in ("continued", "born", "ended", "merges", "splits")} == dict(continued=1, born=2, ended=0, merges=0, splits=1)
    pair.upload(pos)
    c, wc = pair.call("the bridge back")
    assert c["tracks"].tolist() == [(0, 3, halves[0], 200, T.TRACK_CONTINUES | T.TRACK_MERGED)] and wc["parent_ties"] == 1
    assert {k: c["summary"][k] for k in ("continued", "born", "ended", "merges", "splits")} == dict(continued=1, born=0, ended=2, merges=1, splits=0)
    assert c["summary"]["next_track"] == 3
    pair.close()
    pos, where = BS.chain()
    pair = Pair(pos, monkeypatch=monkeypatch)
    pair.call("the chain")
    pair.upload(moved(pos, int(np.flatnonzero(where == 128)[0])))
    d, _ = pair.call("the chain cut in the middle")
    assert sorted(d["table"][:, 1].tolist()) == [1, 128, 128] and d["summary"]["splits"] == 1 and d["summary"]["born"] == 2
    assert d["tracks"]["track"][np.flatnonzero(d["table"][:, 1] == 128)[0]] == 0
    pair.close()


def test_different_links_between_calls(monkeypatch):
    pos, vel = BS.big("uniform4096")
    pair = Pair(pos, vel, monkeypatch=monkeypatch)
    pair.call("fine", 0.025)
    up, _ = pair.call("fine, then coarse", 0.05)
    assert up["summary"]["splits"] == 0 and up["summary"]["merges"] >= 100 and up["summary"]["born"] == 0
    down, _ = pair.call("coarse, then fine", 0.025)
    assert down["summary"]["merges"] == 0 and down["summary"]["splits"] == up["summary"]["merges"] and down["summary"]["ended"] == 0
    pair.close()


def test_with_moments(monkeypatch):
    pos, vel = BS.big("random4096")
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_BODIES_PLAIN", plain)
        sim = sph.Simulator(settings_of(len(pos)))
        sim.upload_state(pos, vel)
        sim.simulate()
        sim.track_bodies(0.08)
        sim.simulate()
        sim.body_measure_stats(reset=True)
        got = sim.track_bodies(0.08, moments=True)
        assert sim.body_measure_stats()["calls"] == 1
        want = sim.measure_bodies(0.08)
        for k in ("labels", "table", "moments", "size_hist"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (plain, k)
        assert len(got["moments"]) == len(got["tracks"]) > 1 and np.array_equal(got["moments"]["label"], got["table"][:, 0])
        sim.close()
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")


# ---- no footprint ----

def run(timed, tracking, steps=10):
    pos, vel = BS.big("dense4096")
    sim = sph.Simulator(settings_of(len(pos)))
    sim.upload_state(pos, vel)
    times = sph.Times()
    seen = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if tracking:
            seen.append(sim.track_bodies(0.025)["summary"])
    st = sim.download_state()
    st["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return st, seen


@pytest.mark.parametrize("timed", [False, True])
def test_a_tracking_between_every_two_steps_leaves_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    with_, seen = run(timed, True)
    without, _ = run(timed, False)
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(words(with_[k]), words(without[k])), f"timed={timed}: {k} differs after 10 steps"
    assert [s["sequence"] for s in seen] == list(range(1, 11)) and min(s["bodies"] for s in seen) > 1


# ---- state rules, options, stats ----

def test_state_rules_error_codes_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_BODIES_PLAIN", "0")
    pos, vel = BS.big("uniform4096")
    sim = sph.Simulator(settings_of(len(pos)))
    L, h = sim._L, sim._h
    host = lambda: L.sph_body_tracks_host(h, None, None, None, None, None, None, None)
    opt = lambda link, cap=0, flags=0, size=C.sizeof(_lib.SphBodyTrackOptions): C.byref(_lib.SphBodyTrackOptions(size, link, cap, flags))
    # before any state, and the results before the first call
    assert L.sph_track_bodies(h, None) == SPH_ESTATE and host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    sim.label_bodies()
    assert host() == SPH_ESTATE, "a labelling alone leaves no tracks"
    # the options
    assert L.sph_track_bodies(h, opt(0.05, size=0)) == SPH_EINVAL
    for bad in (float("nan"), float("inf"), -0.05, float(np.nextafter(F(sim.settings.h), F(1)))):
        assert L.sph_track_bodies(h, opt(bad)) == SPH_EINVAL, bad
    for bits in (2, 4, 0x80000000, 3):
        assert L.sph_track_bodies(h, opt(0.05, flags=bits)) == SPH_EINVAL, bits
    assert host() == SPH_ESTATE
    assert L.sph_track_bodies(h, None) == 0 and host() == 0   # NULL: link = h, no cap, no flags
    sim.track_reset()
    assert host() == SPH_ESTATE, "a reset leaves no results"
    # a refusal by max_edges leaves the reference and next_track alone
    t = T.Tracker()
    sim.body_track_stats(reset=True)
    a = sim.track_bodies(0.06)
    T.assert_same(a, t.call(a["labels"]), "first call after the reset")
    sim.upload_state(jitter(pos, 0.02), vel)
    probe = T.join(t.labels, sim.label_bodies(0.06)["labels"], t.tracks, t.next_track)
    edges = probe["summary"]["edges"]
    assert L.sph_track_bodies(h, opt(0.06, edges - 1)) == SPH_ENOMEM
    msg = L.sph_last_error(h).decode()
    assert str(edges) in msg and str(edges - 1) in msg, msg
    assert host() == SPH_ESTATE
    assert np.array_equal(sim_labels(sim), probe_labels(sim, 0.06)), "the refused call's labelling stands"
    assert t.call(sim_labels(sim), max_edges=edges - 1) is None
    b = sim.track_bodies(0.06, max_edges=edges)        # at the count it passes: as if the refused call had never happened
    T.assert_same(b, t.call(b["labels"]), "after a refused call")
    assert b["summary"]["sequence"] == 2 and b["summary"]["edges"] == edges
    # the stats: three calls queued launches, the refused one added what it counted; their reset
    st = sim.body_track_stats()
    assert st["calls"] == 3 and st["edges"] == 2 * edges and st["partials"] >= 2 * edges and 0.0 < st["seconds"] < 1.0, st
    assert sim.body_track_stats(reset=True) == st and sim.body_track_stats() == dict(calls=0, partials=0, edges=0, seconds=0.0)
    # the reset: no previous bodies, tracks from 0
    sim.track_reset()
    t.reset()
    c = sim.track_bodies(0.06)
    T.assert_same(c, t.call(c["labels"]), "after sph_track_reset")
    assert c["summary"]["sequence"] == 1 and c["summary"]["previous_bodies"] == 0 and c["tracks"]["track"].tolist() == list(range(c["num_bodies"]))
    # an open phase-split step is SPH_ESTATE; the grid phase done by hand is used as it is
    sim.phase("grid")
    d = sim.track_bodies(0.06)
    T.assert_same(d, t.call(d["labels"]), "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_track_bodies(h, None) == SPH_ESTATE
    sim.phase("force")
    sim.phase("readback")
    e = sim.track_bodies(0.06)
    T.assert_same(e, t.call(e["labels"]), "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_track_bodies(other._h, None) == SPH_ESTATE, kw
        assert other._L.sph_body_tracks_host(other._h, None, None, None, None, None, None, None) == SPH_ESTATE, kw
        other.close()
    # no particles: SPH_OK and nothing
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    got = empty.track_bodies(moments=True)
    assert got["tracks"].shape == got["previous"].shape == got["edges"].shape == (0,) and got["num_bodies"] == 0
    assert got["tracks"].dtype == T.TRACK_DTYPE and got["previous"].dtype == T.FATE_DTYPE and got["edges"].dtype == T.EDGE_DTYPE
    assert {k: v for k, v in got["summary"].items() if k != "sequence"} == {k: 0 for k in T.SUMMARY if k != "sequence"}
    assert got["moments"].shape == (0,) and got["size_hist"].tolist() == [0] * 32
    empty.close()


def sim_labels(sim):
    """the labels sph_bodies_host serves now"""
    lab, n = C.POINTER(C.c_uint32)(), C.c_int(0)
    assert sim._L.sph_bodies_host(sim._h, C.byref(lab), C.byref(n), None, None, None) == 0
    return np.array(np.ctypeslib.as_array(lab, shape=(n.value,)), copy=True)


def probe_labels(sim, link):
    return sim.label_bodies(link)["labels"]


# ---- the command-line front end ----

def test_cli_free_body_tracks(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_BODIES_PLAIN", "SPH_FREE_BODIES", "SPH_FREE_BODY_TABLE"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "3", "SPH_FREE_BODY_TRACKS": "0.5", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["body_tracks_%04d.jsonl" % f for f in range(3)] + ["frame_%04d.ppm" % f for f in range(3)]
    said = [l.split() for l in r.stderr.splitlines() if l.startswith("tracks ")]
    sim = sph.Simulator(sph.default_settings(4096, True))
    sim.setup()
    for f in range(3):
        sim.simulate()
        got = sim.track_bodies(0.5 * float(sim.settings.h))
        s, t, p, e = got["summary"], got["tracks"], got["previous"], got["edges"]
        lines = [json.loads(l) for l in open(tmp_path / ("body_tracks_%04d.jsonl" % f))]
        assert lines[0] == dict(frame=f, **s)
        assert len(lines) == 1 + len(t) + len(e) and len(t) > 1 and (f == 0 or len(e) >= len(t))
        for b, line in enumerate(lines[1:1 + len(t)]):
            parent = int(p["label"][t["main_parent"][b]]) if t["parents"][b] else None
            assert line == dict(label=int(got["table"][b, 0]), count=int(got["table"][b, 1]), track=int(t["track"][b]), parents=int(t["parents"][b]),
                                main_parent=parent, main_overlap=int(t["main_overlap"][b]), continues=bool(t["flags"][b] & T.TRACK_CONTINUES)), (f, b)
        for k, line in enumerate(lines[1 + len(t):]):
            assert line == dict(prev=int(p["label"][e["prev"][k]]), cur=int(got["table"][e["cur"][k], 0]), count=int(e["count"][k]),
                                main_parent=bool(e["flags"][k] & T.EDGE_MAIN_PARENT), main_child=bool(e["flags"][k] & T.EDGE_MAIN_CHILD)), (f, k)
        assert said[f] == ["tracks"] + [str(x) for x in (f, s["bodies"], s["continued"], s["born"], s["ended"], s["merges"], s["splits"])]
    sim.close()
    assert len(said) == 3
    # a bad value prints one line and writes no track files
    for value in ("yes", "0", "1.5"):
        bad = tmp_path / ("bad" + value)
        bad.mkdir()
        env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_BODY_TRACKS": value, "SPH_FREE_FRAMES_DIR": str(bad)})
        r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        said = [l for l in r.stderr.splitlines() if "SPH_FREE_BODY_TRACKS" in l]
        assert r.returncode == 0 and said == [l for l in said if ("SPH_FREE_BODY_TRACKS=" + value) in l] and len(said) == 1, r.stderr
        assert sorted(os.listdir(bad)) == ["frame_0000.ppm"], value
