"""The neighbour lists on the GPU (sph_neighbour_lists): the default and the check path
against the two numpy restatements (tests/neighbour_restatement.py) -- the ascending order against all pairs, the walk
order against the 27-cell walk over sph_download_grid --, against what the bodies, the derived fields and the step's
pair counters say about the same state, and the call's absence from the run's results.  Every comparison is of
integer words."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import body_states as BS
import grid_states as G
import neighbour_restatement as NR
import neighbour_states as NS
import test_gpu_analysis_shared as SH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SPH_EINVAL, SPH_ENOMEM, SPH_ESTATE = -1, -3, -4
SLICE = 640          # neighbours.hip's NBR_SLICE (kNbrSlice): the longest run the count and emit walks stage
SORT_SLICE = 1024    # neighbours.hip's NBR_SORT_SLICE (kSortSlice): the longest list the sort stages whole
RADII = (0.0, 0.08, 0.025)
_want = {}


def assert_same_lists(got, want, what):
    """got: neighbour_lists()'s dict; want: a restatement's (offsets, neighbours)"""
    if isinstance(want, dict):
        want = (want["offsets"], want["neighbours"])
    for k, b in zip(("offsets", "neighbours"), want):
        a = got[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} words of {k} differ, first at {np.argwhere(bad)[0]}"


def simulator(pos, vel=None, h=0.1, cells=100, **kw):
    vel = np.zeros_like(pos) if vel is None else vel
    s = sph.default_settings(len(pos), True) if (h, cells) == (0.1, 100) else G.settings_for(len(pos), h, cells, factory=sph.default_settings)
    sim = sph.Simulator(s, **kw)
    sim.upload_state(pos, vel)
    return sim


def all_pairs_of(sim, radius, key=None):
    """restatement (a) of the state the handle holds; `key`: computed once per process and shared"""
    if key is not None and (key, radius) in _want:
        return _want[key, radius]
    want = NR.all_pairs(sim.download_state()["pos"], sim.settings.h, radius)
    if key is not None:
        _want[key, radius] = want
    return want


def walk_of(sim, radius):
    """restatement (b) over the grid the sweep walked (call after neighbour_lists())"""
    g = sim.download_grid()
    ids = g["ids"].astype(np.int64)
    s = sim.settings
    return NR.walk_order(sim.download_state()["pos"][ids], ids, g["cells"], s.h, int(s.numCellsPerDim), radius)


def both_paths(sim, monkeypatch, what, radius=0.0, key=None):
    """neighbour_lists() in both orders on the default and on the check path, all four equal to the restatements
    -> (the ascending lists, the default path's stats over its two calls)"""
    want_a = all_pairs_of(sim, radius, key)
    want_b = None
    n = sim.settings.numParticles
    entries = int(want_a[0][-1])
    longest = int(np.diff(want_a[0].astype(np.int64)).max()) if n else 0
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", plain)
        sim.neighbour_stats(reset=True)
        got = sim.neighbour_lists(radius)
        walked = sim.neighbour_lists(radius, walk_order=True)
        st = sim.neighbour_stats(reset=True)
        want_b = walk_of(sim, radius) if want_b is None else want_b
        assert_same_lists(got, want_a, f"{what}, radius {radius}, plain={plain}, ascending")
        assert_same_lists(walked, want_b, f"{what}, radius {radius}, plain={plain}, walk order")
        assert (st["calls"], st["entries"], st["longest"]) == (2, 2 * entries, longest), (what, st)
        assert 0.0 < st["seconds"] < 1.0, st
        if plain == "0":
            result, stats = got, st
        else:
            assert (st["runs_staged"], st["runs_direct"]) == (0, 0), st
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    return result, stats


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("dense4096", 5), ("random4096", 0)])
def test_both_paths_and_both_orders_are_the_restatements(name, steps, monkeypatch):
    pos, vel = BS.big(name)
    sim = simulator(pos, vel)
    for _ in range(steps):
        sim.simulate()
    results = {}
    for radius in RADII:
        results[radius], st = both_paths(sim, monkeypatch, f"{name} + {steps} steps", radius, key=(name, steps))
        assert st["runs_staged"] > 0
    assert len(results[0.0]["neighbours"]) > len(results[0.025]["neighbours"])
    sim.close()
    # the sweeps that keep a sorted position stream of their own: the same words in ascending order, the walk over
    # their own grid in walk order
    for sweep in ("lds", "direct"):
        other = simulator(pos, vel, sweep=sweep)
        for _ in range(steps):
            other.simulate()
        for radius in RADII:
            assert_same_lists(other.neighbour_lists(radius), results[radius], f"{name} + {steps} steps, radius {radius}, sweep {sweep}")
            walked = other.neighbour_lists(radius, walk_order=True)
            assert_same_lists(walked, walk_of(other, radius), f"{name} + {steps} steps, radius {radius}, sweep {sweep}, walk order")
        other.close()


@pytest.mark.parametrize("name,steps", [("dense4096", 0), ("dense4096", 3), ("random4096", 0)])
def test_pins_to_the_bodies_the_derived_fields_and_the_pair_counters(name, steps, monkeypatch):
    for env in ("SPH_NEIGHBOURS_PLAIN", "SPH_BODIES_PLAIN", "SPH_DERIVE_PLAIN"):
        monkeypatch.setenv(env, "0")
    pos, vel = BS.big(name)
    sim = simulator(pos, vel, flags=_lib.SPH_FLAG_COUNT_PAIRS)
    assert sim.settings.h == F(0.1)
    for _ in range(steps):
        sim.simulate()
    n = len(pos)
    for radius in RADII:
        got = sim.neighbour_lists(radius)
        sim.body_stats(reset=True)
        sim.label_bodies(radius)
        assert len(got["neighbours"]) == int(got["offsets"][-1]) == 2 * sim.body_stats()["links"], radius
    got = sim.neighbour_lists()
    assert np.array_equal(np.diff(got["offsets"].astype(np.int64)) + 1, sim.derive()["neighbours"].astype(np.int64))
    sim.kernel_times(reset=True)
    sim.simulate()
    assert len(got["neighbours"]) + n == int(sim.debug_counters()[15]) > n
    sim.close()


# ---- the smallest shapes that can go wrong ----

def test_one_particle_two_coincident_the_radius_itself_and_nobody_near(monkeypatch):
    sim = simulator(np.array([[5.05, 5.05, 5.05]], F))
    got, st = both_paths(sim, monkeypatch, "n = 1")
    assert got["offsets"].tolist() == [0, 0] and got["neighbours"].shape == (0,)
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    sim.neighbour_lists()
    assert sim.neighbour_stats()["longest"] == 0
    sim.close()
    sim = simulator(np.array([[5.05, 5.05, 5.05]] * 2, F))
    for radius in RADII:
        got, _ = both_paths(sim, monkeypatch, "two coincident particles", radius)
        assert got["offsets"].tolist() == [0, 1, 2] and got["neighbours"].tolist() == [1, 0]
    sim.close()
    pos, (near, far), r2 = BS.boundary_pairs()
    assert near == r2 and far > r2
    sim = simulator(pos)
    got, _ = both_paths(sim, monkeypatch, "boundary pairs")
    assert got["offsets"].tolist() == [0, 1, 2, 2, 2] and got["neighbours"].tolist() == [1, 0]
    sim.close()
    # two cells of one particle each: every list empty, and the pointer to no ids may be NULL
    sim = simulator(NS.far_pair())
    got, _ = both_paths(sim, monkeypatch, "two particles far apart")
    assert got["offsets"].tolist() == [0, 0, 0] and got["neighbours"].shape == (0,) and got["neighbours"].dtype == np.uint32
    off, ids, n, entries = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.c_int(-1), C.c_uint64(7)
    assert sim._L.sph_neighbours_host(sim._h, C.byref(off), C.byref(ids), C.byref(n), C.byref(entries)) == 0
    assert (n.value, entries.value) == (2, 0) and [off[k] for k in range(3)] == [0, 0, 0]
    assert sim._L.sph_neighbours_host(sim._h, None, None, None, None) == 0
    sim.close()


def test_wave_tails_and_grids_of_a_few_cells(monkeypatch):
    for n in (63, 64, 65, 129):
        sim = simulator(BS.cluster(n, n))
        got, st = both_paths(sim, monkeypatch, f"n = {n}")
        assert len(got["neighbours"]) > 0 and st["runs_staged"] > 0
        sim.close()
    for name in ("D1", "D2", "D3"):
        pos, vel, g = NS.on_the_walls(name)
        sim = simulator(pos, vel, g["h"], g["cells"])
        for radius in (0.0, 0.5 * float(g["h"])):
            both_paths(sim, monkeypatch, name, radius)
        sim.close()


def test_crowded_cells_runs_about_the_count_slice_and_lists_about_the_sort_slice(monkeypatch):
    # 1,500 rows in one cell: every wave's only run is longer than the slice, every list longer than the sort's
    sim = simulator(BS.one_cell(1500, 5, (50, 50, 50)))
    got, st = both_paths(sim, monkeypatch, "1500 in one cell")
    lengths = np.diff(got["offsets"].astype(np.int64))
    assert lengths.max() == 1499 and lengths.min() > SORT_SLICE
    # (two calls, a count and an emit walk in each)
    assert (st["runs_staged"], st["runs_direct"]) == (0, 4 * -(-1500 // 64)), st
    sim.close()
    # a run of exactly the slice (rows 0 .. SLICE - 1: whole waves) is staged, a run of one more is not
    sim = simulator(np.concatenate([BS.one_cell(SLICE, 6, (20, 20, 20)), BS.one_cell(SLICE + 1, 7, (60, 60, 60))]))
    got, st = both_paths(sim, monkeypatch, "runs of SLICE and SLICE + 1")
    assert (st["runs_staged"], st["runs_direct"]) == (4 * (SLICE // 64), 4 * -(-(SLICE + 1) // 64)), st
    sim.close()
    # lists of exactly the sort's slice are ranked whole, lists of one more in chunks; shorter ones share their waves
    pos, ball = NS.balls((SORT_SLICE + 1, SORT_SLICE + 2, 40), 8)
    sim = simulator(pos)
    got, st = both_paths(sim, monkeypatch, "lists of SORT_SLICE and SORT_SLICE + 1")
    assert np.array_equal(np.diff(got["offsets"].astype(np.int64)), np.array([SORT_SLICE, SORT_SLICE + 1, 39])[ball])
    sim.close()


def test_the_scans_second_round_of_block_sums(monkeypatch):
    """n = 524,289 = 256 x 2,048 + 1: the scan of the list lengths and the scan of the bodies' label flags take 257
    tiles each, so their offsets kernel carries its total into a second round of block sums, and the last tile holds
    one id.  Nothing the results are held to passes through a scan: the derived fields' neighbour counts, and numpy's
    unique over the labels."""
    for env in ("SPH_NEIGHBOURS_PLAIN", "SPH_BODIES_PLAIN", "SPH_DERIVE_PLAIN"):
        monkeypatch.setenv(env, "0")
    n = 256 * 2048 + 1
    box = float(sph.default_settings(n, True).boxDim)
    sim = simulator((np.random.default_rng(524289).random((n, 3)) * box).astype(F))
    got = sim.neighbour_lists()
    offsets = got["offsets"].astype(np.int64)
    assert offsets.shape == (n + 1,) and offsets[0] == 0 and offsets[-1] == len(got["neighbours"])
    assert np.array_equal(np.diff(offsets) + 1, sim.derive()["neighbours"].astype(np.int64))
    bodies = sim.label_bodies()
    labels, table = bodies["labels"], bodies["table"]
    want, counts = np.unique(labels, return_counts=True)
    assert bodies["num_bodies"] == len(want) == len(table)
    assert np.array_equal(table[:, 0], want) and np.array_equal(table[:, 1], counts.astype(np.uint32))
    assert np.array_equal(labels[table[:, 0]], table[:, 0])
    sim.close()


def test_max_entries(monkeypatch):
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    pos, vel = BS.big("dense4096")
    sim = simulator(pos, vel)
    want = all_pairs_of(sim, 0.08, key=("dense4096", 0))
    entries = int(want[0][-1])
    assert entries > 1
    assert_same_lists(sim.neighbour_lists(0.08, max_entries=entries), want, "max_entries = entries")
    sim.neighbour_stats(reset=True)
    with pytest.raises(sph.SphError) as err:
        sim.neighbour_lists(0.08, max_entries=entries - 1)
    assert f"({SPH_ENOMEM})" in str(err.value) and str(entries) in str(err.value) and str(entries - 1) in str(err.value)
    assert sim._L.sph_neighbours_host(sim._h, None, None, None, None) == SPH_ESTATE
    st = sim.neighbour_stats()
    assert (st["calls"], st["entries"]) == (1, entries) and st["longest"] == int(np.diff(want[0].astype(np.int64)).max())
    assert_same_lists(sim.neighbour_lists(0.08), want, "after a refused call")
    assert sim.neighbour_stats()["entries"] == 2 * entries
    sim.close()


def run(timed, listing, steps=10):
    pos, vel = BS.big("dense4096")
    sim = simulator(pos, vel)
    times = sph.Times()
    entries = []
    for _ in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if listing:
            entries.append(len(sim.neighbour_lists(0.08)["neighbours"]))
    st = SH.final_state(sim)
    sim.close()
    return st, entries


@pytest.mark.parametrize("timed", [False, True])
def test_lists_between_every_two_steps_leave_no_footprint(timed, monkeypatch):
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    with_, entries = run(timed, True)
    without, _ = run(timed, False)
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(SH.words(with_[k]), SH.words(without[k])), f"timed={timed}: {k} differs after 10 steps"
    assert len(entries) == 10 and min(entries) > 0 and len(set(entries)) > 1


def test_all_seven_passes_in_one_gap_share_the_grid_and_leave_no_footprint(monkeypatch, tmp_path):
    def start():
        sim = sph.Simulator(sph.default_settings(SH.N, True))
        sim.setup()
        for _ in range(3):
            sim.simulate()
        return sim

    bare = start()
    bare.simulate()
    want = SH.final_state(bare)
    bare.close()
    sim, fresh = start(), sph.Simulator(sph.default_settings(SH.N, True))
    snap = str(tmp_path / "state.snap")
    sim.save_state(snap)
    sim.kernel_times(reset=True)
    passes = dict(SH.passes_of(sim.download_state()["pos"]), neighbours=lambda s: s.neighbour_lists(0.05))
    for plain in ("0", "1"):
        for env in SH.PLAIN + ("SPH_NEIGHBOURS_PLAIN",):
            monkeypatch.setenv(env, plain)
        lists = {}
        for name, call in passes.items():
            lists[name] = call(sim)
        fresh.load_state(snap)
        SH.assert_same(lists["neighbours"], fresh.neighbour_lists(0.05), f"plain={plain}: among the other six against a handle of its own")
        SH.assert_same(lists["neighbours"], passes["neighbours"](sim), f"plain={plain}: after the other six")
    sim.simulate()
    assert sim.kernel_times().steps == 1   # the step's grid was built once, whoever asked for it first
    got = SH.final_state(sim)
    sim.close()
    fresh.close()
    for k in want:
        assert np.array_equal(SH.words(got[k]), SH.words(want[k])), f"{k} differs from the run without passes"


def test_state_rules_error_codes_and_stats(monkeypatch):
    monkeypatch.setenv("SPH_NEIGHBOURS_PLAIN", "0")
    pos, vel = BS.big("dense4096")
    sim = sph.Simulator(sph.default_settings(len(pos), True))
    L, h = sim._L, sim._h
    host = lambda: L.sph_neighbours_host(h, None, None, None, None)

    def opt(radius=0.0, flags=0, pad=0, size=C.sizeof(_lib.SphNeighbourOptions)):
        return C.byref(_lib.SphNeighbourOptions(size, radius, flags, pad, 0))

    # before any state, and the results before the first call
    assert L.sph_neighbour_lists(h, None) == SPH_ESTATE
    assert host() == SPH_ESTATE
    sim.upload_state(pos, vel)
    assert host() == SPH_ESTATE
    # the options
    assert L.sph_neighbour_lists(h, opt(0.05, size=0)) == SPH_EINVAL
    for bad in (float("nan"), float("inf"), -1.0, 1.5 * float(sim.settings.h), float(np.nextafter(F(sim.settings.h), F(1)))):
        assert L.sph_neighbour_lists(h, opt(bad)) == SPH_EINVAL, bad
    assert L.sph_neighbour_lists(h, opt(flags=2)) == SPH_EINVAL
    assert L.sph_neighbour_lists(h, opt(flags=_lib.SPH_NEIGHBOURS_WALK_ORDER | 4)) == SPH_EINVAL
    assert L.sph_neighbour_lists(h, opt(pad=1)) == SPH_EINVAL
    assert host() == SPH_ESTATE
    assert L.sph_neighbour_lists(h, None) == 0          # NULL: every default
    assert host() == 0
    first = sim.neighbour_lists()
    assert_same_lists(sim.neighbour_lists(float(sim.settings.h)), first, "radius = h against radius = 0")
    assert_same_lists(first, all_pairs_of(sim, 0.0, key=("dense4096", 0)), "every default")
    # an upload, the lists again: the new state's
    sim.upload_state(pos[::-1].copy(), vel)
    sim.neighbour_stats(reset=True)
    second = sim.neighbour_lists(0.025)
    assert_same_lists(second, all_pairs_of(sim, 0.025), "after a second upload")
    assert_same_lists(sim.neighbour_lists(0.025), second, "again")
    # the stats sum over calls and reset
    st = sim.neighbour_stats()
    entries = len(second["neighbours"])
    assert (st["calls"], st["entries"]) == (2, 2 * entries) and entries > 0 and st["longest"] == np.diff(second["offsets"].astype(np.int64)).max()
    assert st["seconds"] > 0 and st["runs_staged"] > 0
    assert sim.neighbour_stats(reset=True) == st
    assert sim.neighbour_stats() == dict(calls=0, entries=0, longest=0, runs_staged=0, runs_direct=0, seconds=0.0)
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    assert_same_lists(sim.neighbour_lists(0.025), second, "after sph_phase_grid")
    sim.phase("density")
    assert L.sph_neighbour_lists(h, None) == SPH_ESTATE
    sim.phase("force")
    assert L.sph_neighbour_lists(h, None) == SPH_ESTATE
    sim.phase("readback")
    assert_same_lists(sim.neighbour_lists(0.025), all_pairs_of(sim, 0.025), "after the phase-split step")
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = sph.Simulator(sph.default_settings(4096, True), **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_neighbour_lists(other._h, None) == SPH_ESTATE, kw
        assert other._L.sph_last_error(other._h), kw
        other.close()
    # no particles: SPH_OK, n = 0, offsets = {0}
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    got = empty.neighbour_lists()
    assert got["offsets"].tolist() == [0] and got["offsets"].dtype == np.uint64
    assert got["neighbours"].shape == (0,) and got["neighbours"].dtype == np.uint32
    empty.close()


def read_bin(path, n):
    blob = open(path, "rb").read()
    assert blob[:8] == b"SPHNBR01"
    rows, zero, entries = struct.unpack("<IIQ", blob[8:24])
    assert (rows, zero) == (n, 0) and len(blob) == 24 + 8 * (n + 1) + 4 * entries
    return np.frombuffer(blob, "<u8", n + 1, 24), np.frombuffer(blob, "<u4", entries, 24 + 8 * (n + 1))


def test_cli_free_neighbours(tmp_path):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_NEIGHBOURS_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_NEIGHBOURS": "1", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["frame_%04d.ppm" % f for f in range(2)] + ["neighbours_%04d.bin" % f for f in range(2)]
    said = [l.split() for l in r.stderr.splitlines() if l.startswith("neighbours ")]
    sim = sph.Simulator(sph.default_settings(4096, False))
    sim.setup()
    for f in range(2):
        sim.simulate()
        want = sim.neighbour_lists(float(sim.settings.h))
        offsets, ids = read_bin(tmp_path / ("neighbours_%04d.bin" % f), 4096)
        assert np.array_equal(offsets, want["offsets"]) and np.array_equal(ids, want["neighbours"]), f
        assert said[f] == ["neighbours", str(f), str(len(ids)), str(int(np.diff(offsets.astype(np.int64)).max()))], said
        assert len(ids) > 0
    sim.close()
    # a bad value prints one line and writes no neighbour files
    for value in ("yes", "0", "1.5"):
        bad = tmp_path / ("bad" + value)
        bad.mkdir()
        env.update({"SPH_FREE_FRAMES": "1", "SPH_FREE_NEIGHBOURS": value, "SPH_FREE_FRAMES_DIR": str(bad)})
        r = subprocess.run([SPH, "-n", "4096", "-i", "grid", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and ("SPH_FREE_NEIGHBOURS=" + value) in r.stderr and sorted(os.listdir(bad)) == ["frame_0000.ppm"], value
