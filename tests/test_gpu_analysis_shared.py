"""What the analysis passes share on the host ("what every analysis pass shares"): one view of the
grid's sorted stream in both of its layouts, one grid built ahead that every pass of a gap between two steps finds,
and one set of state rules.  The passes' own tests hold each result to its restatement; here the passes are held to
each other: all of them between the same two steps leave the run's results alone and give what a handle that holds
nothing but that state gives.  Every comparison is of 32-bit words.  Measured on an MI355X: the three cases take 0.9
to 1.8 s, the costliest 0.5 s."""
import ctypes as C

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
SPH_ESTATE = -4
N = 4096
PLAIN = ("SPH_SAMPLE_PLAIN", "SPH_SURFACE_PLAIN", "SPH_DIAG_PLAIN", "SPH_TRACER_PLAIN", "SPH_DERIVE_PLAIN", "SPH_BODIES_PLAIN", "SPH_PAIRS_PLAIN")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def flat(result):
    """a pass's result as name -> words"""
    if isinstance(result, dict):
        return {k: words(np.asarray(v)) if isinstance(v, np.ndarray) else np.array([v], np.uint32) for k, v in result.items()}
    return {"": words(result)}


def assert_same(got, want, what):
    got, want = flat(got), flat(want)
    assert got.keys() == want.keys(), what
    for k in got:
        assert got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} vs {want[k].shape}"
        bad = got[k] != want[k]
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words of {k or 'the result'} differ"


def lattice_of(pos):
    """an 8^3 lattice over the particles' box: origin, spacing"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    return tuple(float(v) for v in lo), tuple(float(v) for v in (hi - lo) / F(7))


def passes_of(pos):
    """name -> call(sim) of the seven passes (the pair statistics twice) on the state whose positions (id order) are
    `pos`; the same arguments for every handle that holds that state"""
    origin, spacing = lattice_of(pos)
    seeds = np.ascontiguousarray(pos[:130] + F(0.013))  # two full waves and a tail

    def tracers(sim):
        sim.set_tracers(seeds)
        sim.advect_tracers()
        return sim.tracers()

    def diagnostics(sim):
        sim.diagnose("density")
        return np.frombuffer(bytes(sim.diagnostics_raw()), np.uint8).copy()

    def surface(sim):
        # a level the lattice's densities straddle
        field = sim.sample_field("density", origin, spacing, (8, 8, 8))
        return sim.extract_surface(float(F(0.5) * field.max()), origin, spacing, (8, 8, 8))

    return {"sample": lambda sim: sim.sample_field("speed", origin, spacing, (8, 8, 8)),
            "surface": surface, "diagnostics": diagnostics, "tracers": tracers,
            "derive": lambda sim: sim.derive(), "bodies": lambda sim: sim.label_bodies(0.05),
            # (the raw rows: the pairs, the low and high words of the four sums, the saturation counts)
            # this lattice start's neighbours stand just under h apart: the table within 0.05 is empty, the one within h not
            "pairs": lambda sim: sim.pair_statistics(16, 0.05)["rows"].view(np.uint64),
            "pairs within h": lambda sim: sim.pair_statistics(0, 0.0)["rows"].view(np.uint64)}


def final_state(sim):
    st = sim.download_state()
    st["host"] = np.array(sim.getPosition(), copy=True)
    return st


@pytest.mark.parametrize("sweep", ["list", "direct"])  # the interleaved records (stride 2), the two sorted streams (stride 1)
def test_all_passes_between_steps_share_one_grid_and_leave_no_footprint(sweep, monkeypatch, tmp_path):
    def start():
        sim = sph.Simulator(sph.default_settings(N, True), sweep=sweep)
        sim.setup()
        for _ in range(3):
            sim.simulate()
        return sim

    bare = start()
    for _ in range(4):
        bare.simulate()
    want = final_state(bare)
    bare.close()

    sim, fresh = start(), sph.Simulator(sph.default_settings(N, True), sweep=sweep)
    snap = str(tmp_path / "state.snap")
    sim.kernel_times(reset=True)
    meshes = 0
    for step in range(4):
        sim.simulate()
        if step == 3:
            break
        sim.save_state(snap)  # the rows as the handle holds them, densities included
        passes = passes_of(sim.download_state()["pos"])
        results = {}
        for plain in ("0", "1"):
            for env in PLAIN:
                monkeypatch.setenv(env, plain)
            for name, call in passes.items():
                got = results[name, plain] = call(sim)
                fresh.load_state(snap)
                assert_same(got, call(fresh), f"{name} (plain={plain}) after step {4 + step}, among the others against a handle of its own")
        for name in passes:
            assert_same(results[name, "1"], results[name, "0"], f"{name} after step {4 + step}: check path against default path")
        meshes += len(results["surface", "0"]["triangles"])
        assert results["bodies", "0"]["num_bodies"] >= 1 and results["derive", "0"]["neighbours"].min() >= 1
        assert results["pairs within h", "0"].reshape(32, -1)[:, 0].sum() > 0
    assert meshes > 0, "no lattice met the surface"
    # every step's grid was built once, whoever asked for it first
    kt = sim.kernel_times()
    assert kt.steps == 4
    got = final_state(sim)
    sim.close()
    fresh.close()
    for k in want:
        assert np.array_equal(words(got[k]), words(want[k])), f"{k} differs from the run without passes"


def entry_points():
    """name -> call(sim) -> return code of the five entry points that walk the grid's sorted stream, with valid arguments"""
    lat = _lib.SphSampleLattice()
    lat.struct_size = C.sizeof(_lib.SphSampleLattice)
    lat.nx = lat.ny = lat.nz = 2
    lat.spacing[:] = [0.5, 0.5, 0.5]
    lat.field = _lib.FIELDS["density"]
    srf = _lib.SphSurfaceOptions()
    srf.struct_size = C.sizeof(_lib.SphSurfaceOptions)
    srf.nx = srf.ny = srf.nz = 2
    srf.spacing[:] = [0.5, 0.5, 0.5]
    srf.iso = 1.0
    return {"sph_sample_field": lambda s: s._L.sph_sample_field(s._h, C.byref(lat)),
            "sph_extract_surface": lambda s: s._L.sph_extract_surface(s._h, C.byref(srf)),
            "sph_tracers_advect": lambda s: s._L.sph_tracers_advect(s._h, 0.0),
            "sph_derive": lambda s: s._L.sph_derive(s._h),
            "sph_label_bodies": lambda s: s._L.sph_label_bodies(s._h, None)}


def test_state_rules_of_the_five_entry_points():
    calls = entry_points()
    make = lambda **kw: sph.Simulator(sph.default_settings(N, True), **kw)
    # SPH_ESTATE: a slab handle, no state yet, the linked lists, Morton keys
    for what, kw, stepped in (("slab handle", dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=N), False),
                              ("before setup()", dict(), False),
                              ("SPH_SWEEP_LINKED", dict(sweep="linked"), True),
                              ("SPH_KEY_MORTON", dict(sweep="direct", key_order="morton"), True)):
        other = make(**kw)
        if stepped:
            other.setup()
            other.simulate()
        for name, call in calls.items():
            assert call(other) == SPH_ESTATE, (name, what)
            assert other._L.sph_last_error(other._h), (name, what)
        other.close()

    sim = make()
    sim.setup()
    sim.set_tracers(np.full((130, 3), 0.5, F))
    sim.simulate()
    # phase 0: the first pass builds the next step's grid ahead, the others find it, the step consumes it
    sim.kernel_times(reset=True)
    for name, call in calls.items():
        assert call(sim) == 0, name
    sim.simulate()
    assert sim.kernel_times(reset=True).steps == 1
    # phase 1: the grid is there; nothing is built (the phase calls record no events, a grid built ahead would)
    sim.phase("grid")
    for name, call in calls.items():
        assert call(sim) == 0, name
    # SPH_ESTATE: a phase-split step is open
    for phase in ("density", "force"):
        sim.phase(phase)
        for name, call in calls.items():
            assert call(sim) == SPH_ESTATE, (name, phase)
    sim.phase("readback")
    kt = sim.kernel_times()
    assert (kt.steps, kt.hash, kt.sort) == (0, 0.0, 0.0)
    for name, call in calls.items():
        assert call(sim) == 0, name
    sim.close()

    # no particles: SPH_OK and empty results
    empty = sph.Simulator(sph.default_settings(0, True))
    empty.setup()
    seeds = np.full((3, 3), 0.5, F)
    empty.set_tracers(seeds)
    for name, call in calls.items():
        assert call(empty) == 0, name
    assert not empty.sample_field("density", shape=(2, 2, 2)).any()
    mesh = empty.extract_surface(1.0, shape=(2, 2, 2))
    assert mesh["vertices"].shape == (0, 3) and mesh["triangles"].shape == (0, 3)
    t = empty.tracers()
    assert np.array_equal(t["pos"], seeds) and not t["den"].any() and not t["vel"].any()
    d = empty.derive()
    assert d["vorticity"].shape == d["grad_rho"].shape == (0, 3) and d["rho"].shape == d["neighbours"].shape == (0,)
    b = empty.label_bodies()
    assert b["labels"].shape == (0,) and b["table"].shape == (0, 8) and (b["num_bodies"], b["largest"]) == (0, 0)
    empty.close()
