"""The field sample on the GPU (sph_sample_field): against the density sweep's own rho,
against its numpy restatement (tests/field_sample_restatement.py) fed by sph_download_grid + sph_download_state,
the tile path against the plain path, and its absence from the run's results.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import field_sample_restatement as FS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SWEEPS = ("list", "lds", "direct")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == F, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} values differ, first at {np.argwhere(bad)[0]}: " \
                          f"{a[tuple(np.argwhere(bad)[0])]!r} vs {b[tuple(np.argwhere(bad)[0])]!r}"


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def sorted_state(sim):
    """what the restatement is fed with: the grid the sampler walked and the state, row by row of the sorted stream"""
    g = sim.download_grid()
    st = sim.download_state()
    ids = g["ids"].astype(np.int64)
    return st["pos"][ids], st["vel"][ids], st["rho"][ids], g["cells"]


def restate(sim, grid, field, origin, spacing, shape):
    s = sim.settings
    return FS.sample(grid[0], grid[1], grid[2], grid[3], s.h, s.d_kernel_coeff, s.numCellsPerDim, field, origin, spacing, shape)


# (origin, spacing, (nz, ny, nx)) around a point `a` inside the fluid: spacing << h (a whole wave in one cell,
# nx = 200), spacing > h (every lane a cell of its own, nx = 65), nx = 63 and nx = 1, one point; then the lattices
# that leave the grid: x from -0.05 to past 10 through cells 0 and D - 1, and the same for y and for z.
def lattices(a):
    ax, ay, az = (float(v) for v in a)
    return [((ax - 0.1, ay - 0.05, az - 0.05), (0.001, 0.05, 0.05), (3, 3, 200)),
            ((ax - 1.5, ay - 0.15, az - 0.15), (0.15, 0.15, 0.15), (3, 3, 65)),
            ((ax - 0.6, ay - 0.03, az - 0.03), (0.02, 0.07, 0.07), (2, 2, 63)),
            ((ax - 0.01, ay - 0.1, az - 0.1), (0.05, 0.05, 0.05), (4, 5, 1)),
            ((ax + 0.01, ay + 0.01, az + 0.01), (0.1, 0.1, 0.1), (1, 1, 1)),
            ((-0.05, 0.03, 0.03), (0.0506, 4.98, 4.98), (3, 3, 200)),
            ((0.03, -0.05, 0.03), (0.02, 5.04, 0.02), (2, 3, 5)),
            ((0.03, 0.03, -0.05), (0.02, 0.02, 5.04), (3, 2, 5))]


def check_everything(sims, anchor, what, monkeypatch, fields=FS.FIELDS):
    """Every lattice and field: the tile path of sims[0] against the restatement, then the plain path of the same
    handle and both paths of the other handles (other sweeps, same state) against those values."""
    grid = None
    nonzero = 0
    for origin, spacing, shape in lattices(anchor):
        for field in fields:
            monkeypatch.setenv("SPH_SAMPLE_PLAIN", "0")
            got = sims[0].sample_field(field, origin, spacing, shape)
            if grid is None:
                grid = sorted_state(sims[0])      # (taken after the call: the grid the sampler walked)
            assert_same_bits(got, restate(sims[0], grid, field, origin, spacing, shape), f"{what} {field} {origin} {spacing} {shape}")
            nonzero += int((got > 0).sum())
            for k, sim in enumerate(sims):
                for plain in ("0", "1"):
                    if k == 0 and plain == "0":
                        continue
                    monkeypatch.setenv("SPH_SAMPLE_PLAIN", plain)
                    assert_same_bits(sim.sample_field(field, origin, spacing, shape), got,
                                     f"{what} {field} {origin} {spacing} {shape}: sweep {SWEEPS[k]}, plain={plain}")
    assert nonzero > 100, f"{what}: the lattices miss the fluid"


def test_density_sample_on_the_initial_lattice_is_the_sweeps_rho():
    # -i grid: particle id (x * 109 + y) * 109 + z sits at h + (0.9f h) * (x, y, z); n = 2048: x = 0, id = y * 109 + z.
    # The lattice below puts a point on every one of them; the density sweep of the first step then forms the
    # same sum, over the same candidates in the same order, and clamps it to EPS_F.
    sim = make(2048, random=False)
    sim.setup()
    h = F(sim.settings.h)
    sp = float(F(0.9) * h)
    sample = sim.sample_field("density", (float(h),) * 3, (sp, sp, sp), (109, 19, 1))
    pos0 = sim.download_state()["pos"]
    sim.simulate()
    rho = sim.download_state()["rho"]
    pts = FS.lattice_points((float(h),) * 3, (sp, sp, sp), (109, 19, 1))
    compared = 0
    for y in range(19):
        for z in range(109):
            i = y * 109 + z
            if i >= 2048:
                continue
            assert bits(pts[z, y, 0]).tolist() == bits(pos0[i]).tolist()
            assert bits(np.maximum(sample[z, y, 0], FS.EPS_F)).item() == bits(rho[i]).item(), (y, z, sample[z, y, 0], rho[i])
            compared += 1
    assert compared == 2048 and (rho > FS.EPS_F).all()
    sim.close()


@pytest.mark.parametrize("steps", [0, 5])
@pytest.mark.parametrize("name", ["dense4096", "random4096"])
def test_fields_against_the_restatement_on_every_path_and_sweep(name, steps, monkeypatch):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    sims = []
    for sweep in SWEEPS:
        sim = make(len(data["pos_1"]), sweep=sweep)
        sim.upload_state(data["pos_1"], data["vel_1"])
        for _ in range(steps):
            sim.simulate()
        sims.append(sim)
    st = sims[0].download_state()
    if steps:
        assert (st["rho"] > 0).all()
        assert name != "dense4096" or (st["prs"] > 0).any(), "no particle under pressure: the case is not covered"
    check_everything(sims, st["pos"][7], f"{name} + {steps} steps", monkeypatch)
    for sim in sims:
        sim.close()


def crowded_state():
    """3000 particles in cell (50, 50, 50), its +x neighbour empty, 60 in the -x neighbour, 15 each in cell 0 and in
    cell D - 1 of every axis: the stretch a wave stages runs over several LDS chunks"""
    rng = np.random.default_rng(11)
    parts = [5.0 + 0.099 * rng.random((3000, 3)), np.array([4.9, 5.0, 5.0]) + 0.099 * rng.random((60, 3)),
             0.099 * rng.random((15, 3)), 9.9 + 0.09 * rng.random((15, 3))]
    pos = np.ascontiguousarray(np.concatenate(parts), dtype=F)
    vel = rng.uniform(-2, 2, pos.shape).astype(F)
    return pos, vel


def set_densities(sim, rho, path):
    """rho (by particle id) into the state through a snapshot: 64 bytes of header, then n rows (x, y, z, id) and n
    rows (vx, vy, vz, rho)"""
    sim.save_state(path)
    blob = np.fromfile(path, np.uint8)
    n = sim.n
    rows = blob[64:].view(F).reshape(2, n, 4)
    ids = rows[0, :, 3].view(np.uint32)
    rows[1, :, 3] = rho[ids]
    blob.tofile(path)
    sim.load_state(path)


def test_a_crowded_cell_runs_over_several_chunks(monkeypatch, tmp_path):
    pos, vel = crowded_state()
    rho = np.random.default_rng(12).uniform(800, 1400, len(pos)).astype(F)   # pressure 0 for a third, up to 400
    sims = []
    for sweep in SWEEPS:
        sim = make(len(pos), sweep=sweep)
        sim.upload_state(pos, vel)
        set_densities(sim, rho, tmp_path / "crowded.bin")
        sims.append(sim)
    st = sims[0].download_state()
    assert np.array_equal(bits(st["rho"]), bits(rho)) and (st["prs"] > 0).any() and (st["prs"] == 0).any()
    check_everything(sims, (5.05, 5.05, 5.05), "crowded cell", monkeypatch)
    cells = sims[0].download_grid()["cells"]
    run = cells[(50 * 100 + 50) * 100 + 50]
    assert run[1] - run[0] == 3000 and (cells[(50 * 100 + 50) * 100 + 51] == 0).all()
    # the corner cells hold fluid the edge lattices see
    got = sims[0].sample_field("density", (-0.05, 0.03, 0.03), (0.0506, 4.98, 4.98), (3, 3, 200))
    assert got[0, 0, 1] > 0 and got[2, 2, 198] > 0 and bits(got[0, 0, 0]) == 0 and bits(got[2, 2, 199]) == 0
    for sim in sims:
        sim.close()


SLICE = ((0.0, 0.0, 5.0), (0.25, 0.25, 1.0), (1, 40, 40))


def run_steps(n, steps, timed, sampling, between=None):
    sim = make(n)
    sim.setup()
    times = sph.Times()
    for k in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if k + 1 < steps:
            if sampling:
                sim.sample_field("speed" if k & 1 else "density", *SLICE)
            if between:
                between(sim, k)
    out = sim.download_state()
    out["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return out, times


def assert_same_run(a, b, what):
    for k in ("pos", "vel", "rho", "host"):
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("pipeline", ["0", "1"])
@pytest.mark.parametrize("timed", [False, True])
def test_sampling_between_steps_leaves_no_footprint(timed, pipeline, monkeypatch):
    monkeypatch.setenv("SPH_PIPELINE", pipeline)
    with_samples, t1 = run_steps(4096, 6, timed, True)
    without, t0 = run_steps(4096, 6, timed, False)
    assert_same_run(with_samples, without, f"timed={timed} SPH_PIPELINE={pipeline}")
    if timed:
        for t in (t0, t1):
            assert t.iters == 6 and t.buildGrid > 0 and t.sphUpdate > 0


def test_a_click_or_a_reload_after_a_sample_drops_its_grid(tmp_path):
    def click(sim, k):
        if k == 2:
            sim.moveParticles((400, 300))

    def reload(sim, k):
        if k == 2:
            sim.save_state(tmp_path / "state.bin")
            sim.load_state(tmp_path / "state.bin")

    for what, between in (("click", click), ("save + load", reload)):
        a, _ = run_steps(4096, 5, False, True, between)
        b, _ = run_steps(4096, 5, False, False, between)
        assert_same_run(a, b, what)
    # ... and the click did something
    plain, _ = run_steps(4096, 5, False, False)
    clicked, _ = run_steps(4096, 5, False, False, click)
    assert not np.array_equal(bits(clicked["vel"]), bits(plain["vel"]))


def click_sequence(timed, sampling, order):
    """6 steps, then the calls of `order` ("c" a click, "s" a sample, skipped without sampling), then 2 more steps"""
    sim = make(4096)
    sim.setup()
    times = sph.Times()
    step = (lambda: sim.simulateAndTime(times)) if timed else sim.simulate
    for _ in range(6):
        step()
    for call in order:
        if call == "c":
            sim.moveParticles((400, 300))
        elif sampling:
            sim.sample_field("density", *SLICE)
    mid = sim.download_state()
    for _ in range(2):
        step()
    out = sim.download_state()
    out["host"] = np.array(sim.getPosition(), copy=True)
    sim.close()
    return mid, out


@pytest.mark.parametrize("timed,pipeline,order", [(True, "1", "cscs"), (False, "1", "scsc"), (True, "0", "scscsc"), (False, "0", "cscsc")])
def test_clicks_between_samples_walk_the_last_steps_table(timed, pipeline, order, monkeypatch):
    # every grid build between two steps leaves the table of the last completed step alone: a second (third)
    # click after a sample walks it like the first
    monkeypatch.setenv("SPH_PIPELINE", pipeline)
    mid1, end1 = click_sequence(timed, True, order)
    mid0, end0 = click_sequence(timed, False, order)
    assert np.array_equal(bits(mid1["vel"]), bits(mid0["vel"])), f"{order}: velocities after the clicks differ"
    assert_same_run(end1, end0, f"timed={timed} SPH_PIPELINE={pipeline} {order}")
    # ... and every click of the sequence did something: one click fewer gives other velocities
    fewer, _ = click_sequence(timed, False, order.replace("c", "", 1))
    assert not np.array_equal(bits(fewer["vel"]), bits(mid0["vel"]))


def test_state_rules_and_the_grid_that_was_walked():
    sim = make(4096)
    sim.setup()
    sim.simulate()
    # phase 0: the sample builds the next step's grid; sph_download_grid returns it, and it is the grid of the
    # state the handle holds now
    got = sim.sample_field("density", *SLICE)
    grid = sorted_state(sim)
    assert_same_bits(got, restate(sim, grid, "density", *SLICE), "after a step")
    st = sim.download_state()
    keys = sim.download_grid()["keys"]
    c, outside = FS.cells_of(grid[0], sim.settings.h, sim.settings.numCellsPerDim)
    assert not outside.any() and np.array_equal(keys, ((c[:, 2] * 100 + c[:, 1]) * 100 + c[:, 0]).astype(np.uint32))
    assert (np.diff(keys.astype(np.int64)) >= 0).all() and st["pos"].shape == (4096, 3)
    # a second sample uses it as it is; a grid phase called by hand is used as it is, too
    assert_same_bits(sim.sample_field("density", *SLICE), got, "second sample")
    sim.phase("grid")
    assert_same_bits(sim.sample_field("density", *SLICE), got, "after sph_phase_grid")
    sim.phase("density")
    with pytest.raises(sph.SphError, match=r"\(-4\)"):       # an open phase-split step
        sim.sample_field("density", *SLICE)
    sim.phase("force")
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.sample_field("density", *SLICE)
    sim.phase("readback")
    after = sim.sample_field("density", *SLICE)
    assert_same_bits(after, restate(sim, sorted_state(sim), "density", *SLICE), "after the phase-split step")
    assert not np.array_equal(bits(after), bits(got))
    sim.close()


def test_error_codes():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):       # SPH_ESTATE: before any state
        sim.sample_field("density", *SLICE)
    assert not sim._L.sph_sample_host(sim._h, None, None, None)
    sim.setup()
    nan, inf = float("nan"), float("inf")
    ok = dict(field="density", origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1), shape=(2, 2, 2))
    bad = [dict(shape=(0, 2, 2)), dict(shape=(2, 0, 2)), dict(shape=(2, 2, 0)), dict(shape=(2, 2, 4097)), dict(shape=(-1, 2, 2)),
           dict(shape=(4096, 4096, 2)), dict(shape=(257, 256, 256)),
           dict(origin=(nan, 0, 0)), dict(origin=(0, inf, 0)), dict(origin=(0, 0, -inf)),
           dict(spacing=(0.0, 0.1, 0.1)), dict(spacing=(0.1, -0.1, 0.1)), dict(spacing=(0.1, 0.1, nan)), dict(spacing=(inf, 0.1, 0.1)),
           dict(field=3), dict(field=-1)]
    for b in bad:
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.sample_field(**{**ok, **b})
    lat = _lib.SphSampleLattice()                            # struct_size left at 0
    assert sim._L.sph_sample_field(sim._h, C.byref(lat)) == -1
    assert sim._L.sph_sample_field(sim._h, None) == -1
    assert sim.sample_field(**{**ok, "shape": (256, 256, 256)}).shape == (256, 256, 256)   # 1 << 24 points: allowed
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = make(4096, **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        with pytest.raises(sph.SphError, match=r"\(-4\)"):
            other.sample_field(**ok)
        other.close()


def test_no_particles_samples_zeros_and_the_time_is_counted():
    empty = make(0)
    empty.setup()
    got = empty.sample_field("speed", *SLICE)
    assert got.shape == (1, 40, 40) and (bits(got) == 0).all()
    empty.close()
    sim = make(4096)
    sim.setup()
    sim.sample_time(reset=True)
    for field in FS.FIELDS:
        out = sim.sample_field(field, *SLICE)
        assert out.shape == (1, 40, 40) and out.dtype == F
    sec, count = sim.sample_time(reset=True)
    assert count == 3 and 0.0 < sec < 1.0
    assert sim.sample_time() == (0.0, 0)
    # the defaults of the Python front end: one point at the origin, density
    assert sim.sample_field().shape == (1, 1, 1)
    nx, ny, nz = C.c_int(0), C.c_int(0), C.c_int(0)
    assert sim._L.sph_sample_host(sim._h, C.byref(nx), C.byref(ny), C.byref(nz))
    assert (nx.value, ny.value, nz.value) == (1, 1, 1)
    sim.close()


def test_cli_free_slice(tmp_path):
    env = dict(os.environ)
    env.pop("SPH_FREE_SHADE", None)
    env.update({"SPH_FREE_FRAMES": "3", "SPH_FREE_FRAMES_DIR": str(tmp_path), "SPH_FREE_SLICE": "density"})
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(tmp_path))
    assert names == ["frame_%04d.ppm" % f for f in range(3)] + ["slice_%04d.ppm" % f for f in range(3)]
    blob = open(os.path.join(tmp_path, names[-1]), "rb").read()
    header = b"P6\n400 400\n255\n"
    assert blob.startswith(header) and len(blob) == len(header) + 400 * 400 * 3
    # the last slice is the plane z = 5 of the state after three steps, row 0 = largest y, coloured over its own range
    sim = make(4096)
    sim.setup()
    for _ in range(3):
        sim.simulate()
    sp = float(F(10) / F(400))
    v = sim.sample_field("density", (0.0, 0.0, 5.0), (sp, sp, 1.0), (1, 400, 400))[0]
    sim.close()
    import field_frame_restatement as FF
    want = FF.ramp(FF.quantise(v[::-1], v.min(), v.max()))
    assert v.max() > v.min()
    assert np.array_equal(np.frombuffer(blob[len(header):], np.uint8).reshape(400, 400, 3), want)


def test_sample_plain_selects_the_plain_kernel(tmp_path):
    # SPH_STEP_TRACE=1 makes the library say which kernel served its samples; the slices do not depend on it
    blobs = {}
    for plain in ("0", "1"):
        out = tmp_path / plain
        out.mkdir()
        env = dict(os.environ)
        env.pop("SPH_FREE_SHADE", None)
        env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_FRAMES_DIR": str(out), "SPH_FREE_SLICE": "speed",
                    "SPH_SAMPLE_PLAIN": plain, "SPH_STEP_TRACE": "1"})
        r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        want = "2 samples by k_sample_tile, 0 by k_sample_plain" if plain == "0" else "0 samples by k_sample_tile, 2 by k_sample_plain"
        assert want in r.stderr, r.stderr
        blobs[plain] = open(out / "slice_0001.ppm", "rb").read()
    assert blobs["0"] == blobs["1"] and len(blobs["0"]) > 400 * 400 * 3


def test_cli_with_the_linked_sweep_writes_frames_and_no_slices(tmp_path):
    env = dict(os.environ)
    env.pop("SPH_FREE_SHADE", None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_FRAMES_DIR": str(tmp_path), "SPH_FREE_SLICE": "density", "SPH_SWEEP": "linked"})
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert "sampleField" in r.stderr and "SPH_SWEEP_LINKED" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["frame_0000.ppm", "frame_0001.ppm"]
