"""The surface mesh on the GPU (sph_extract_surface): against its numpy restatement
(tests/surface_restatement.py) fed by the field sample of the same lattice, the production path against the plain path, the
three sweeps against each other, its topology and volume around one and two particles, and its absence from the run's
results.  Every comparison of a mesh is exact."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import surface_restatement as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SWEEPS = ("list", "lds", "direct")
MASS = 0.02


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_mesh(a, b, what):
    va, vb = a["vertices"], b["vertices"]
    assert va.shape == vb.shape and va.dtype == vb.dtype == F, f"{what}: vertices {va.shape} {va.dtype} vs {vb.shape} {vb.dtype}"
    bad = bits(va) != bits(vb)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {va.size} coordinates differ, first at {np.argwhere(bad)[0]}"
    ta, tb = a["triangles"], b["triangles"]
    assert ta.shape == tb.shape and ta.dtype == tb.dtype == np.uint32, f"{what}: triangles {ta.shape} {ta.dtype} vs {tb.shape} {tb.dtype}"
    bad = ta != tb
    assert not bad.any(), f"{what}: {int(bad.sum())} of {ta.size} indices differ, first at {np.argwhere(bad)[0]}"


SLICE = ((0.0, 0.0, 5.0), (0.25, 0.25, 1.0), (1, 40, 40))
BOX = ((0.0, 0.0, 0.0), 0.25, (41, 41, 41))
ISO = 1.0


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def restate(field, origin, spacing, iso):
    v, t, _ = SR.extract(field, origin, spacing, iso)
    return {"vertices": v, "triangles": t}


# (origin, spacing, (nz, ny, nx)) around a point `a` inside the fluid, h = 0.1: 33^3 with spacing h / 4; nx = 65, one
# point past a wave; nx = 2, the narrowest row, in 4900 rows; x from -0.05 to 10.05 through a; the whole box and a
# margin, which leaves the grid on both sides of every axis.  (A wave holds 64 consecutive points of the lattice: with
# nx = 65, 2, 129, 66 and 33 its rows end at every lane.)
def lattices(a, h):
    ax, ay, az = (float(v) for v in a)
    q = float(F(h) / F(4))
    return [((ax - 16 * q, ay - 16 * q, az - 16 * q), (q, q, q), (33, 33, 33)),
            ((ax - 32 * q, ay - 2 * q, az - 2 * q), (q, q, q), (5, 6, 65)),
            ((ax - q / 2, ay - 35 * q, az - 35 * q), (q, q, q), (70, 70, 2)),
            ((-0.05, ay - 2 * q, az - 2 * q), (10.1 / 128, q, q), (5, 5, 129)),
            ((-0.05, -0.05, -0.05), (10.1 / 65,) * 3, (66, 66, 66))]


@pytest.mark.parametrize("steps", [0, 5])
@pytest.mark.parametrize("name", ["dense4096", "random4096"])
def test_meshes_against_the_restatement_on_every_path_and_sweep(name, steps, monkeypatch):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    sims = []
    for sweep in SWEEPS:
        sim = make(len(data["pos_1"]), sweep=sweep)
        sim.upload_state(data["pos_1"], data["vel_1"])
        for _ in range(steps):
            sim.simulate()
        sims.append(sim)
    anchor = sims[0].download_state()["pos"][7]
    triangles = 0
    for origin, spacing, shape in lattices(anchor, sims[0].settings.h):
        what = f"{name} + {steps} steps {origin} {spacing} {shape}"
        field = sims[0].sample_field("density", origin, spacing, shape)
        iso = float(field.max()) / 2 if field.max() > 0 else 1.0
        monkeypatch.setenv("SPH_SURFACE_PLAIN", "0")
        got = sims[0].extract_surface(iso, origin, spacing, shape)
        assert_same_mesh(got, restate(field, origin, spacing, iso), what)
        triangles += len(got["triangles"])
        for k, sim in enumerate(sims):
            for plain in ("0", "1"):
                if k == 0 and plain == "0":
                    continue
                monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
                assert_same_mesh(sim.extract_surface(iso, origin, spacing, shape), got, f"{what}: sweep {SWEEPS[k]}, plain={plain}")
    assert triangles > 100, f"{name} + {steps} steps: the lattices miss the surface"
    for sim in sims:
        sim.close()


def test_the_scan_across_more_blocks_than_one_round_takes(monkeypatch):
    # the scan across the blocks' sums walks them in rounds of 2048 blocks of 1024 points: 130^3 points are 2146 blocks
    sim = make(4096)
    sim.setup()
    origin, spacing, shape = (-0.05, -0.05, -0.05), 10.1 / 129, (130, 130, 130)
    field = sim.sample_field("density", origin, spacing, shape)
    want = restate(field, origin, spacing, ISO)
    assert len(want["triangles"]) > 100
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
        assert_same_mesh(sim.extract_surface(ISO, origin, spacing, shape), want, f"130^3, plain={plain}")
    sim.close()


@pytest.mark.parametrize("particles,shape,chi", [(1, (21, 21, 21), 2), (2, (21, 21, 49), 4)])
def test_the_surface_around_single_particles(particles, shape, chi, monkeypatch):
    # a particle's density is MASS d_kernel_coeff (h^2 - r^2)^3 within h: the level set is a sphere
    sim = make(particles)
    s = sim.settings
    h = float(s.h)
    sp = float(F(h) / F(8))
    first = np.array([5.03, 5.02, 5.01])
    pos = np.array([first + (3 * h * k, 0, 0) for k in range(particles)], F)
    sim.upload_state(pos)
    nz, ny, nx = shape
    origin = tuple(float(v) for v in (first + (1.5 * h * (particles - 1), 0, 0) - (sp * (nx - 1) / 2, sp * (ny - 1) / 2, sp * (nz - 1) / 2)))
    peak = MASS * float(s.d_kernel_coeff) * h ** 6
    iso = peak / 2
    r = math.sqrt(h * h - (iso / (MASS * float(s.d_kernel_coeff))) ** (1.0 / 3.0))
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
        mesh = sim.extract_surface(iso, origin, sp, shape)
        verts, tris = mesh["vertices"], mesh["triangles"]
        assert len(tris) > 100 * particles
        most, lone = SR.edge_pairing(tris)
        assert most == 1 and len(lone) == 0, "the mesh is not closed"
        assert SR.euler(verts, tris) == chi
        vol = SR.signed_volume(verts, tris)
        lo, hi = (particles * 4 / 3 * math.pi * (r + k * math.sqrt(3) * sp) ** 3 for k in (-1, 1))
        assert 0 < lo < vol < hi, (lo, vol, hi)
    sim.close()


def test_the_sample_is_left_alone():
    sim = make(4096)
    sim.setup()
    sim.simulate()
    want = sim.sample_field("density", *SLICE)
    mesh = sim.extract_surface(ISO, *BOX)
    assert len(mesh["triangles"]) > 0
    nx, ny, nz = C.c_int(0), C.c_int(0), C.c_int(0)
    p = sim._L.sph_sample_host(sim._h, C.byref(nx), C.byref(ny), C.byref(nz))
    assert p and (nx.value, ny.value, nz.value) == (40, 40, 1)
    assert np.array_equal(bits(np.ctypeslib.as_array(p, shape=(1, 40, 40))), bits(want))
    sim.close()


def run_steps(n, steps, timed, meshing, between=None):
    sim = make(n)
    sim.setup()
    times = sph.Times()
    for k in range(steps):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if k + 1 < steps:
            if meshing:
                sim.extract_surface(ISO * (1 + k), *BOX)
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
def test_extracting_between_steps_leaves_no_footprint(timed, pipeline, monkeypatch):
    monkeypatch.setenv("SPH_PIPELINE", pipeline)
    with_meshes, t1 = run_steps(4096, 6, timed, True)
    without, t0 = run_steps(4096, 6, timed, False)
    assert_same_run(with_meshes, without, f"timed={timed} SPH_PIPELINE={pipeline}")
    if timed:
        for t in (t0, t1):
            assert t.iters == 6 and t.buildGrid > 0 and t.sphUpdate > 0


def test_a_click_or_a_reload_after_an_extraction_drops_its_grid(tmp_path):
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
    plain, _ = run_steps(4096, 5, False, False)
    clicked, _ = run_steps(4096, 5, False, False, click)
    assert not np.array_equal(bits(clicked["vel"]), bits(plain["vel"]))


def test_state_rules_and_the_grid_that_was_walked():
    sim = make(4096)
    sim.setup()
    sim.simulate()
    # phase 0: the extraction builds the next step's grid; the sample of the same lattice walks the same grid
    got = sim.extract_surface(ISO, *BOX)
    keys = sim.download_grid()["keys"]
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    assert_same_mesh(got, restate(sim.sample_field("density", *BOX), *BOX[:2], ISO), "after a step")
    assert np.array_equal(sim.download_grid()["keys"], keys)
    assert_same_mesh(sim.extract_surface(ISO, *BOX), got, "second extraction")
    sim.phase("grid")
    assert_same_mesh(sim.extract_surface(ISO, *BOX), got, "after sph_phase_grid")
    sim.phase("density")
    with pytest.raises(sph.SphError, match=r"\(-4\)"):       # an open phase-split step
        sim.extract_surface(ISO, *BOX)
    sim.phase("force")
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.extract_surface(ISO, *BOX)
    sim.phase("readback")
    after = sim.extract_surface(ISO, *BOX)
    assert_same_mesh(after, restate(sim.sample_field("density", *BOX), *BOX[:2], ISO), "after the phase-split step")
    assert after["vertices"].shape != got["vertices"].shape or not np.array_equal(bits(after["vertices"]), bits(got["vertices"]))
    sim.close()


def test_error_codes():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):       # SPH_ESTATE: before any state
        sim.extract_surface(ISO, *BOX)
    assert sim._L.sph_surface_host(sim._h, None, None, None, None) == -4
    sim.setup()
    nan, inf = float("nan"), float("inf")
    ok = dict(iso=1.0, origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1), shape=(2, 2, 2))
    bad = [dict(shape=(1, 2, 2)), dict(shape=(2, 1, 2)), dict(shape=(2, 2, 1)), dict(shape=(0, 2, 2)), dict(shape=(2, 2, 4097)),
           dict(shape=(-1, 2, 2)), dict(shape=(4096, 4096, 2)), dict(shape=(257, 256, 256)),
           dict(origin=(nan, 0, 0)), dict(origin=(0, inf, 0)), dict(origin=(0, 0, -inf)),
           dict(spacing=(0.0, 0.1, 0.1)), dict(spacing=(0.1, -0.1, 0.1)), dict(spacing=(0.1, 0.1, nan)), dict(spacing=(inf, 0.1, 0.1)),
           dict(iso=0.0), dict(iso=-1.0), dict(iso=nan), dict(iso=inf)]
    for b in bad:
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.extract_surface(**{**ok, **b})
    opt = _lib.SphSurfaceOptions()                           # struct_size left at 0
    assert sim._L.sph_extract_surface(sim._h, C.byref(opt)) == -1
    assert sim._L.sph_extract_surface(sim._h, None) == -1
    # 1 << 24 points: allowed, as a cube and as 1 << 23 rows of two points
    for shape, spacing in (((256, 256, 256), 10.0 / 255), ((4096, 2048, 2), (5.0, 10.0 / 2047, 10.0 / 4095))):
        mesh = sim.extract_surface(1.0, (0.0, 0.0, 0.0), spacing, shape)
        assert len(mesh["triangles"]) > 100 and mesh["triangles"].max() == len(mesh["vertices"]) - 1
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = make(4096, **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        with pytest.raises(sph.SphError, match=r"\(-4\)"):
            other.extract_surface(**ok)
        other.close()


def test_empty_meshes_and_the_time_is_counted(monkeypatch):
    empty = make(0)
    empty.setup()
    mesh = empty.extract_surface(ISO, *BOX)
    assert mesh["vertices"].shape == (0, 3) and mesh["triangles"].shape == (0, 3)
    assert mesh["vertices"].dtype == F and mesh["triangles"].dtype == np.uint32
    empty.close()
    sim = make(4096)
    sim.setup()
    top = float(sim.sample_field("density", *BOX).max())
    assert top > ISO
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_SURFACE_PLAIN", plain)
        mesh = sim.extract_surface(2 * top, *BOX)            # above the field's maximum
        assert mesh["vertices"].shape == (0, 3) and mesh["triangles"].shape == (0, 3)
        nv, nt = C.c_int64(-1), C.c_int64(-1)
        assert sim._L.sph_surface_host(sim._h, None, C.byref(nv), None, C.byref(nt)) == 0 and (nv.value, nt.value) == (0, 0)
    sim.surface_time(reset=True)
    for k in range(3):
        assert len(sim.extract_surface(ISO, *BOX)["triangles"]) > 0
    sample, extract, calls = sim.surface_time(reset=True)
    assert calls == 3 and 0.0 < sample < 1.0 and 0.0 < extract < 1.0
    assert sim.surface_time() == (0.0, 0.0, 0)
    # the defaults of the Python front end: one cell at the origin
    assert sim.extract_surface(ISO)["triangles"].shape[1] == 3
    sim.close()


def read_ply(path):
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    header = blob[:end].decode().split("\n")
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert header[3:6] == ["property float x", "property float y", "property float z"]
    assert header[7] == "property list uchar int vertex_indices"
    nv, nt = int(header[2].split()[-1]), int(header[6].split()[-1])
    assert header[2] == f"element vertex {nv}" and header[6] == f"element face {nt}"
    assert len(blob) == end + 12 * nv + 13 * nt
    verts = np.frombuffer(blob, "<f4", 3 * nv, end).reshape(nv, 3)
    faces = np.frombuffer(blob, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nt, end + 12 * nv)
    assert (faces["n"] == 3).all()
    return {"vertices": verts, "triangles": faces["v"].astype(np.uint32)}, blob


def run_cli(out, **env_extra):
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_FREE_SLICE", "SPH_SWEEP", "SPH_SURFACE_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": "2", "SPH_FREE_FRAMES_DIR": str(out), "SPH_FREE_SURFACE": str(ISO), **env_extra})
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_free_surface(tmp_path):
    blobs = {}
    for plain in ("0", "1"):
        out = tmp_path / plain
        out.mkdir()
        r = run_cli(out, SPH_SURFACE_PLAIN=plain, SPH_STEP_TRACE="1")
        assert sorted(os.listdir(out)) == ["frame_0000.ppm", "frame_0001.ppm", "surface_0000.ply", "surface_0001.ply"]
        want = "2 extractions by the lane-exchange path, 0 by the plain path" if plain == "0" else "0 extractions by the lane-exchange path, 2 by the plain path"
        assert want in r.stderr, r.stderr
        mesh, blobs[plain] = read_ply(out / "surface_0001.ply")
    assert blobs["0"] == blobs["1"]
    sim = make(4096)
    sim.setup()
    for _ in range(2):
        sim.simulate()
    sp = float(F(sim.settings.boxDim) / F(100))
    want = sim.extract_surface(ISO, (0.0, 0.0, 0.0), sp, (101, 101, 101))
    sim.close()
    assert len(want["triangles"]) > 0
    assert_same_mesh(mesh, want, "surface_0001.ply")


def test_cli_with_the_linked_sweep_writes_frames_and_no_surfaces(tmp_path):
    r = run_cli(tmp_path, SPH_SWEEP="linked")
    assert "extractSurface" in r.stderr and "SPH_SWEEP_LINKED" in r.stderr
    assert r.stderr.count("extractSurface") == 1
    assert sorted(os.listdir(tmp_path)) == ["frame_0000.ppm", "frame_0001.ppm"]
