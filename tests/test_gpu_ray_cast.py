"""Ray casting and the view frame on the GPU (rays.hip) against their numpy restatement (tests/ray_cast_restatement.py),
fed by sph_download_state.  Every comparison is exact: hit words word for word on the default path and on the check
path, view frames byte for byte, no tolerance anywhere.  tests/test_ray_cast_cpu.py holds the restatement's walk to
its brute force and to float64 on the same ray sets (tests/ray_sets.py)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import field_frame_restatement as FF
import grid_states as G
import ray_cast_restatement as RC
import ray_sets as RS
import row_walk_cases as RW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
SPH_EINVAL, SPH_ESTATE = -1, -4
GRIDS = ["D1", "D2", "D3", "D7", "D41", "D102", "D257"]


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def from_golden(name, steps=0, **kw):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    sim = make(len(data["pos_1"]), **kw)
    sim.upload_state(data["pos_1"], data["vel_1"])
    for _ in range(steps):
        sim.simulate()
    return sim


def geometry(sim):
    s = sim.settings
    return float(s.h), int(s.numCellsPerDim), float(s.boxDim)


def cast(sim, rays, radius=0.0):
    return sim.cast_words(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], radius)


def assert_same_words(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} words differ, first at {np.argwhere(bad)[0]}: {got[bad][0]:#x} vs {want[bad][0]:#x}"


def check_casts(sim, what, monkeypatch, radii=(0.0,), sets=None, st=None):
    """every ray set at every radius: the default path against the restatement's brute force over the downloaded
    positions, the check path against the same words.  -> the hits"""
    h, D, box = geometry(sim)
    st = st or sim.download_state()
    sets = sets if sets is not None else RS.ray_sets(st["pos"], h, D, box)
    hits = 0
    for radius in radii:
        for key, rays in sets.items():
            want = RC.brute(st["pos"], rays, h, D, radius)
            for plain in ("0", "1"):
                monkeypatch.setenv("SPH_CAST_PLAIN", plain)
                assert_same_words(cast(sim, rays, radius), want, f"{what}, {key}, radius {radius}, plain={plain}")
            hits += int((want != RC.MISS).sum())
    monkeypatch.setenv("SPH_CAST_PLAIN", "0")
    return hits


def gpu_view(sim, cam, width, height, **opt):
    sim.render_view(cam["eye"], cam["target"], cam["up"], width, height, cam["tan_half"], **opt)
    return dict(rgb=np.array(sim.frame_host(), copy=True), words=sim.view_buffer())


def restate_view(sim, st, cam, width, height, near=0.0, far=0.0, radius=0.0, shade="flat", lo=0.0, hi=0.0, light=(0.0, 0.0, 0.0),
                 edge_radius=0.0, words=None):
    h, D, box = geometry(sim)
    c = RC.camera(cam["eye"], cam["target"], cam["up"], width, height, cam["tan_half"], near, far, h)
    return RC.render_view(st["pos"], st["vel"], st["rho"], h, D, c, radius, shade, lo, hi, light, edge_radius, box, words)


def check_view(sim, st, cam, width, height, what, monkeypatch, words=None, **opt):
    """both paths against the restatement; -> its result"""
    want = restate_view(sim, st, cam, width, height, words=words, **opt)
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_CAST_PLAIN", plain)
        got = gpu_view(sim, cam, width, height, **opt)
        assert_same_words(got["words"], want["words"], f"{what} {width}x{height} {opt}, plain={plain}")
        bad = (got["rgb"] != want["rgb"]).any(axis=2)
        assert not bad.any(), f"{what} {width}x{height} {opt}, plain={plain}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}"
    monkeypatch.setenv("SPH_CAST_PLAIN", "0")
    return want


@pytest.fixture(scope="module")
def stepped():
    """random4096 + 3 steps: the state the view tests share (nothing renders into the state)"""
    sim = from_golden("random4096", 3)
    st = sim.download_state()
    yield sim, st
    sim.close()


# ---- hit words ----

@pytest.mark.parametrize("name", ["random4096", "dense4096", "grid2048"])
def test_goldens(name, monkeypatch):
    sim = from_golden(name)
    h = sim.settings.h
    hits = check_casts(sim, name, monkeypatch, radii=(0.0, float(h)))
    assert hits > 100, f"{name}: only {hits} hits: the rays do not cover the fluid"
    sim.close()


@pytest.mark.parametrize("name", GRIDS)
def test_other_grids(name, monkeypatch):
    pos, vel, g = G.grid_state(name)
    sim = sph.Simulator(G.settings_for(len(pos), g["h"], g["cells"], factory=sph.default_settings))
    sim.upload_state(pos, vel)
    hits = check_casts(sim, name, monkeypatch, radii=(0.0, float(F(g["h"]))))
    assert hits > 0, name
    sim.close()


def test_across_a_step_and_after_a_click(monkeypatch):
    sim = from_golden("random4096")
    h, D, box = geometry(sim)
    rays = RS.camera_rays(RS.cameras(None, box)["oblique"], 64, 48, h)
    first = cast(sim, rays)
    assert_same_words(first, RC.brute(sim.download_state()["pos"], rays, h, D), "before the step")
    for k in range(2):
        sim.simulate()
        assert check_casts(sim, f"after step {k + 1}", monkeypatch, sets={"oblique": rays}) > 100
    assert (cast(sim, rays) != first).any(), "the particles did not move under the rays"
    sim.moveParticles((400, 300))
    check_casts(sim, "after a click", monkeypatch, sets={"oblique": rays})   # (a click changes velocities only)
    sim.simulate()
    check_casts(sim, "a step after the click", monkeypatch, sets={"oblique": rays})
    sim.close()


def test_rows_outside_the_grid_and_no_particles(monkeypatch):
    """D1 after one step: the walls have put every row at a coordinate of h or beyond, outside the one cell, where the
    grid build keys it to the clamped cell: the walk finds the rows and must not take them."""
    pos, vel, g = RW.walls("D1")
    h, D = g["h"], g["cells"]
    sim = sph.Simulator(G.settings_for(len(pos), h, D, factory=sph.default_settings))
    sim.upload_state(pos, vel)
    inside = RC.make_rays(pos + F(0.3 * h), np.tile(F([-1, -1, -1]), (len(pos), 1)))
    assert check_casts(sim, "D1 before the step", monkeypatch, radii=(0.0, float(F(h))), sets={"at the rows": inside}) > 0
    sim.simulate()
    st = sim.download_state()
    p = st["pos"]
    assert ((p < 0) | (p / F(h) >= D)).any(axis=1).all(), "premise: D1's step leaves no particle inside"
    sets = RS.ray_sets(p, h, D, float(sim.settings.boxDim))
    sets["at the rows"] = RC.make_rays(p + F(0.3 * h), np.tile(F([-1, -1, -1]), (len(p), 1)))
    assert check_casts(sim, "D1 after a step", monkeypatch, radii=(0.0, float(F(h))), sets=sets, st=st) == 0
    sim.cast_stats(reset=True)
    cast(sim, sets["at the rows"], float(F(h)))
    assert sim.cast_stats()["tests"] >= len(p), "the walk did not meet the rows in their clamped cell"
    assert sim.download_grid()["cells"].tolist() == [[0, len(pos)]]
    sim.close()
    box = 10.0
    empty = make(0)
    empty.setup()
    rays = RS.random_rays(65, box, 3)
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_CAST_PLAIN", plain)
        assert (cast(empty, rays) == RC.MISS).all()
        t, ids = empty.cast_rays(rays[:, 0:3], rays[:, 4:7])
        assert np.isinf(t).all() and (ids == -1).all()
        assert len(cast(empty, rays[:0])) == 0
        empty.render_view((5, 5, 15), (5, 5, 0), width=5, height=3, edge_radius=-1.0)
        assert not empty.frame_host().any() and (empty.view_buffer() == RC.MISS).all()
    empty.close()


def test_fast_math_handle_gives_the_same_words(monkeypatch):
    strict, fast = from_golden("random4096", 1), from_golden("random4096", 0, math="fast")
    st = strict.download_state()
    fast.upload_state(st["pos"], st["vel"])
    h, D, box = geometry(strict)
    sets = RS.ray_sets(st["pos"], h, D, box, sizes=RS.SIZES[:1])
    check_casts(fast, "fast math", monkeypatch, sets=sets, st=fast.download_state())
    for key, rays in sets.items():
        assert_same_words(cast(fast, rays), cast(strict, rays), "fast against strict, " + key)
    strict.close()
    fast.close()


# ---- view frames ----

@pytest.mark.parametrize("camera", ["reference", "oblique", "inside"])
def test_views(stepped, camera, monkeypatch):
    sim, st = stepped
    h, D, box = geometry(sim)
    cam = RS.cameras(st["pos"], box)[camera]
    filled = 0
    for (w, hh) in RS.SIZES:
        want = check_view(sim, st, cam, w, hh, camera, monkeypatch)
        filled += int((want["words"] != RC.MISS).sum())
    assert filled > 50, camera


def test_every_shade_and_range_draws_its_own_picture(monkeypatch):
    """dense4096 after five steps, seen from nearby with the near plane inside the block: speeds, densities and pressures
    differ from particle to particle (on its surface alone the pressure is 0 everywhere).  The flat shade ignores the
    range; every field shade draws one picture over the automatic range and another over the middle half of it: seven
    pictures, no two the same."""
    sim = from_golden("dense4096", 5)
    st = sim.download_state()
    cam = dict(eye=(5.1, 1.9, 5.3), target=(4.2, 1.2, 4.2), up=(0.0, 1.0, 0.0), tan_half=(0.0, 0.0))
    words = restate_view(sim, st, cam, 64, 48, near=1.5)["words"]
    winners = RC.split(words.reshape(-1))[1]
    winners = winners[winners >= 0]
    assert len(winners) > 300
    seen = {}
    for shade in ("flat", "speed", "density", "pressure"):
        ranges = [(0.0, 0.0)]
        if shade != "flat":
            s = FF.scalar(st["vel"], st["rho"], shade)
            assert len(np.unique(s[winners])) > 50, f"premise: the {shade} of the spheres in sight varies"
            quarter = F(0.25) * (s.max() - s.min())
            ranges.append((float(s.min() + quarter), float(s.max() - quarter)))   # the middle half of the field's range
        for lo, hi in ranges:
            want = check_view(sim, st, cam, 64, 48, "shades", monkeypatch, words=words, near=1.5, shade=shade, lo=lo, hi=hi)
            seen.setdefault(want["rgb"].tobytes(), []).append((shade, lo, hi))
    assert len(seen) == 7, [v for v in seen.values() if len(v) > 1]
    sim.close()


def test_view_lights_edges_radius_and_window(stepped, monkeypatch):
    sim, st = stepped
    h, D, box = geometry(sim)
    cam = RS.cameras(st["pos"], box)["oblique"]
    words = restate_view(sim, st, cam, 64, 48)["words"]
    seen = {check_view(sim, st, cam, 64, 48, "default light", monkeypatch, words=words)["rgb"].tobytes()}
    for light in ((1.0, 0.2, -0.3), (0.0, -2.0, 0.0)):
        want = check_view(sim, st, cam, 64, 48, "lights", monkeypatch, words=words, light=light)
        assert want["rgb"].tobytes() not in seen
        seen.add(want["rgb"].tobytes())
    plain = check_view(sim, st, cam, 64, 48, "no edges", monkeypatch, words=words, edge_radius=-1.0)
    thick = check_view(sim, st, cam, 64, 48, "thick edges", monkeypatch, words=words, edge_radius=0.05 * box)
    white = (thick["rgb"] == 255).all(axis=2)
    assert white.any() and not (plain["rgb"] == 255).all(axis=2).any() and (thick["rgb"][~white] == plain["rgb"][~white]).all()
    # the radius of the spheres and a window
    check_view(sim, st, cam, 64, 48, "radius h", monkeypatch, radius=float(sim.settings.h))
    check_view(sim, st, cam, 64, 48, "window", monkeypatch, near=0.9 * box, far=1.3 * box)


def test_an_edge_at_the_hits_depth_wins(monkeypatch):
    """tests/test_ray_cast_cpu.py's exact tie, on the device: through a 1 x 1 view from (0, 5, 15) down -z the sphere of
    radius 0.0625 at (0, 5, 9.96875) and the edge of radius 0.03125 along y through (0, 10) are both entered at 4.96875.
    The edge wins the tie and where the sphere lies one ulp further; the sphere where it lies one ulp nearer."""
    sim = make(1)
    cam = dict(eye=(0.0, 5.0, 15.0), target=(0.0, 5.0, 0.0), up=(0.0, 1.0, 0.0), tan_half=(2.0, 2.0))
    z = F(9.96875)
    pictures = []
    for zz in (np.nextafter(z, F(0)), z, np.nextafter(z, F(20))):
        sim.upload_state(np.array([[0.0, 5.0, zz]], F), np.zeros((1, 3), F))
        st = sim.download_state()
        want = check_view(sim, st, cam, 1, 1, f"z = {zz!r}", monkeypatch, radius=0.0625, edge_radius=0.03125)
        t = RC.split(want["words"].reshape(-1))[0][0]
        pictures.append((float(t), want["rgb"][0, 0].tolist()))
        bare = check_view(sim, st, cam, 1, 1, f"z = {zz!r}, no edges", monkeypatch, radius=0.0625, edge_radius=-1.0)
    ulp = float(np.spacing(z))
    assert [t for t, _ in pictures] == [4.96875 + ulp, 4.96875, 4.96875 - ulp]
    assert pictures[0][1] == pictures[1][1] == [255, 255, 255] and pictures[2][1] == bare["rgb"][0, 0].tolist() != [255, 255, 255]
    sim.close()


def test_the_state_and_the_other_frames_are_left_alone(monkeypatch):
    def run(between):
        sim = from_golden("random4096", 2)
        frames = {}
        if between:
            h, D, box = geometry(sim)
            cam = RS.cameras(None, box)["oblique"]
            cast(sim, RS.camera_rays(cam, 64, 48, h))
            gpu_view(sim, cam, 64, 48, shade="speed")
            L, hd = sim._L, sim._h
            u32 = (C.c_uint32 * (64 * 48))()
            u64 = (C.c_uint64 * (64 * 48))()
            lo = C.c_float()
            assert L.sph_download_frame_buffers(hd, u32, None, None) == SPH_ESTATE
            assert L.sph_download_field_buffer(hd, u32) == SPH_ESTATE and L.sph_field_range(hd, C.byref(lo), None) == SPH_ESTATE
            assert L.sph_download_column_buffer(hd, u64) == SPH_ESTATE and L.sph_column_range(hd, C.byref(lo), None) == SPH_ESTATE
            assert L.sph_download_liquid_buffers(hd, u32, None, None, None) == SPH_ESTATE
            assert L.sph_download_view_buffer(hd, u64) == 0
        size = dict(width=64, height=48)
        frames["flat"] = sim.render(**size).tobytes()
        if between:
            assert sim._L.sph_download_view_buffer(sim._h, (C.c_uint64 * (64 * 48))()) == SPH_ESTATE
            gpu_view(sim, RS.cameras(None, 10.0)["reference"], 64, 48)
        sim.render_field("speed", **size)
        frames["field"] = sim.frame_host().tobytes() + sim.field_buffer().tobytes()
        if between:
            gpu_view(sim, RS.cameras(None, 10.0)["reference"], 64, 48)
        sim.render_column(**size)
        frames["column"] = sim.frame_host().tobytes() + sim.column_buffer().tobytes()
        if between:
            gpu_view(sim, RS.cameras(None, 10.0)["reference"], 64, 48)
        sim.render_liquid(**size)
        frames["liquid"] = sim.frame_host().tobytes() + sim.liquid_buffers()["smooth"].tobytes()
        sec, count = sim.render_time()
        assert count == (8 if between else 4) and sec > 0
        sim.simulate()
        sha = hashlib.sha256(sim.download_state()["pos"].tobytes()).hexdigest()
        sim.close()
        return frames, sha

    assert run(True) == run(False)


# ---- refusals and stats ----

def test_refusals(monkeypatch):
    monkeypatch.setenv("SPH_CAST_PLAIN", "0")
    sim = make(4096)
    L, hd = sim._L, sim._h
    rays = np.zeros(4, _lib.ray_dtype())
    rp = rays.ctypes.data_as(C.POINTER(_lib.SphRay))

    def copt(radius=0.0, size=C.sizeof(_lib.SphCastOptions)):
        return C.byref(_lib.SphCastOptions(size, radius))

    def vopt(**kw):
        o = _lib.SphViewOptions()
        o.struct_size = C.sizeof(_lib.SphViewOptions)
        o.width, o.height = 5, 3
        o.eye[:], o.target[:], o.up[:] = (5, 5, 15), (5, 5, 0), (0, 1, 0)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[:] = v
            else:
                setattr(o, k, v)
        return C.byref(o)

    assert L.sph_cast_rays(hd, rp, 4, None) == SPH_ESTATE and L.sph_render_view(hd, vopt()) == SPH_ESTATE   # before any state
    assert L.sph_cast_host(hd, None, None) == SPH_ESTATE
    sim.setup()
    assert L.sph_cast_host(hd, None, None) == SPH_ESTATE
    hh = float(sim.settings.h)
    for bad in (float("nan"), float("inf"), -1.0, 1.5 * hh, float(np.nextafter(F(hh), F(1)))):
        assert L.sph_cast_rays(hd, rp, 4, copt(bad)) == SPH_EINVAL, bad
        assert L.sph_render_view(hd, vopt(radius=bad)) == SPH_EINVAL, bad
    assert L.sph_cast_rays(hd, rp, 4, copt(size=0)) == SPH_EINVAL
    for m in (-1, (1 << 24) + 1):
        assert L.sph_cast_rays(hd, rp, m, None) == SPH_EINVAL, m
    assert L.sph_cast_rays(hd, None, 4, None) == SPH_EINVAL
    assert L.sph_render_view(hd, None) == SPH_EINVAL and L.sph_render_view(hd, vopt(struct_size=0)) == SPH_EINVAL
    nan = float("nan")
    for kw in (dict(target=(5, 5, 15)), dict(up=(0, 0, -1)), dict(up=(0, 0, 0)), dict(eye=(nan, 5, 15)), dict(up=(0, nan, 0)),
               dict(target=(float("inf"), 5, 0)), dict(tan_half_x=1.0), dict(tan_half_x=-1.0, tan_half_y=1.0), dict(tan_half_x=1.0, tan_half_y=nan),
               dict(near=-1.0), dict(near=nan), dict(far=-1.0), dict(near=2.0, far=1.0), dict(far=nan), dict(shade=4), dict(shade=-1),
               dict(value_lo=1.0, value_hi=0.5), dict(value_lo=nan), dict(light=(nan, 0, 0)), dict(edge_radius=nan),
               dict(width=0 - 1), dict(width=4097), dict(height=4097)):
        assert L.sph_render_view(hd, vopt(**kw)) == SPH_EINVAL, kw
        assert L.sph_last_error(hd), kw
    assert L.sph_cast_host(hd, None, None) == SPH_ESTATE
    assert L.sph_cast_rays(hd, rp, 4, None) == 0 and L.sph_cast_host(hd, None, None) == 0
    assert L.sph_cast_rays(hd, None, 0, None) == 0
    m = C.c_int(-1)
    assert L.sph_cast_host(hd, None, C.byref(m)) == 0 and m.value == 0
    assert L.sph_render_view(hd, vopt()) == 0
    # the grid phase done by hand is used as it is; an open phase-split step is SPH_ESTATE
    sim.phase("grid")
    assert L.sph_cast_rays(hd, rp, 4, None) == 0 and L.sph_render_view(hd, vopt()) == 0
    for phase in ("density", "force"):
        sim.phase(phase)
        assert L.sph_cast_rays(hd, rp, 4, None) == SPH_ESTATE and L.sph_render_view(hd, vopt()) == SPH_ESTATE
    sim.phase("readback")
    assert L.sph_cast_rays(hd, rp, 4, None) == 0 and L.sph_render_view(hd, vopt()) == 0
    # the check path's limit: rays x particles <= 2^32
    monkeypatch.setenv("SPH_CAST_PLAIN", "1")
    big = np.zeros((1 << 20) + 1, _lib.ray_dtype())
    bp = big.ctypes.data_as(C.POINTER(_lib.SphRay))
    assert L.sph_cast_rays(hd, bp, 1 << 20, None) == 0
    assert L.sph_cast_rays(hd, bp, (1 << 20) + 1, None) == SPH_EINVAL and b"2^32" in L.sph_last_error(hd)
    assert L.sph_render_view(hd, vopt(width=1024, height=1024)) == 0
    assert L.sph_render_view(hd, vopt(width=1025, height=1024)) == SPH_EINVAL and b"2^32" in L.sph_last_error(hd)
    monkeypatch.setenv("SPH_CAST_PLAIN", "0")
    assert L.sph_cast_rays(hd, bp, (1 << 20) + 1, None) == 0
    sim.close()
    for kw in (dict(flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096), dict(sweep="linked"), dict(sweep="direct", key_order="morton")):
        other = make(4096, **kw)
        if not kw.get("flags"):
            other.setup()
            other.simulate()
        assert other._L.sph_cast_rays(other._h, rp, 4, None) == SPH_ESTATE, kw
        assert other._L.sph_last_error(other._h), kw
        assert other._L.sph_render_view(other._h, vopt()) == SPH_ESTATE, kw
        other.close()


def test_stats(monkeypatch):
    monkeypatch.setenv("SPH_CAST_PLAIN", "0")
    sim = from_golden("random4096")
    h, D, box = geometry(sim)
    rays = RS.camera_rays(RS.cameras(None, box)["oblique"], 64, 48, h)
    assert sim.cast_stats() == dict(calls=0, rays=0, layers=0, tests=0, seconds=0.0)
    cast(sim, rays)
    cast(sim, rays[:65])
    cast(sim, rays[:0])
    st = sim.cast_stats()
    n = sim.n
    assert (st["calls"], st["rays"]) == (2, len(rays) + 65) and st["seconds"] > 0
    assert 0 < st["tests"] <= st["rays"] * n and st["tests"] < st["rays"] * n // 50, st
    assert 0 < st["layers"] <= st["rays"] * D
    gpu_view(sim, RS.cameras(None, box)["oblique"], 64, 48)
    both = sim.cast_stats()
    assert (both["calls"], both["rays"]) == (3, 2 * len(rays) + 65) and both["seconds"] == st["seconds"]
    assert sim.cast_stats(reset=True) == both
    assert sim.cast_stats() == dict(calls=0, rays=0, layers=0, tests=0, seconds=0.0)
    monkeypatch.setenv("SPH_CAST_PLAIN", "1")
    cast(sim, rays[:65])
    st = sim.cast_stats()
    assert (st["calls"], st["rays"], st["layers"], st["tests"]) == (1, 65, 0, 65 * n)
    sim.close()


def free_run(tmp_path, frames, view, **more):
    """./sph -n 4096 -i random -m free with SPH_FREE_VIEW=view into tmp_path -> the finished process"""
    env = dict(os.environ)
    for k in ("SPH_FREE_SHADE", "SPH_CAST_PLAIN"):
        env.pop(k, None)
    env.update({"SPH_FREE_FRAMES": str(frames), "SPH_FREE_VIEW": view, "SPH_FREE_FRAMES_DIR": str(tmp_path)}, **more)
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_free_view(tmp_path):
    free_run(tmp_path, 2, "-4,13,9,5,5,5,speed")
    assert sorted(os.listdir(tmp_path)) == ["frame_%04d.ppm" % f for f in range(2)] + ["view_%04d.ppm" % f for f in range(2)]
    sim = make(4096)
    sim.setup()
    for f in range(2):
        sim.simulate()
        sim.render_view((-4, 13, 9), (5, 5, 5), shade="speed")
        want = b"P6\n800 600\n255\n" + sim.frame_host().tobytes()
        assert open(tmp_path / ("view_%04d.ppm" % f), "rb").read() == want, f
        assert (sim.view_buffer() != RC.MISS).any()
    sim.close()


def test_cli_free_view_over_slabs(tmp_path):
    """refused like the other frames: one line, no view files, the run goes on"""
    r = free_run(tmp_path, 2, "-4,13,9,5,5,5", SPH_GPUS="4", SPH_TRANSPORT="loopback")
    assert r.stderr.count("renderView: frames of a multi-GPU run (SPH_GPUS > 1) are not rendered") == 1, r.stderr
    assert not [x for x in os.listdir(tmp_path) if x.startswith("view_")]


@pytest.mark.parametrize("value", ["5,5,15,5,5,0,purple", "5,5,5,5,5,5"])   # an unknown shade; an eye on its target
def test_cli_free_view_bad_value(tmp_path, value):
    """one line, no view, the frames go on"""
    r = free_run(tmp_path, 1, value)
    assert r.stderr.count("SPH_FREE_VIEW=" + value) == 1 and sorted(os.listdir(tmp_path)) == ["frame_0000.ppm"], r.stderr
