"""The liquid frame on the GPU against its numpy restatement (tests/liquid_frame_restatement.py), fed by
sph_download_state.  Every comparison is exact: front words, smoothed-depth bits, normal bits, column words and
RGB, no tolerance anywhere."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import column_frame_restatement as CF
import field_frame_restatement as FF
import grid_states as G
import liquid_frame_restatement as LF
import render_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
EMPTY = LF.EMPTY
# 64 x 48: every workgroup's hull fits the LDS tile; 800 x 600: a 1024-row workgroup of these few thousand particles
# spans far more than a tile, every workgroup issues the per-hit atomics; one odd size; two images smaller than one
# 64 x 4 smoothing rectangle, the second smaller than the halo as well
SIZES = [dict(width=64, height=48), dict(width=800, height=600), dict(width=333, height=77), dict(width=5, height=3),
         dict(width=1, height=1)]
SPLATS = {}   # the restatement's splatted buffers per (state, radius, size): the options of a test only differ behind them


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def golden(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    return data["pos_1"], data["vel_1"]


def from_golden(name, steps, settings=None, **kw):
    pos, vel = golden(name)
    sim = sph.Simulator(settings, **kw) if settings is not None else make(len(pos), **kw)
    sim.upload_state(pos, vel)
    for _ in range(steps):
        sim.simulate()
    return sim


def gpu_liquid(sim, **opt):
    sim.render_liquid(**opt)
    out = sim.liquid_buffers()
    out["rgb"] = np.array(sim.frame_host(), copy=True)
    return out


def assert_liquid_equal(got, want, what):
    for k in ("front", "column", "smooth", "normals", "rgb"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.dtype == F:
            a, b = a.view(np.uint32), b.view(np.uint32)   # the bits: -0 is not +0
        bad = a != b
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {a.size} entries differ, first at {np.argwhere(bad)[0]}"


def restate(sim, st, **opt):
    s = sim.settings
    opt = dict(opt)
    opt["width"], opt["height"] = opt.get("width") or 800, opt.get("height") or 600
    want = LF.render_liquid(st["pos"], s.h, s.d_kernel_coeff, cache=SPLATS, **opt)
    assert want["border"] == 0, "a contribution on the border of the restatement's box"
    return want


def check(sim, what, st=None, **opt):
    """render with `opt`, compare everything with the restatement of the downloaded state"""
    st = st or sim.download_state()
    got = gpu_liquid(sim, **opt)
    want = restate(sim, st, **opt)
    assert_liquid_equal(got, want, f"{what} {opt}")
    # the automatic scale is the value of the largest word the device itself splatted
    assert want["scale"] == CF.value(got["column"].max(initial=0)) or opt.get("thickness_scale")
    return got


@pytest.fixture(scope="module")
def stepped():
    """random4096 + 3 steps: the state most tests share (nothing renders into the state)"""
    sim = from_golden("random4096", 3)
    st = sim.download_state()
    yield sim, st
    sim.close()


@pytest.mark.parametrize("steps", [0, 3])
def test_paths_tile_fallback_and_plain(steps, monkeypatch):
    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = from_golden("random4096", steps)
    st = sim.download_state()
    tiled = [check(sim, f"random4096 + {steps} steps", st, **size) for size in SIZES]
    assert all((t["front"] != EMPTY).any() for t in tiled[:3])
    big = tiled[1]
    assert (big["smooth"] != big["front"]).any(), "the smoothing moved nothing: it is not covered"
    sim.close()
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    twin = from_golden("random4096", steps)  # a fresh handle: nothing of the tiled frames is left in its buffers
    for size, a in zip(SIZES, tiled):
        assert_liquid_equal(gpu_liquid(twin, **size), a, f"plain vs tiled, {steps} steps {size}")
    twin.close()


def test_contention_in_the_dense_block():
    sim = from_golden("dense4096", 5)
    st = sim.download_state()
    for size in SIZES[:2]:
        check(sim, "dense4096 + 5 steps", st, **size)
    hits = np.zeros(800 * 600, np.int64)
    CF.column_buffer(st["pos"], sim.settings.h, sim.settings.d_kernel_coeff, 800, 600, hits=hits)
    assert hits.max() > 100, f"only {hits.max()} particles on the busiest pixel: contention is not covered"
    sim.close()


def test_lattice():
    sim = make(2048, random=False)
    sim.setup()
    for _ in range(2):
        sim.simulate()
    st = sim.download_state()
    for size in SIZES[:3]:
        check(sim, "grid2048 + 2 steps", st, **size)
    sim.close()


@pytest.mark.parametrize("n", [1, 1000])
def test_particle_counts(n):
    # 1000: not a multiple of the 1024-row workgroup, nor of the 256-row one of the check path
    sim = make(n)
    sim.setup()
    for _ in range(2):
        sim.simulate()
    st = sim.download_state()
    for size in SIZES[:3]:
        got = check(sim, f"n = {n}", st, **size)
    assert (got["front"] != EMPTY).any() or n == 1
    sim.close()
    if n == 1:   # ... and the one particle on the axis of a 33 x 33 image: exactly the centre pixel
        sim = make(1)
        sim.upload_state(np.array([[5, 5, 5]], F), np.zeros((1, 3), F))
        got = check(sim, "one particle on the axis", width=33, height=33)
        assert np.argwhere(got["front"] != EMPTY).tolist() == [[16, 16]]
        assert got["normals"][16, 16].tolist() == [0, 0, 1]
        sim.close()


def test_other_h(monkeypatch):
    # h = 0.2 on 50 cells: spheres twice as wide, a radius hard-coded for h = 0.1 misses their rim
    pos, _ = golden("random4096")
    s = G.settings_for(len(pos), 0.2, 50, factory=sph.default_settings)
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_RENDER_PLAIN", plain)
        sim = from_golden("random4096", 0, settings=s)
        st = sim.download_state()
        for size in SIZES[:3]:
            got = check(sim, f"h = 0.2, plain={plain}", st, **size)
        narrow = LF.front_buffer(st["pos"], 0.1, 333, 77)[0]
        assert ((got["front"] != EMPTY) & (narrow == EMPTY)).any()   # pixels only the wider spheres reach
        sim.simulate()
        sim.simulate()
        check(sim, f"h = 0.2 + 2 steps, plain={plain}", **SIZES[0])
        sim.close()


def test_radius(stepped, monkeypatch):
    sim, st = stepped
    h = sim.settings.h
    for size in SIZES[:3]:
        half = check(sim, "radius 0.5 h", st, radius=0.5 * h, **size)
        full = check(sim, "radius h, spelled out", st, radius=h, **size)
    assert (half["front"] != EMPTY).sum() < (full["front"] != EMPTY).sum()
    assert np.array_equal(half["column"], full["column"])   # the column words keep h
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    twin = from_golden("random4096", 3)
    assert_liquid_equal(gpu_liquid(twin, radius=0.5 * h, **SIZES[2]), half, "plain, radius 0.5 h")
    twin.close()


def test_smoothing_options(stepped):
    sim, st = stepped
    size = SIZES[2]
    base = check(sim, "defaults", st, **size)
    seen = {}
    for it in (0, 1, 8):
        for k in (0, 1, 7):
            got = check(sim, "smoothing", st, smooth_iterations=it, smooth_radius=k, **size)
            seen[it, k] = got["smooth"]
            assert np.array_equal(got["front"], base["front"])
            if it == 0 or k == 0:
                assert np.array_equal(got["smooth"], got["front"])
    assert (seen[1, 1] != base["front"]).any() and (seen[8, 7] != seen[1, 7]).any() and (seen[1, 7] != seen[1, 1]).any()
    # delta below every difference of two neighbours' depths blends nothing; far above all of them: everything in reach
    none = check(sim, "tiny delta", st, smooth_depth=1e-12, **size)
    assert np.array_equal(none["smooth"], none["front"])
    every = check(sim, "huge delta", st, smooth_depth=1e6, smooth_iterations=8, smooth_radius=7, **size)
    v, f = every["smooth"][every["smooth"] != EMPTY].view(F), every["front"][every["front"] != EMPTY].view(F)
    assert v.std() < 0.5 * f.std()
    check(sim, "800 x 600, k = 7", st, smooth_iterations=1, smooth_radius=7, **SIZES[1])   # (many rectangles, the widest halo)
    check(sim, "smaller than the halo", st, smooth_iterations=8, smooth_radius=7, **SIZES[3])


def test_thickness_scale_and_light(stepped):
    sim, st = stepped
    for size in SIZES[1:3]:
        auto = check(sim, "automatic scale", st, **size)
        top = float(CF.value(auto["column"].max()))
        assert top > 0
        same = check(sim, "the automatic scale, given", st, thickness_scale=top, **size)
        assert np.array_equal(same["rgb"], auto["rgb"])
        thin = check(sim, "a scale 100 times the largest column", st, thickness_scale=100 * top, **size)
        thick = check(sim, "a scale of a hundredth of it", st, thickness_scale=0.01 * top, **size)
        water = (auto["front"] != EMPTY) & (auto["column"] != 0) & ~((R.edge_buffer(**size) != EMPTY))
        assert (thin["rgb"][water].astype(int) >= thick["rgb"][water].astype(int)).all()
        assert (thin["rgb"][water][:, 0] > thick["rgb"][water][:, 0]).any()
        for light in ((1.0, 0.0, 0.0), (0.0, -3.0, 0.25), (0.0, 0.0, 1e-3)):
            lit = check(sim, "light", st, light=light, **size)
            assert (lit["rgb"] != auto["rgb"]).any() and np.array_equal(lit["normals"], auto["normals"])
        again = check(sim, "the default light, spelled out", st, light=LF.DEFAULT_LIGHT, **size)
        assert np.array_equal(again["rgb"], auto["rgb"])


def test_column_words_are_the_column_frames(stepped):
    sim, st = stepped
    for size in SIZES[:3]:
        liquid = gpu_liquid(sim, **size)
        sim.render_column(**size)
        assert np.array_equal(liquid["column"], sim.column_buffer()), size
        with pytest.raises(sph.SphError, match=r"\(-4\).*liquid"):
            sim.liquid_buffers()


def test_no_readback_linked_and_morton_handles():
    twin = make(4096)
    dark = make(4096, flags=_lib.SPH_FLAG_NO_READBACK)
    for s in (twin, dark):
        s.setup()
        for _ in range(4):
            s.simulate()
    st = twin.download_state()
    for size in SIZES[:2]:
        check(dark, "no-read-back handle", st, **size)
        check(twin, "its twin", st, **size)
    twin.close()
    dark.close()
    for kw in (dict(sweep="linked"), dict(sweep="direct", key_order="morton"), dict(sweep="direct"), dict(sweep="lds")):
        sim = make(4096, **kw)
        sim.setup()
        for _ in range(3):
            sim.simulate()
        st = sim.download_state()
        for size in SIZES[:2]:
            check(sim, str(kw), st, **size)
        sim.close()


def test_other_frame_kinds_after_a_liquid_frame(stepped):
    sim, st = stepped
    for opt in (dict(), dict(width=64, height=48), dict(width=333, height=77)):
        size = dict(width=opt.get("width", 800), height=opt.get("height", 600))
        check(sim, "liquid first", st, **opt)
        with pytest.raises(sph.SphError, match=r"\(-4\).*liquid"):   # no point depth or count behind a liquid frame
            sim.frame_buffers()
        for call in (sim.field_buffer, sim.field_range, sim.column_buffer, sim.column_range):
            with pytest.raises(sph.SphError, match=r"\(-4\)"):
                call()
        for shade in ("flat", "count"):
            rgb = sim.render(shade=shade, **opt)
            got = sim.frame_buffers()
            want = R.render(st["pos"], shade=shade, **size)
            assert np.array_equal(rgb, want["rgb"]), f"{shade} {opt}"
            for k in ("depth", "count", "edge"):
                assert np.array_equal(got[k], want[k]), f"{shade} {k} {opt}"
            with pytest.raises(sph.SphError, match=r"\(-4\).*liquid"):
                sim.liquid_buffers()
            check(sim, f"liquid after {shade}", st, **opt)
        sim.render_field(field="speed", **opt)
        got = dict(rgb=np.array(sim.frame_host(), copy=True), value=sim.field_buffer(), range=sim.field_range())
        got.update(sim.frame_buffers())
        want = FF.render_field(st["pos"], st["vel"], st["rho"], "speed", **size)
        for k in ("edge", "count", "depth", "value", "rgb"):
            assert np.array_equal(got[k], want[k]), f"field {k} {opt}"
        assert np.array(got["range"], F).view(np.uint32).tolist() == np.array(want["range"], F).view(np.uint32).tolist()
        with pytest.raises(sph.SphError, match=r"\(-4\).*liquid"):
            sim.liquid_buffers()
        check(sim, "liquid after field", st, **opt)
        sim.render_column(**opt)
        s = sim.settings
        want = CF.render_column(st["pos"], s.h, s.d_kernel_coeff, **size)
        assert np.array_equal(sim.column_buffer(), want["column"]) and np.array_equal(np.array(sim.frame_host()), want["rgb"])
        assert np.array(sim.column_range(), F).view(np.uint32).tolist() == np.array(want["range"], F).view(np.uint32).tolist()


def test_a_liquid_frame_leaves_the_run_alone_and_is_timed():
    sims = [make(4096), make(4096)]
    for s in sims:
        s.setup()
        s.simulate()
    sims[0].render_time(reset=True)
    sims[0].render_liquid()
    sims[0].render_liquid(width=64, height=48)
    sims[0].render_frame()
    sec, frames = sims[0].render_time(reset=True)
    assert frames == 3 and 0.0 < sec < 1.0
    sims[0].render_liquid()
    for s in sims:
        s.simulate()
    a, b = (s.download_state() for s in sims)
    for k in ("pos", "vel", "rho"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # NULL options: 800 x 600, every default; NULL buffers: nothing is written
    assert sims[0]._L.sph_render_liquid(sims[0]._h, None) == 0
    got = sims[0].liquid_buffers()
    got["rgb"] = np.array(sims[0].frame_host(), copy=True)
    assert_liquid_equal(got, restate(sims[0], a), "NULL options")
    assert sims[0]._L.sph_download_liquid_buffers(sims[0]._h, None, None, None, None) == 0
    for s in sims:
        s.close()


def test_error_paths():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):   # SPH_ESTATE: no state yet
        sim.render_liquid()
    sim.setup()
    h = sim.settings.h
    nan, inf = float("nan"), float("inf")
    for bad in (dict(width=4097), dict(height=-5), dict(width=-1), dict(radius=-0.05), dict(radius=1.01 * h), dict(radius=nan),
                dict(radius=inf), dict(smooth_iterations=9), dict(smooth_iterations=-2), dict(smooth_radius=8),
                dict(smooth_radius=-2), dict(smooth_depth=-1.0), dict(smooth_depth=nan), dict(smooth_depth=inf),
                dict(light=(nan, 0, 1)), dict(light=(0, inf, 1)), dict(light=(0, 0, -inf)), dict(thickness_scale=-1.0),
                dict(thickness_scale=nan), dict(thickness_scale=inf)):
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.render_liquid(**bad)
    o = _lib.SphLiquidFrameOptions()  # struct_size left at 0
    assert sim._L.sph_render_liquid(sim._h, o) == -1
    assert sim._L.sph_render_liquid(None, None) == -1 and sim._L.sph_download_liquid_buffers(None, None, None, None, None) == -1
    with pytest.raises(sph.SphError):    # nothing rendered yet
        sim.liquid_buffers()
    assert sim._L.sph_download_liquid_buffers(sim._h, None, None, None, None) == -4
    sim.render_liquid(radius=h)          # the largest radius
    assert sim.liquid_buffers()["front"].shape == (600, 800)
    for render in (sim.render_frame, sim.render_field, sim.render_column):   # the liquid buffers are gone
        sim.render_liquid(width=64, height=48)
        assert sim.liquid_buffers()["normals"].shape == (48, 64, 3)
        render()
        with pytest.raises(sph.SphError, match=r"\(-4\).*liquid"):
            sim.liquid_buffers()
    sim.close()
    slab = make(4096, flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096)
    with pytest.raises(sph.SphError, match=r"\(-4\).*slab"):
        slab.render_liquid()
    slab.close()


def test_cli_free_shade_liquid(tmp_path):
    env = dict(os.environ)
    env.update({"SPH_FREE_FRAMES": "4", "SPH_FREE_FRAMES_DIR": str(tmp_path), "SPH_PRINT_SHA256": "1", "SPH_FREE_SHADE": "liquid"})
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(tmp_path))
    assert names == ["frame_%04d.ppm" % f for f in range(4)]
    blob = open(os.path.join(tmp_path, names[-1]), "rb").read()
    header = b"P6\n800 600\n255\n"
    assert blob.startswith(header) and len(blob) == len(header) + 1440000
    last = np.frombuffer(blob[len(header):], np.uint8).reshape(600, 800, 3)
    assert "SPH_FREE_SHADE" not in r.stderr
    # the Python binding reproduces the state the CLI printed, and the last frame is the restatement of that state
    sim = make(4096)
    sim.setup()
    for _ in range(4):
        sim.simulate()
    host = np.array(sim.getPosition(), copy=True)
    printed = re.search(r"positions_sha256 ([0-9a-f]{64})", r.stdout).group(1)
    assert hashlib.sha256(host.tobytes()).hexdigest() == printed
    st = sim.download_state()
    want = restate(sim, st)["rgb"]
    sim.close()
    assert np.array_equal(last, want)
