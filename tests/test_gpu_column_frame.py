"""The column frame on the GPU against its numpy restatement (tests/column_frame_restatement.py), fed by
sph_download_state.  Every comparison is exact: column words, RGB and the bits of the range, no tolerance
anywhere."""
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
import render_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
# 64 x 48: every workgroup's hull fits the LDS tile; 800 x 600: a 1024-row workgroup of these few thousand particles
# spans far more than a tile, every workgroup issues the per-hit atomics; one odd size
SIZES = [dict(width=64, height=48), dict(width=800, height=600), dict(width=333, height=77)]


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


def gpu_column(sim, **opt):
    sim.render_column(**opt)
    return dict(rgb=np.array(sim.frame_host(), copy=True), column=sim.column_buffer(), range=sim.column_range())


def assert_column_equal(got, want, what):
    for k in ("column", "rgb"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {a.size} entries differ, first at {np.argwhere(bad)[0]}"
    ga, wa = (np.array(x["range"], F).view(np.uint32).tolist() for x in (got, want))
    assert ga == wa, f"{what}: range {got['range']} vs {want['range']}"


def restate(sim, st, **opt):
    s = sim.settings
    want = CF.render_column(st["pos"], s.h, s.d_kernel_coeff, lo=opt.get("lo", 0.0), hi=opt.get("hi", 0.0),
                            width=opt.get("width") or 800, height=opt.get("height") or 600)
    assert want["border"] == 0, "a contribution on the border of the restatement's box"
    return want


def check(sim, what, st=None, **opt):
    """render with `opt`, compare everything with the restatement of the downloaded state"""
    st = st or sim.download_state()
    got = gpu_column(sim, **opt)
    want = restate(sim, st, **opt)
    assert_column_equal(got, want, f"{what} {opt}")
    return got


@pytest.mark.parametrize("steps", [0, 3])
def test_paths_tile_fallback_and_plain(steps, monkeypatch):
    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = from_golden("random4096", steps)
    st = sim.download_state()
    tiled = [check(sim, f"random4096 + {steps} steps", st, **size) for size in SIZES]
    assert all((t["column"] != 0).any() for t in tiled)
    sim.close()
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    twin = from_golden("random4096", steps)  # a fresh handle: nothing of the tiled frames is left in its buffers
    for size, a in zip(SIZES, tiled):
        assert_column_equal(gpu_column(twin, **size), a, f"plain vs tiled, {steps} steps {size}")
    twin.close()


def test_contention_in_the_dense_block():
    sim = from_golden("dense4096", 5)
    st = sim.download_state()
    for size in SIZES[:2]:
        hits = np.zeros(size["width"] * size["height"], np.int64)
        CF.column_buffer(st["pos"], sim.settings.h, sim.settings.d_kernel_coeff, size["width"], size["height"], hits=hits)
        if size["width"] == 800:   # (the block is 0.375 wide: some 100 pixels, several hundred particles on each)
            assert hits.max() > 100, f"only {hits.max()} particles on the busiest pixel: contention is not covered"
        check(sim, "dense4096 + 5 steps", st, **size)
    sim.close()


def test_lattice():
    sim = make(2048, random=False)
    sim.setup()
    for _ in range(2):
        sim.simulate()
    st = sim.download_state()
    for size in SIZES:
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
    for size in SIZES:
        got = check(sim, f"n = {n}", st, **size)
    assert (got["column"] != 0).any() or n == 1
    sim.close()
    if n == 1:   # ... and the one particle on the axis of a 33 x 33 image: exactly the centre pixel
        sim = make(1)
        sim.upload_state(np.array([[5, 5, 5]], F), np.zeros((1, 3), F))
        got = check(sim, "one particle on the axis", width=33, height=33)
        assert np.argwhere(got["column"]).tolist() == [[16, 16]]
        sim.close()


def test_other_h(monkeypatch):
    # h = 0.2 on 50 cells: footprints twice as wide, a radius hard-coded for h = 0.1 misses their rim
    pos, _ = golden("random4096")
    s = G.settings_for(len(pos), 0.2, 50, factory=sph.default_settings)
    ref = sph.default_settings(len(pos), True)
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_RENDER_PLAIN", plain)
        sim = from_golden("random4096", 0, settings=s)
        st = sim.download_state()
        for size in SIZES:
            got = check(sim, f"h = 0.2, plain={plain}", st, **size)
        narrow = CF.column_buffer(st["pos"], ref.h, ref.d_kernel_coeff, 333, 77)[0]
        assert ((got["column"] != 0) & (narrow == 0)).any()   # pixels only the wider footprints reach
        sim.simulate()
        sim.simulate()
        check(sim, f"h = 0.2 + 2 steps, plain={plain}", **SIZES[0])
        check(sim, f"h = 0.2 + 2 steps, plain={plain}", **SIZES[1])
        sim.close()


def test_cap(monkeypatch):
    pos, _ = golden("random4096")
    s = sph.default_settings(len(pos), True)
    s.d_kernel_coeff = float(F(s.d_kernel_coeff) * F(1e6))
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_RENDER_PLAIN", plain)
        sim = from_golden("random4096", 0, settings=s)   # (rendered as uploaded: this coefficient is no fluid to step)
        st = sim.download_state()
        for size in SIZES:
            got = check(sim, f"coefficient x 1e6, plain={plain}", st, **size)
        assert (got["column"] >= np.uint64(1 << 52)).any(), "no capped term: the case is not covered"
        sim.close()
    one = sph.default_settings(2, True)
    one.d_kernel_coeff = s.d_kernel_coeff
    sim = sph.Simulator(one)
    sim.upload_state(np.array([[5, 5, 5], [5, 5, 5]], F), np.zeros((2, 3), F))
    got = check(sim, "two capped terms", width=33, height=33)
    assert int(got["column"][16, 16]) == 1 << 53
    sim.close()


def test_ranges():
    sim = from_golden("random4096", 3)
    st = sim.download_state()
    for size in SIZES[1:]:
        col = CF.column_buffer(st["pos"], sim.settings.h, sim.settings.d_kernel_coeff, size["width"], size["height"])[0]
        v = np.sort(CF.value(col[col != 0]))
        lo, hi = v[len(v) // 4], v[(3 * len(v)) // 4]
        assert v[0] < lo < hi < v[-1], "the columns do not spread over their quartiles: the clipping case is not covered"
        got = check(sim, "both ends clip", st, lo=float(lo), hi=float(hi), **size)
        assert got["range"] == (lo, hi)
        q = FF.quantise(CF.value(col[col != 0]), lo, hi)
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any()
        top = float(v[-1])
        above = check(sim, "range above the data", st, lo=top + 1.0, hi=top + 2.0, **size)
        below = check(sim, "range below the data", st, lo=-2.0, hi=-1.0, **size)
        hit = (col != 0) & (R.edge_buffer(size["width"], size["height"]) == R.EMPTY)
        assert (above["rgb"][hit] == (223, 239, 255)).all() and (below["rgb"][hit] == (0, 48, 128)).all()
        auto = check(sim, "automatic", st, **size)
        assert auto["range"] == (F(0), CF.value(col.max())) and auto["range"][1] > 0
    sim.close()


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


def test_other_frame_kinds_after_a_column_frame():
    sim = from_golden("random4096", 3)
    st = sim.download_state()
    for opt in (dict(), dict(width=64, height=48), dict(width=333, height=77)):
        size = dict(width=opt.get("width", 800), height=opt.get("height", 600))
        check(sim, "column first", st, **opt)
        with pytest.raises(sph.SphError, match=r"\(-4\).*column"):   # no depth or count behind a column frame
            sim.frame_buffers()
        for call in (sim.field_buffer, sim.field_range):
            with pytest.raises(sph.SphError, match=r"\(-4\)"):
                call()
        for shade in ("flat", "count"):
            rgb = sim.render(shade=shade, **opt)
            got = sim.frame_buffers()
            want = R.render(st["pos"], shade=shade, **size)
            assert np.array_equal(rgb, want["rgb"]), f"{shade} {opt}"
            for k in ("depth", "count", "edge"):
                assert np.array_equal(got[k], want[k]), f"{shade} {k} {opt}"
            for call in (sim.column_buffer, sim.column_range):
                with pytest.raises(sph.SphError, match=r"\(-4\)"):
                    call()
            check(sim, f"column after {shade}", st, **opt)
        sim.render_field(field="speed", **opt)
        got = dict(rgb=np.array(sim.frame_host(), copy=True), value=sim.field_buffer(), range=sim.field_range())
        got.update(sim.frame_buffers())
        want = FF.render_field(st["pos"], st["vel"], st["rho"], "speed", **size)
        for k in ("edge", "count", "depth", "value", "rgb"):
            assert np.array_equal(got[k], want[k]), f"field {k} {opt}"
        assert np.array(got["range"], F).view(np.uint32).tolist() == np.array(want["range"], F).view(np.uint32).tolist()
        for call in (sim.column_buffer, sim.column_range):
            with pytest.raises(sph.SphError, match=r"\(-4\)"):
                call()
    sim.close()


def test_a_column_frame_leaves_the_run_alone_and_is_timed():
    sims = [make(4096), make(4096)]
    for s in sims:
        s.setup()
        s.simulate()
    sims[0].render_time(reset=True)
    sims[0].render_column()
    sims[0].render_column(width=64, height=48)
    sims[0].render_frame()
    sec, frames = sims[0].render_time(reset=True)
    assert frames == 3 and 0.0 < sec < 1.0
    sims[0].render_column()
    for s in sims:
        s.simulate()
    a, b = (s.download_state() for s in sims)
    for k in ("pos", "vel", "rho"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # NULL options: 800 x 600, automatic range
    assert sims[0]._L.sph_render_column(sims[0]._h, None) == 0
    got = dict(rgb=np.array(sims[0].frame_host(), copy=True), column=sims[0].column_buffer(), range=sims[0].column_range())
    assert_column_equal(got, restate(sims[0], a), "NULL options")
    for s in sims:
        s.close()


def test_error_paths():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):   # SPH_ESTATE: no state yet
        sim.render_column()
    sim.setup()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(lo=2.0, hi=1.0), dict(lo=nan, hi=1.0), dict(lo=0.0, hi=nan), dict(lo=0.0, hi=inf),
                dict(lo=-inf, hi=0.0), dict(width=4097), dict(height=-5), dict(width=-1)):
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.render_column(**bad)
    o = _lib.SphColumnFrameOptions()  # struct_size left at 0
    assert sim._L.sph_render_column(sim._h, o) == -1
    assert sim._L.sph_render_column(None, None) == -1 and sim._L.sph_download_column_buffer(sim._h, None) == -1
    with pytest.raises(sph.SphError):    # nothing rendered yet
        sim.column_buffer()
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.column_range()
    sim.render_column(width=4096, height=4096)   # the largest image
    assert sim.column_buffer().shape == (4096, 4096) and sim.frame_host().shape == (4096, 4096, 3)
    sim.render_column()
    assert sim.column_buffer().shape == (600, 800)
    sim.render_field()                   # a field frame: the column buffer and range are gone
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.column_buffer()
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.column_range()
    sim.close()
    slab = make(4096, flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096)
    with pytest.raises(sph.SphError, match=r"\(-4\).*slab"):
        slab.render_column()
    slab.close()


def _run_cli(tmp_path, extra):
    env = dict(os.environ)
    env.pop("SPH_FREE_SHADE", None)
    env.update({"SPH_FREE_FRAMES": "4", "SPH_FREE_FRAMES_DIR": str(tmp_path), "SPH_PRINT_SHA256": "1"})
    env.update(extra)
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(tmp_path))
    assert names == ["frame_%04d.ppm" % f for f in range(4)]
    blob = open(os.path.join(tmp_path, names[-1]), "rb").read()
    header = b"P6\n800 600\n255\n"
    assert blob.startswith(header) and len(blob) == len(header) + 1440000
    return r, np.frombuffer(blob[len(header):], np.uint8).reshape(600, 800, 3)


@pytest.mark.parametrize("shade", ["column", None, "thickness"])
def test_cli_free_shade(tmp_path, shade):
    r, last = _run_cli(tmp_path, {"SPH_FREE_SHADE": shade} if shade else {})
    # the Python binding reproduces the state the CLI printed ...
    sim = make(4096)
    sim.setup()
    for _ in range(4):
        sim.simulate()
    host = np.array(sim.getPosition(), copy=True)
    printed = re.search(r"positions_sha256 ([0-9a-f]{64})", r.stdout).group(1)
    assert hashlib.sha256(host.tobytes()).hexdigest() == printed
    st = sim.download_state()
    assert np.array_equal(st["pos"].view(np.uint32), host.view(np.uint32))
    # ... and the last frame is the restatement of that state
    if shade == "column":
        want = restate(sim, st)["rgb"]
        assert "SPH_FREE_SHADE" not in r.stderr
    else:  # unset, or an unknown name (reported): the flat frame, as before
        want = R.render(st["pos"])["rgb"]
        assert ("SPH_FREE_SHADE=thickness" in r.stderr) == (shade is not None)
    sim.close()
    assert np.array_equal(last, want)
