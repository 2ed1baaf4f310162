"""The field frame on the GPU against its numpy restatement (tests/field_frame_restatement.py), fed by
sph_download_state.  Every comparison is exact: RGB, value buffer, depth, count, edge layer and the bits of
the range, no tolerance anywhere."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import field_frame_restatement as FF
import render_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def from_golden(name, steps, **kw):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    sim = make(len(data["pos_1"]), **kw)
    sim.upload_state(data["pos_1"], data["vel_1"])
    for _ in range(steps):
        sim.simulate()
    return sim


def gpu_field(sim, **opt):
    sim.render_field(**opt)
    out = dict(rgb=np.array(sim.frame_host(), copy=True), value=sim.field_buffer(), range=sim.field_range())
    out.update(sim.frame_buffers())
    return out


def assert_field_equal(got, want, what):
    for k in ("edge", "count", "depth", "value", "rgb"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {a.size} entries differ, first at {np.argwhere(bad)[0]}"
    ga, wa = (np.array(x["range"], F).view(np.uint32).tolist() for x in (got, want))
    assert ga == wa, f"{what}: range {got['range']} vs {want['range']}"


def check(sim, what, st=None, **opt):
    """render with `opt`, compare everything with the restatement of the downloaded state"""
    st = st or sim.download_state()
    got = gpu_field(sim, **opt)
    ropt = dict(opt)
    for k, d in (("width", 800), ("height", 600), ("point_size", 3)):
        ropt[k] = ropt.get(k) or d
    assert_field_equal(got, FF.render_field(st["pos"], st["vel"], st["rho"], **ropt), f"{what} {opt}")
    return got


def check_clipped(sim, what, st, field, **opt):
    """a fixed range between the quartiles of the field: values below lo AND above hi, both ends clip"""
    v = np.sort(FF.scalar(st["vel"], st["rho"], field))
    lo, hi = v[len(v) // 4], v[(3 * len(v)) // 4]
    assert v[0] < lo < hi < v[-1], f"{what}: {field} does not spread over its quartiles: the clipping case is not covered"
    got = check(sim, what, st, field=field, lo=float(lo), hi=float(hi), **opt)
    assert got["range"] == (lo, hi)


# 64 x 48: the whole image fits the LDS tile, every workgroup aggregates; 800 x 600: a 1024-row workgroup of
# these 4096 particles spans far more than a tile, every workgroup issues the per-hit atomics; one odd size
PATH_CASES = [dict(width=64, height=48, point_size=1), dict(width=64, height=48, point_size=9),
              dict(width=800, height=600, point_size=3), dict(width=333, height=77, point_size=3)]


@pytest.mark.parametrize("steps", [0, 3])
def test_paths_tile_fallback_and_plain(steps, monkeypatch):
    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = from_golden("random4096", steps)
    st = sim.download_state()
    assert (FF.scalar(st["vel"], st["rho"], "speed") > 0).any()
    tiled = [check(sim, f"random4096 + {steps} steps", st, field="speed", **case) for case in PATH_CASES]
    sim.close()
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    twin = from_golden("random4096", steps)  # a fresh handle: nothing of the tiled frames is left in its buffers
    for case, a in zip(PATH_CASES, tiled):
        assert_field_equal(gpu_field(twin, field="speed", **case), a, f"plain vs tiled, {steps} steps {case}")
    twin.close()


def test_ties_and_all_three_fields_on_the_lattice():
    sim = make(2048, random=False)
    sim.setup()
    for _ in range(2):
        sim.simulate()
    st = sim.download_state()
    # the lattice: squares that cover the same pixel with the same bits of w and different values -- the low
    # word decides
    px, py, wb = R.project(st["pos"], 800, 600)
    s = FF.scalar(st["vel"], st["rho"], "density")
    cover = np.concatenate([((py + dy) * 800 + (px + dx)) * (1 << 32) + wb.astype(np.int64)
                            for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    order = np.argsort(cover, kind="stable")
    cover, s9 = cover[order], np.tile(s, 9)[order]
    assert ((cover[1:] == cover[:-1]) & (s9[1:] != s9[:-1])).any(), "no tie in w with different values: not covered"
    for field in FF.FIELDS:
        check(sim, "grid2048 + 2 steps", st, field=field)
        check(sim, "grid2048 + 2 steps", st, field=field, point_size=9, width=64, height=48)
        # a fixed range: everything below it, everything above it (whatever the field holds, both clip)
        top = float(FF.scalar(st["vel"], st["rho"], field).max())
        check(sim, "grid2048 + 2 steps", st, field=field, lo=top + 1.0, hi=top + 2.0)
        check(sim, "grid2048 + 2 steps", st, field=field, lo=-2.0, hi=-1.0)
    # ... and one that clips at both ends: the density of the lattice differs between its faces and its inside
    check_clipped(sim, "grid2048 + 2 steps", st, "density")
    sim.close()


def test_pressure_above_zero_in_the_dense_block():
    sim = from_golden("dense4096", 5)
    st = sim.download_state()
    assert (st["prs"] > 0).any(), "no particle under pressure: the case is not covered"
    # the restatement's pressure is the one sph_download_state reports
    assert np.array_equal(FF.scalar(st["vel"], st["rho"], "pressure").view(np.uint32), st["prs"].view(np.uint32))
    got = check(sim, "dense4096 + 5 steps", st, field="pressure")
    assert got["range"][1] == st["prs"].max() > 0   # (the particles under pressure are inside the block, mostly hidden)
    hi = float(st["prs"].max())
    assert (st["prs"] < 0.25 * hi).any() and (st["prs"] > 0.5 * hi).any()   # clips at both ends
    check(sim, "dense4096 + 5 steps", st, field="pressure", lo=0.25 * hi, hi=0.5 * hi)
    check_clipped(sim, "dense4096 + 5 steps", st, "speed")
    check_clipped(sim, "dense4096 + 5 steps", st, "density")
    check(sim, "dense4096 + 5 steps", st, field="density", width=64, height=48, point_size=9)
    check(sim, "dense4096 + 5 steps", st, field="speed", width=333, height=77)
    sim.close()


def test_depth_and_count_are_those_of_the_flat_frame_and_flat_frames_are_unchanged():
    sim = from_golden("random4096", 3)
    st = sim.download_state()
    for opt in (dict(), dict(width=64, height=48, point_size=9), dict(width=333, height=77, point_size=1)):
        sim.render_frame(**opt)
        flat = sim.frame_buffers()
        field = gpu_field(sim, field="speed", **opt)
        for k in ("depth", "count", "edge"):
            assert np.array_equal(flat[k], field[k]), f"{k} {opt}"
        # a flat and a count frame after the field frame: the existing restatement, and no field buffer any more
        for shade in ("flat", "count"):
            rgb = sim.render(shade=shade, **opt)
            got = sim.frame_buffers()
            want = R.render(st["pos"], width=opt.get("width", 800), height=opt.get("height", 600),
                            point_size=opt.get("point_size", 3), shade=shade)
            assert np.array_equal(rgb, want["rgb"]), f"{shade} {opt}"
            for k in ("depth", "count", "edge"):
                assert np.array_equal(got[k], want[k]), f"{shade} {k} {opt}"
    sim.close()


def test_a_click_shows_in_the_speed_frame():
    frames = {}
    for click in (False, True):
        sim = make(4096)
        sim.setup()
        sim.simulate()
        if click:
            sim.moveParticles((400, 300))
        sim.simulate()
        frames[click] = check(sim, f"click={click}", field="speed", lo=0.0, hi=2.0)
        check(sim, f"click={click}", field="speed")
        sim.close()
    assert not np.array_equal(frames[True]["rgb"], frames[False]["rgb"])
    assert not np.array_equal(frames[True]["value"], frames[False]["value"])


def test_no_readback_and_linked_handles():
    twin = make(4096)
    dark = make(4096, flags=_lib.SPH_FLAG_NO_READBACK)
    for s in (twin, dark):
        s.setup()
        for _ in range(4):
            s.simulate()
    st = twin.download_state()
    for field in ("speed", "density"):
        check(dark, "no-read-back handle", st, field=field)
        check(twin, "its twin", st, field=field)
    twin.close()
    dark.close()
    linked = make(4096, sweep="linked")
    linked.setup()
    for _ in range(3):
        linked.simulate()
    for field in FF.FIELDS:
        check(linked, "linked", field=field)
    linked.close()


def test_render_time_counts_both_kinds_and_defaults():
    sim = make(4096)
    sim.setup()
    sim.simulate()
    sim.render_time(reset=True)
    sim.render_frame()
    sim.render_field()
    sim.render_field(field="density")
    sec, frames = sim.render_time(reset=True)
    assert frames == 3 and 0.0 < sec < 1.0
    st = sim.download_state()
    assert sim._L.sph_render_field(sim._h, None) == 0   # NULL = 800 x 600, size 3, speed, automatic range
    got = dict(rgb=np.array(sim.frame_host(), copy=True), value=sim.field_buffer(), range=sim.field_range())
    got.update(sim.frame_buffers())
    assert_field_equal(got, FF.render_field(st["pos"], st["vel"], st["rho"], "speed"), "NULL options")
    sim.close()


def test_error_paths():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):   # SPH_ESTATE: no state yet
        sim.render_field()
    sim.setup()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(field=3), dict(field=-1), dict(lo=2.0, hi=1.0), dict(lo=nan, hi=1.0), dict(lo=0.0, hi=nan),
                dict(lo=0.0, hi=inf), dict(lo=-inf, hi=0.0), dict(point_size=2), dict(point_size=11),
                dict(width=4097), dict(height=-5)):
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.render_field(**bad)
    o = _lib.SphFieldFrameOptions()  # struct_size left at 0
    assert sim._L.sph_render_field(sim._h, o) == -1
    with pytest.raises(sph.SphError):    # nothing rendered yet
        sim.field_buffer()
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.field_range()
    sim.render_field()
    assert sim.field_buffer().shape == (600, 800)
    sim.render_frame()                   # a flat frame: the field buffer and range are gone
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.field_buffer()
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.field_range()
    assert sim.frame_host().shape == (600, 800, 3)
    sim.close()
    slab = make(4096, flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096)
    with pytest.raises(sph.SphError, match=r"\(-4\).*slab"):
        slab.render_field()
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


@pytest.mark.parametrize("shade", ["speed", None, "viscosity"])
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
    sim.close()
    assert np.array_equal(st["pos"].view(np.uint32), host.view(np.uint32))
    # ... and the last frame is the restatement of that state
    if shade == "speed":
        want = FF.render_field(st["pos"], st["vel"], st["rho"], "speed")["rgb"]
        assert "SPH_FREE_SHADE" not in r.stderr
    else:  # unset, or an unknown name (reported): the flat frame, as before
        want = R.render(st["pos"])["rgb"]
        assert ("SPH_FREE_SHADE=viscosity" in r.stderr) == (shade is not None)
    assert np.array_equal(last, want)
