"""The frame renderer on the GPU against its numpy restatement (tests/render_restatement.py).
Every comparison is exact: integers and bytes, no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import render_restatement as R
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")


def make(n, random=True, **kw):
    sim = sph.Simulator(sph.default_settings(n, random), **kw)
    return sim


def gpu_frame(sim, **opt):
    rgb = sim.render(**opt)
    out = sim.frame_buffers()
    out["rgb"] = rgb
    return out


def assert_frame_equal(got, want, what):
    for k in ("edge", "count", "depth", "rgb"):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {a.size} entries differ, first at {np.argwhere(bad)[0]}"


def check_against_restatement(sim, what, pos=None, **opt):
    """render with `opt` and compare all four buffers with the restatement of the downloaded positions"""
    if pos is None:
        pos = sim.download_state()["pos"]
    got = gpu_frame(sim, **opt)
    ropt = dict(width=opt.get("width") or 800, height=opt.get("height") or 600,
                point_size=opt.get("point_size") or 3, shade=opt.get("shade", "flat"))
    assert_frame_equal(got, R.render(pos, **ropt), f"{what} {opt}")
    return got


@pytest.mark.parametrize("name", ["random4096", "dense4096", "grid2048"])
def test_golden_states(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    for key in [k for k in data.files if k.startswith("pos_")]:
        pos = data[key]
        sim = make(len(pos))
        sim.upload_state(pos)
        check_against_restatement(sim, f"{name}/{key} uploaded")
        check_against_restatement(sim, f"{name}/{key} uploaded", shade="count")
        sim.simulate()  # the same through the cell-sorted stream
        check_against_restatement(sim, f"{name}/{key} + 1 step", shade="count")
        sim.close()


def test_random_262144_after_0_1_and_30_steps_all_sizes_shades_and_points():
    sim = make(262144)
    sim.setup()
    done = 0
    for steps in (0, 1, 30):
        while done < steps:
            sim.simulate()
            done += 1
        pos = sim.download_state()["pos"]
        for shade in ("flat", "count"):
            check_against_restatement(sim, f"step {steps}", pos, shade=shade)
        for w, h in ((1, 1), (333, 77), (4096, 4096)):
            check_against_restatement(sim, f"step {steps}", pos, width=w, height=h, shade="count")
        for ps in (1, 3, 9):
            check_against_restatement(sim, f"step {steps}", pos, point_size=ps, shade="count")
            check_against_restatement(sim, f"step {steps}", pos, width=333, height=77, point_size=ps)
    # defaults spelled out == defaults
    a = sim.render()
    b = sim.render(width=800, height=600, point_size=3, shade="flat")
    assert a.shape == (600, 800, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    sim.close()


def test_floor_pile_4m_after_100_steps(monkeypatch):
    """n = 4,194,304 after 100 steps: 44 % of the particles in the floor layer, the contended case;
    the aggregated splat, the plain splat and the restatement agree."""
    sim = make(4194304)
    sim.setup()
    for _ in range(100):
        sim.simulate()
    pos = sim.download_state()["pos"]
    want = {s: R.render(pos, shade=s) for s in ("flat", "count")}
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_RENDER_PLAIN", plain)
        for shade in ("flat", "count"):
            assert_frame_equal(gpu_frame(sim, shade=shade), want[shade], f"4M step 100 plain={plain} {shade}")
    assert want["count"]["count"].max() > 1000  # the pile is there
    sim.close()


def test_aggregated_splat_equals_plain_splat(monkeypatch):
    states = []
    for name in ("random4096", "dense4096", "grid2048"):
        data = np.load(os.path.join(GOLD, name + ".npz"))
        states += [data[k] for k in data.files if k.startswith("pos_")]
    for pos in states:
        sim = make(len(pos))
        sim.upload_state(pos)
        for steps in (0, 2):
            for _ in range(steps):
                sim.simulate()
            for opt in (dict(), dict(point_size=9, shade="count"), dict(width=333, height=77, point_size=1)):
                monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
                a = gpu_frame(sim, **opt)
                monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
                b = gpu_frame(sim, **opt)
                assert_frame_equal(a, b, f"aggregated vs plain {opt}")
        sim.close()
    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = make(262144)
    sim.setup()
    for _ in range(30):
        sim.simulate()
    a = gpu_frame(sim, shade="count")
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    assert_frame_equal(a, gpu_frame(sim, shade="count"), "aggregated vs plain, n = 262144 step 30")
    sim.close()


# the shapes test_gpu_field_frame.py holds the field splat to.  64 x 48: the whole image fits the LDS tile, every
# workgroup aggregates; 800 x 600: a 1024-row workgroup of these 4096 particles spans far more than a tile, every
# workgroup issues the per-hit atomics; one odd size
PATH_CASES = [dict(width=64, height=48, point_size=1), dict(width=64, height=48, point_size=9),
              dict(width=800, height=600, point_size=3), dict(width=333, height=77, point_size=3)]


@pytest.mark.parametrize("steps", [0, 3])
def test_paths_tile_fallback_and_plain(steps, monkeypatch):
    data = np.load(os.path.join(GOLD, "random4096.npz"))

    def handle():
        sim = make(len(data["pos_1"]))
        sim.upload_state(data["pos_1"], data["vel_1"])
        for _ in range(steps):
            sim.simulate()
        return sim

    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = handle()
    pos = sim.download_state()["pos"]
    tiled = [check_against_restatement(sim, f"random4096 + {steps} steps", pos, shade="count", **case) for case in PATH_CASES]
    sim.close()
    monkeypatch.setenv("SPH_RENDER_PLAIN", "1")
    twin = handle()  # a fresh handle: nothing of the tiled frames is left in its buffers
    for case, a in zip(PATH_CASES, tiled):
        assert_frame_equal(gpu_frame(twin, shade="count", **case), a, f"plain vs tiled, {steps} steps {case}")
    twin.close()


def test_same_image_from_every_sweep_and_key_order():
    n, steps = 32768, 5
    frames, poses = {}, {}
    for tag, kw in (("list", dict(sweep="list")), ("lds", dict(sweep="lds")), ("direct", dict(sweep="direct")),
                    ("morton", dict(sweep="direct", key_order="morton"))):
        sim = make(n, **kw)
        sim.setup()
        for _ in range(steps):
            sim.simulate()
        poses[tag] = sim.download_state()["pos"]
        frames[tag] = gpu_frame(sim, shade="count")
        sim.close()
    for tag in ("lds", "direct"):
        assert_bit_equal(poses[tag], poses["list"], f"positions {tag} vs list")  # first: same positions
        assert_frame_equal(frames[tag], frames["list"], f"{tag} vs list")
    assert_frame_equal(frames["list"], R.render(poses["list"], shade="count"), "list vs restatement")
    # Morton keys sum the neighbours in another order: positions agree with the flattened order to
    # rounding only (test_gpu_parity.py), so the image is held to its own positions, and to the list
    # sweep's image where the positions happen to be the same bits
    assert_frame_equal(frames["morton"], R.render(poses["morton"], shade="count"), "morton vs restatement")
    if np.array_equal(poses["morton"].view(np.uint32), poses["list"].view(np.uint32)):
        assert_frame_equal(frames["morton"], frames["list"], "morton vs list")


def test_linked_sweep_renders_from_its_state_array():
    sim = make(8192, sweep="linked")
    sim.setup()
    for _ in range(3):
        sim.simulate()
    check_against_restatement(sim, "linked", shade="count")
    sim.close()


def _run_ten_steps(render, timed, click):
    sim = make(65536)
    sim.setup()
    times = sph.Times()
    for k in range(10):
        if timed:
            sim.simulateAndTime(times)
        else:
            sim.simulate()
        if render:
            sim.render_frame(shade="count")
            if k % 3 == 0:
                sim.frame_host()
        if click and k == 4:
            sim.moveParticles((400, 300))
            if render:
                sim.render_frame()
    out = sim.download_state()
    host = np.array(sim.getPosition(), copy=True)
    frame = gpu_frame(sim, shade="count") if render else None
    sim.close()
    return out, host, frame


@pytest.mark.parametrize("env", [{}, {"SPH_PIPELINE": "1"}, {"SPH_PIPELINE": "0"}])
@pytest.mark.parametrize("timed", [False, True])
@pytest.mark.parametrize("click", [False, True])
def test_rendering_changes_nothing(env, timed, click, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, host_a, _ = _run_ten_steps(False, timed, click)
    b, host_b, frame = _run_ten_steps(True, timed, click)
    assert_bit_equal(a["pos"], b["pos"], "positions with vs without renders")
    assert_bit_equal(a["rho"], b["rho"], "densities with vs without renders")
    assert_bit_equal(a["vel"], b["vel"], "velocities with vs without renders")
    assert_bit_equal(host_a, host_b, "getPosition() with vs without renders")
    # and the frames drawn in between showed the right state
    assert_frame_equal(frame, R.render(b["pos"], shade="count"), "frame after the run")


def test_frame_after_a_click_shows_the_same_positions():
    sim = make(16384)
    sim.setup()
    for _ in range(3):
        sim.simulate()
    before = gpu_frame(sim)
    sim.moveParticles((400, 300))  # velocities only
    after = gpu_frame(sim)
    assert_frame_equal(after, before, "frame after a click")
    sim.close()


def test_no_readback_handle_renders_what_its_twin_holds():
    twin = make(65536)
    dark = make(65536, flags=_lib.SPH_FLAG_NO_READBACK)
    for s in (twin, dark):
        s.setup()
        for _ in range(7):
            s.simulate()
    pos = twin.download_state()["pos"]
    assert_frame_equal(gpu_frame(dark, shade="count"), R.render(pos, shade="count"), "no-read-back handle")
    assert_frame_equal(gpu_frame(twin, shade="count"), R.render(pos, shade="count"), "twin")
    twin.close()
    dark.close()


def test_render_time_counts_frames():
    sim = make(4096)
    sim.setup()
    sim.simulate()
    sim.render_time(reset=True)
    for _ in range(5):
        sim.render_frame()
    sec, frames = sim.render_time(reset=True)
    assert frames == 5 and 0.0 < sec < 1.0
    assert sim.render_time() == (0.0, 0)
    assert sim.frame_host().shape == (600, 800, 3)  # still valid after the reset
    sim.close()


def test_error_paths():
    sim = make(4096)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):   # SPH_ESTATE: no state yet
        sim.render_frame()
    with pytest.raises(sph.SphError):
        sim.frame_host()
    sim.setup()
    for bad in (dict(width=4097), dict(height=4097), dict(width=-1), dict(height=-5), dict(point_size=2),
                dict(point_size=11), dict(point_size=-1), dict(shade=2), dict(shade=-1)):
        with pytest.raises(sph.SphError, match=r"\(-1\)"):   # SPH_EINVAL
            sim.render_frame(**bad)
    o = _lib.SphRenderOptions()  # struct_size left at 0
    assert sim._L.sph_render_frame(sim._h, o) == -1
    assert sim._L.sph_render_frame(sim._h, None) == 0   # NULL = display.cpp's
    assert sim.frame_host().shape == (600, 800, 3)
    sim.close()
    slab = make(4096, flags=_lib.SPH_FLAG_EXTERNAL_STATE, capacity=4096)
    with pytest.raises(sph.SphError, match=r"\(-4\).*slab"):
        slab.render_frame()
    slab.close()


def _run_cli(tmp_path, extra):
    env = dict(os.environ)
    env.update({"SPH_FREE_FRAMES": "3", "SPH_FREE_FRAMES_DIR": str(tmp_path)})
    env.update(extra)
    r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("click", [False, True])
def test_cli_writes_the_frames_the_python_binding_renders(tmp_path, click):
    r = _run_cli(tmp_path, {"SPH_FREE_CLICK": "1"} if click else {})
    names = sorted(os.listdir(tmp_path))
    assert names == ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]
    header = b"P6\n800 600\n255\n"
    blobs = []
    for nme in names:
        blob = open(os.path.join(tmp_path, nme), "rb").read()
        assert blob.startswith(header) and len(blob) == len(header) + 1440000, nme
        blobs.append(blob[len(header):])
    sim = make(4096)
    sim.setup()
    for f in range(3):
        if click and f == 1:  # headless.cpp: the click is raised before frame frames / 2
            sim.mouseClicked, sim.clickCoords = True, (400, 300)
        sim.simulate()
    assert sim.render().tobytes() == blobs[2]
    sim.close()
    # the frames change nothing on stdout
    env = dict(os.environ)
    env.update({"SPH_FREE_FRAMES": "3"})
    if click:
        env["SPH_FREE_CLICK"] = "1"
    env.pop("SPH_FREE_FRAMES_DIR", None)
    plain = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True,
                           timeout=120, env=env)
    assert plain.returncode == 0 and plain.stdout == r.stdout


def test_cli_frame_every(tmp_path):
    _run_cli(tmp_path, {"SPH_FREE_FRAMES": "5", "SPH_FREE_FRAME_EVERY": "2"})
    assert sorted(os.listdir(tmp_path)) == ["frame_0000.ppm", "frame_0002.ppm", "frame_0004.ppm"]
