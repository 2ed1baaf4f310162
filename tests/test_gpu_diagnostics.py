"""Run diagnostics on the GPU (sph_diagnose) against the numpy / Python-int restatement
(tests/diagnostics_restatement.py) of what download_state returns.  Every comparison is exact and covers every raw
word -- the struct is compared byte for byte: the sums are integer sums, so launch shape, row order, the kernel path
and the number of slabs cannot change a bit, and no tolerance appears anywhere."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib
from cudafluidsimulator_amd import mgpu as M

import diagnostics_restatement as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
GOLDENS = ("random4096", "dense4096", "grid2048")
SPH_EINVAL, SPH_ESTATE = -1, -4


def make(n, random=True, **kw):
    return sph.Simulator(sph.default_settings(n, random), **kw)


def from_golden(name, **kw):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    sim = make(len(data["pos_1"]), **kw)
    sim.upload_state(data["pos_1"], data["vel_1"])
    return sim


def words(sim, **kw):
    sim.diagnose(**kw)
    return sim.diagnostics_raw()


def restated(st, **kw):
    return D.to_struct(D.restate(st["pos"], st["vel"], st["rho"], **kw))


def check(sim, what, st=None, **kw):
    """the GPU's words against the restatement of the downloaded state; returns them"""
    st = st or sim.download_state()
    got = words(sim, **kw)
    D.assert_same_words(got, restated(st, **kw), f"{what} {kw}")
    return got


def small_state(n, seed, nan=False):
    """velocities of both signs, some tiny (2^-30), one row at 1e6 (its v2 saturates); nan: NaN and infinite ones too"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.1, 9.9, (n, 3)).astype(F)
    vel = (rng.uniform(-3, 3, (n, 3)) * rng.choice([1.0, 2.0**-30], (n, 1))).astype(F)
    vel[n // 2] = (1e6, -0.75, 2.0**-30)
    if n >= 3:  # terms below one unit of Q32.32, of both signs, and a denormal
        vel[n // 2 + 1] = (-(2.0**-40), 2.0**-40, -0.0)
        vel[n // 2 - 1] = (-(2.0**-33), -1e-40, 1e-40)
    if nan:
        vel[n // 3, 1] = np.nan
        vel[(2 * n) // 3] = np.nan
        vel[n // 4] = (-(2.0**31), np.inf, -np.inf)  # -2^31 is the last value in range; the infinities saturate
    return pos, vel


# ---- small shapes: partial waves, one wave, more than one workgroup; the plain path gives the same words ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_small_shapes_and_the_plain_path(n, monkeypatch):
    sim = make(n)
    sim.upload_state(*small_state(n, n))
    st = sim.download_state()
    for kw in (dict(), dict(hist="speed", value_range=(0.0, 3.0))):
        monkeypatch.setenv("SPH_DIAG_PLAIN", "0")
        got = check(sim, f"n = {n}", st, **kw)
        assert got.saturated >= 1 and got.n == n
        monkeypatch.setenv("SPH_DIAG_PLAIN", "1")
        D.assert_same_words(words(sim, **kw), got, f"plain vs production, n = {n} {kw}")
    sim.close()


def test_nan_velocities_count_as_saturated_and_sort_by_their_bits(monkeypatch):
    n = 300
    sim = make(n)
    sim.upload_state(*small_state(n, 5, nan=True))
    st = sim.download_state()
    assert np.isnan(st["vel"]).sum() == 4
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_DIAG_PLAIN", plain)
        got = check(sim, f"NaN velocities, plain = {plain}", st, hist="speed")
        # vy of one row, vx vy vz of another, the v2 of both, the 1e6 row's v2, and the infinite vy, vz and v2 of one row
        assert got.saturated == 4 + 2 + 1 + 3
        assert np.isnan(np.array([got.max_bits[3]], np.uint32).view(F)[0]), "a +NaN speed is the key-ordered maximum"
    sim.close()


def test_every_lane_takes_at_least_two_rows(monkeypatch):
    """The production launch is capped at 1024 workgroups of 256 lanes: beyond 2^19 rows every lane loops."""
    n = (1 << 19) + 1000
    rng = np.random.default_rng(1)
    pos = rng.uniform(0.1, 9.9, (n, 3)).astype(F)
    vel = rng.uniform(-2, 2, (n, 3)).astype(F)
    vel[123456] = (1e6, 0, 0)
    sim = make(n, flags=_lib.SPH_FLAG_NO_READBACK)
    sim.upload_state(pos, vel)
    want = D.to_struct(D.restate(pos, vel, np.zeros(n, F), hist="speed", value_range=(0.0, 3.0)))
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_DIAG_PLAIN", plain)
        D.assert_same_words(words(sim, hist="speed", value_range=(0.0, 3.0)), want, f"n = {n}, plain = {plain}")
    sim.close()


def test_no_particles():
    sim = make(0)
    sim.setup()
    got = words(sim, hist="density")
    empty = np.zeros((0, 3), F)
    D.assert_same_words(got, D.to_struct(D.restate(empty, empty, np.zeros(0, F), hist="density")), "n = 0")
    assert got.min_bits[0] == 0x7F800000 and got.max_bits[0] == 0xFF800000
    sim.close()


# ---- the goldens: after upload, 1 and 20 steps, a click; every sweep and key order ----

def walk(sims, click=True):
    """run the sims in lockstep through the points, checking each against its own download_state; yields
    (label, [words per sim])"""
    def point(label):
        return label, [check(s, label, hist="density", value_range=(900.0, 1100.0)) for s in sims]
    yield point("after upload")
    for s in sims:
        s.simulate()
    yield point("after 1 step")
    for _ in range(19):
        for s in sims:
            s.simulate()
    yield point("after 20 steps")
    if click:
        for s in sims:
            s.moveParticles((400, 300))
        yield point("after a click")
        for s in sims:
            s.simulate()
        yield point("one step after the click")


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_sorted_sweeps_agree_word_for_word(name):
    sims = [from_golden(name, sweep=s) for s in ("list", "lds", "direct")]
    sims.append(from_golden(name, sweep="direct", key_order="morton"))  # (held against its own state only)
    moved = False
    for label, got in walk(sims):
        D.assert_same_words(got[1], got[0], f"{name} {label}: lds vs list")
        D.assert_same_words(got[2], got[0], f"{name} {label}: direct vs list")
        moved = moved or any(got[0].sum[k].lo or got[0].sum[k].hi for k in (3, 4, 5))
    assert moved, "no momentum anywhere: the velocity sums are not covered"
    for s in sims:
        s.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_linked_backend(name):
    sim = from_golden(name, sweep="linked")  # particle-id order on the device; no click with this backend
    for _ in walk([sim], click=False):
        pass
    sim.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_resumed_snapshot(name, tmp_path):
    path, k = tmp_path / "state.sph", 4
    sim = from_golden(name)
    for _ in range(5):
        sim.simulate()
    sim.save_state(path)
    at_save = check(sim, f"{name} at the snapshot", hist="speed")
    for _ in range(k):
        sim.simulate()
    later = check(sim, f"{name} {k} steps on", hist="speed")
    sim.close()
    twin = from_golden(name)  # a fresh handle
    twin.load_state(path)
    D.assert_same_words(words(twin, hist="speed"), at_save, f"{name}: right after load_state")
    for _ in range(k):
        twin.simulate()
    D.assert_same_words(words(twin, hist="speed"), later, f"{name}: {k} steps after load_state")
    check(twin, f"{name} resumed", hist="speed")
    twin.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_without_readback(name):
    sim, twin = from_golden(name, flags=_lib.SPH_FLAG_NO_READBACK), from_golden(name)
    for steps in (0, 1, 19):
        for _ in range(steps):
            sim.simulate()
            twin.simulate()
        check(sim, f"{name} NO_READBACK", st=twin.download_state(), hist="pressure")
    sim.close()
    twin.close()


# ---- the histogram ----

@pytest.fixture(scope="module")
def dense_after_steps():
    sim = from_golden("dense4096")
    for _ in range(3):
        sim.simulate()
    st = sim.download_state()
    assert (st["prs"] > 0).any() and (st["prs"] == 0).any(), "dense4096 no longer switches the pressure term on"
    yield sim, st
    sim.close()


@pytest.mark.parametrize("field", D.FIELDS)
def test_histogram_fixed_automatic_and_degenerate_ranges(field, dense_after_steps, monkeypatch):
    sim, st = dense_after_steps
    s = np.sort(D.columns(st["pos"], st["vel"], st["rho"])[D.EXT_OF_FIELD[field]])
    u = np.unique(s)
    assert len(u) >= 4, f"{field} does not spread: the clipping case is not covered"
    lo, hi = float(u[len(u) // 4]), float(u[(3 * len(u)) // 4])  # values below lo and above hi: both ends clip
    assert s[0] < lo < hi < s[-1]
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_DIAG_PLAIN", plain)
        fixed = check(sim, "fixed range", st, hist=field, value_range=(lo, hi))
        assert sum(fixed.hist) == sim.n and fixed.hist[0] >= 2 and fixed.hist[255] >= 2
        auto = check(sim, "automatic range", st, hist=field)
        assert sum(auto.hist) == sim.n and auto.hist[255] >= 1
        got_range = np.array([auto.hist_lo_bits, auto.hist_hi_bits], np.uint32).view(F)
        assert (got_range[0], got_range[1]) == (s[0], s[-1])
        D.assert_same_words(words(sim, hist=field, value_range=tuple(float(v) for v in got_range)), auto,
                            "the reported range passed explicitly")
        flat = check(sim, "hi == lo", st, hist=field, value_range=(hi, hi))
        assert flat.hist[0] == sim.n


# ---- no interference with the step ----

def test_diagnostics_change_no_result_of_any_step():
    def run(diagnose, phased):
        sim = from_golden("random4096")
        mid = []
        for _ in range(20):
            if diagnose:
                before = words(sim)
            if phased:
                sim.phase("grid")
                if diagnose:  # the state is still the one `before` saw
                    D.assert_same_words(words(sim, hist="speed"), words(sim, hist="speed"), "twice in a row")
                    now = words(sim)
                    D.assert_same_words(now, before, "between phase_grid and phase_density")
                    mid.append(now)
                for p in ("density", "force", "readback"):
                    sim.phase(p)
            else:
                sim.simulate()
        out = dict(st=sim.download_state(), pos=np.array(sim.getPosition(), copy=True), steps=sim.kernel_times().steps)
        if diagnose:
            assert sim.diagnostics_time()[1] == (80 if phased else 20)
        sim.close()
        return out
    for phased in (False, True):
        a, b = run(True, phased), run(False, phased)
        assert a["steps"] == b["steps"]
        assert a["pos"].tobytes() == b["pos"].tobytes()
        for k in ("pos", "vel", "rho", "prs"):
            assert a["st"][k].tobytes() == b["st"][k].tobytes(), k


# ---- slabs: N slabs give the single domain's words ----

def moving_state(n, seed, vz=9.0):
    """random fluid as moving_state of tests/test_mgpu.py, but every z-velocity points up (0 .. 0.9 cells per step):
    particles change slabs every step, and the fluid as a whole drifts, so a re-cut moves the cuts"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.5, 9.5, (n, 3)).astype(F)
    vel = rng.uniform(-1, 1, (n, 3)).astype(F)
    vel[:, 2] = rng.uniform(0, vz, n).astype(F)
    return pos, vel


SLAB_N, SLAB_STEPS, SLAB_HIST = 4096, 10, dict(hist="speed", value_range=(0.0, 10.0))


@pytest.fixture(scope="module")
def single_domain_words():
    """the single domain's words before the first step and after each of the ten"""
    pos, vel = moving_state(SLAB_N, 5)
    sim = sph.Simulator(sph.default_settings(SLAB_N, False))
    sim.upload_state(pos, vel)
    out = [check(sim, "single domain, step 0", **SLAB_HIST)]
    for k in range(SLAB_STEPS):
        sim.simulate()
        out.append(check(sim, f"single domain, step {k + 1}", **SLAB_HIST))
    sim.close()
    return pos, vel, out


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("transport", ["loopback", "streams"])
def test_slabs_equal_the_single_domain_byte_for_byte(world, transport, single_domain_words):
    pos, vel, want = single_domain_words
    mg = M.MultiGpuSimulator(sph.default_settings(SLAB_N, False), world=world, transport=transport, recut_every=3)
    mg.upload_state(pos, vel)
    D.assert_same_words(mg.diagnostics_raw(**SLAB_HIST), want[0], "step 0")
    owned = set()
    for k in range(SLAB_STEPS):
        mg.simulate()
        D.assert_same_words(mg.diagnostics_raw(**SLAB_HIST), want[k + 1], f"{world} slabs over {transport}, step {k + 1}")
        owned.add(tuple(mg.stats().owned[:world]))
    st = mg.stats()
    assert st.recuts >= 1, "no re-cut happened: not covered"
    assert len(owned) > 1, "the slab sizes never changed: the order-independence claim is not exercised"
    assert mg.diagnostics()["kinetic"] == _lib.diagnostics_dict(want[-1], mg.settings)["kinetic"]
    mg.close()


def test_one_object_per_rank_merges_with_add(single_domain_words):
    pos, vel, want = single_domain_words
    world, L = 3, sph.load_library()
    settings = sph.default_settings(SLAB_N, False)
    ranks = [M.MultiGpuSimulator(settings, world=world, rank=r, devices=[0], transport="mailbox") for r in range(world)]
    for mg in ranks:
        mg.upload_state(pos, vel)
    for k in range(SLAB_STEPS + 1):
        if k:
            for phase in (1, 2, 3, 4):
                for mg in ranks:
                    mg.step_phase(phase)
        parts = [mg.diagnostics_raw(**SLAB_HIST) for mg in ranks]
        assert all(0 < p.n < SLAB_N for p in parts) and sum(p.n for p in parts) == SLAB_N
        for p in parts[1:]:
            assert L.sph_diagnostics_add(C.byref(parts[0]), C.byref(p)) == 0
        D.assert_same_words(parts[0], want[k], f"ranks merged, step {k}")
    for mg in ranks:
        mg.close()


# ---- errors ----

def test_errors():
    L = sph.load_library()
    sim = make(64)
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.diagnose()  # before any state
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        sim.diagnostics_raw()
    sim.setup()
    with pytest.raises(sph.SphError, match=r"sph_diagnostics_host failed \(-4\)"):
        sim.diagnostics_raw()  # before the first sph_diagnose
    for kw in (dict(hist=3), dict(hist=-2), dict(hist="speed", value_range=(2.0, 1.0)),
               dict(hist="density", value_range=(0.0, float("inf"))), dict(hist="pressure", value_range=(float("nan"), 1.0))):
        with pytest.raises(sph.SphError, match=r"sph_diagnose failed \(-1\)"):
            sim.diagnose(**kw)
    o = _lib.diagnostics_options()
    o.struct_size = 0
    assert L.sph_diagnose(sim._h, C.byref(o)) == SPH_EINVAL
    assert L.sph_slab_diagnose(sim._h, 0, 0, 1, None) == SPH_ESTATE  # not a slab handle
    sim.diagnose(value_range=(2.0, 1.0))  # (no histogram: the range is not looked at)
    assert sim.diagnostics_raw().hist_field == -1
    sim.close()
    slab = make(64, flags=_lib.SPH_FLAG_EXTERNAL_STATE | _lib.SPH_FLAG_NO_READBACK, capacity=64)
    assert L.sph_diagnose(slab._h, None) == SPH_ESTATE
    auto = _lib.diagnostics_options("speed")
    assert L.sph_slab_diagnose(slab._h, 0, 0, 1, C.byref(auto)) == SPH_EINVAL
    assert L.sph_slab_diagnose(slab._h, 0, 0, 1, None) == SPH_ESTATE  # no buffers bound
    slab.close()
    mg = M.MultiGpuSimulator(sph.default_settings(4096, True), world=2, transport="loopback")
    with pytest.raises(sph.SphError, match=r"\(-4\)"):
        mg.diagnostics_raw()  # before any state
    mg.setup()
    with pytest.raises(sph.SphError, match=r"\(-1\)"):
        mg.diagnostics_raw(hist="speed")  # an automatic range
    with pytest.raises(sph.SphError, match=r"\(-1\)"):
        mg.diagnostics_raw(hist=9, value_range=(0.0, 1.0))
    assert mg.diagnostics_raw().n == 4096
    mg.close()


# ---- ./sph -m free writes the numbers ----

def test_cli_writes_stats_lines(tmp_path):
    def run(out, **env):
        os.makedirs(out)
        e = dict(os.environ, SPH_FREE_FRAMES="3", SPH_FREE_FRAMES_DIR=str(out), **env)
        r = subprocess.run([SPH, "-n", "4096", "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=e)
        assert r.returncode == 0, r.stderr
    run(tmp_path / "with", SPH_FREE_STATS="1")
    lines = [json.loads(l) for l in open(tmp_path / "with" / "stats.jsonl")]
    assert [l["frame"] for l in lines] == [0, 1, 2]
    sim = make(4096, random=True)
    sim.setup()
    for line in lines:
        sim.simulate()
        d = sim.diagnostics()
        for name in ("kinetic", "potential", "max_speed", "cfl", "min_rho", "mean_rho", "max_rho"):
            assert line[name] == float("%.17g" % d[name]) == d[name], name
        assert tuple(line["momentum"]) == d["momentum"] and tuple(line["com"]) == d["com"]
        assert line["saturated"] == d["saturated"] == 0
    assert lines[-1]["kinetic"] > 0
    sim.close()
    run(tmp_path / "without")
    assert sorted(os.listdir(tmp_path / "without")) == ["frame_%04d.ppm" % f for f in range(3)]
