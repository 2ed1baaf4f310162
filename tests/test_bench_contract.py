"""bench.py prints ONE JSON line with the driver's contract fields, the `roofline` and
(--full) `cpu_baseline` objects, and (N > 1) goes through the C++ multi-GPU driver."""
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_needs_a_gpu(have_gpu):
    if have_gpu:
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "GPU" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_single_gpu_line():
    d = run_bench("-n", "262144", "--steps", "6", "--warmup", "2", "--cpu-steps", "2", "--no-linked-leg", "--full")
    assert "other_configs" not in d   # the config 2 / config 4 legs ride on the default command only
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["vs_baseline"] is None
    assert d["full_run"] is False and "first 6 of the 100 steps" in d["metric"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None and "traffic_note" in r          # no PMC run of THIS command
    assert 0 < r["force_hit_fraction"] < 1 and r["force_valu_frac"] < 1
    # free fall: every recorded hit is an exact-zero pair and the filter drops it
    assert r["force_pair_bodies_per_launch"] <= r["force_hits_recorded_per_launch"]
    # the metric BASELINE.json names (the 100-step loop) is always measured, whatever --steps is
    f = d["full_run_100"]
    assert f["steps"] == 100 and f["value"] > 0 and f["roofline"]["bound"] == "hbm"
    assert abs(f["value"] - 262144 * 100 / (f["ms_per_step"] * 1e-3 * 100)) < 1e-3 * f["value"]
    assert set(f["kernel_ms_per_step"]) >= {"sort", "density", "force_integrate"}
    g = d["cpu_baseline"].get("gpu_same_window")
    assert g and g["ratio"] > 10
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["steps"] == 2 and "-march=native" in c["build"] and c["value"] > 0
    assert d["value"] > 10 * c["value"]


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_samples_a_large_output_with_a_fixed_seed(monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 1200)
    pos = np.arange(3000, dtype=np.float32).reshape(1000, 3)
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        b.dump_outputs(d1, {"positions": pos})
        b.dump_outputs(d2, {"positions": pos})
        a1, a2 = np.load(os.path.join(d1, "positions.npy")), np.load(os.path.join(d2, "positions.npy"))
    assert a1.dtype == np.float32 and a1.shape == (100, 3) and a1.nbytes <= 1200
    assert np.array_equal(a1, a2)                                   # the same rows every run
    rows = (a1[:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(pos[rows], a1)


def test_dump_outputs_writes_a_small_output_whole():
    b = _bench_module()
    pos = np.random.default_rng(1).random((4096, 3), dtype=np.float32)
    with tempfile.TemporaryDirectory() as d:
        b.dump_outputs(os.path.join(d, "out"), {"positions": pos})
        got = np.load(os.path.join(d, "out", "positions.npy"))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), pos.view(np.uint32))


@pytest.mark.gpu
def test_plain_line_is_lean_and_dumps_the_last_step():
    """Without --full the run times the K steps only: no replay, no extra legs, no CPU baseline.
    --dump-outputs writes the last timed step's positions, identical from run to run and equal
    to a fresh simulator's positions after the same K steps."""
    n, K = 262144, 4
    with tempfile.TemporaryDirectory() as d:
        runs = []
        for tag in ("a", "b"):
            out = os.path.join(d, tag)
            line = run_bench("-n", str(n), "--steps", str(K), "--warmup", "1", "--dump-outputs", out)
            runs.append((line, np.load(os.path.join(out, "positions.npy"))))
    (d1, p1), (_, p2) = runs
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d1, k
    assert d1["steps"] == K and d1["unit"] == "particle-steps/s" and d1["dtype"] == "f32"
    assert abs(d1["value"] - n * K / (d1["ms_per_step"] * 1e-3 * K)) < 1e-6 * d1["value"]
    for k in ("cpu_baseline", "full_run_100", "other_configs", "fast_math", "reference_structure"):
        assert k not in d1, k
    assert "valu_frac" not in d1["roofline"]
    assert p1.dtype == np.float32 and p1.shape == (n, 3)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    import cudafluidsimulator_amd as sph
    sim = sph.Simulator(sph.default_settings(n, True), device=0)
    sim.setup()
    t = sph.Times()
    for _ in range(K):
        sim.simulateAndTime(t)
    want = np.array(sim.getPosition(), copy=True)
    sim.close()
    assert np.array_equal(p1.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_full_line_bounds_its_secondary_legs_past_100_steps():
    """--full with a window longer than the 100-step loop: the linked-list and fast-math legs
    cover the first 100 steps only, the pair-count replay is left to `full_run_100`."""
    d = run_bench("-n", "262144", "--steps", "120", "--warmup", "1", "--cpu-steps", "0", "--full")
    assert d["steps"] == 120 and abs(d["value"] - 262144 * 120 / (d["ms_per_step"] * 1e-3 * 120)) < 1e-6 * d["value"]
    assert d["reference_structure"]["steps"] == 100 and d["fast_math"]["steps"] == 100
    assert "valu_frac" not in d["roofline"] and "full_run_100" in d["roofline"]["valu_frac_note"]
    f = d["full_run_100"]
    assert f["steps"] == 100 and f["roofline"]["valu_frac"] > 0


@pytest.mark.gpu
def test_multi_gpu_code_path_with_one_rank():
    """N > 1 runs one process per GPU through libsph_mgpu.so (ncclCommInitRank with a unique
    id handed out over torch.distributed).  A one-GPU box can run that path with one rank."""
    d = run_bench("-n", "262144", "--steps", "5", "--warmup", "1", "--cpu-steps", "0",
                  env={"SPH_BENCH_FORCE_MGPU": "1"})
    m = d["multi_gpu_driver"]
    assert m["host_syncs_per_step"] == 1.0 and m["slabs"] == 1 and m["owned"] == [262144]
    assert d["value"] > 0 and d["roofline"]["avg_launch_us"] > 0


@pytest.mark.gpu
def test_loopback_slab_study_line():
    d = run_bench("-n", "262144", "--steps", "5", "--warmup", "1", "--cpu-steps", "0", "--loopback-slabs", "4")
    m = d["multi_gpu_driver"]
    assert m["slabs"] == 4 and len(m["kernel_ms_per_step_per_slab"]) == 4 and sum(m["owned"]) == 262144
    assert "LOOPBACK" in d["config"]["parallelism"]
