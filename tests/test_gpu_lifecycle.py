"""A handle gives back what it took: create / use / destroy cycles that go through every buffer the handle allocates
late or resizes (the frame and its resize, the field frame, the sample's grow path, the diagnostics block, the initial
copy, the staged upload, the trace's base event), and the device memory in use after the 8th cycle against the 2nd.
The bound is one particle stream (n float4 = 4 MiB): any of the per-particle buffers leaked once per cycle would show
six times over.  An event or an 8-byte block is invisible here: tests/test_owned_cpu.py covers those."""
import torch  # (before the HIP library is loaded, as in test_slab.py)

import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib
from cudafluidsimulator_amd import mgpu as M

N = 262144
STREAM_BYTES = N * 16
CYCLES = 8


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def growth_over_cycles(cycle):
    """device bytes in use after the last cycle minus those after the second (the first two warm the allocators);
    `cycle(probe)` calls probe() once while its object is alive"""
    used, alive = [], []
    for _ in range(CYCLES):
        cycle(lambda: alive.append(used_bytes()))
        used.append(used_bytes())
    growth = used[-1] - used[1]
    print(f"device memory in use after each cycle, MiB: {[round(u / 2**20, 2) for u in used]}; growth {growth} bytes; "
          f"while alive, MiB: {[round(a / 2**20, 2) for a in alive]}")
    # the probe sees what an object holds: alive, at least its four particle streams more than after it is gone
    assert alive[-1] - used[-1] >= 4 * STREAM_BYTES
    return growth


def single_domain_cycle(sweep, flags, probe):
    sim = sph.Simulator(sph.default_settings(N, True), sweep=sweep, flags=flags)
    sim.setup()
    t = sph.Times()
    sim.simulateAndTime(t)
    sim.simulateAndTime(t)
    sim.simulate()
    for w, h in ((64, 48), (96, 64)):  # (the second size: a resize)
        assert sim.render(w, h).shape == (h, w, 3)
    for w, h in ((64, 48), (96, 64)):
        sim.render_field("speed", width=w, height=h)
        assert sim.frame_host().shape == (h, w, 3)
    for d in (8, 16):  # (the second lattice: the buffers grow)
        assert sim.sample_field("density", origin=(1.0, 1.0, 1.0), spacing=8.0 / d, shape=(d, d, d)).shape == (d, d, d)
    out = sim.diagnostics(hist="speed")
    assert out["raw"]["n"] == N and int(out["raw"]["hist"].sum()) == N
    probe()
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sweep,flags", [("list", 0), ("list", _lib.SPH_FLAG_MAPPED_POSITIONS), ("direct", 0)],
                         ids=["list", "list-mapped-positions", "direct"])
def test_single_domain_handle_gives_back_what_it_took(sweep, flags, monkeypatch):
    monkeypatch.setenv("SPH_STEP_TRACE", "1")  # (the trace's base event is one of the handle's resources)
    assert growth_over_cycles(lambda probe: single_domain_cycle(sweep, flags, probe)) < STREAM_BYTES


@pytest.mark.gpu
def test_two_slabs_give_back_what_they_took(monkeypatch):
    """faces of 300 rows are far too small for a layer of this state (as in test_mgpu.py's tiny faces): every step
    has an overflow round, so the slabs' overflow buffers (ensure_extra) are part of the cycle"""
    monkeypatch.setenv("SPH_STEP_TRACE", "1")

    def cycle(probe):
        mg = M.MultiGpuSimulator(sph.default_settings(N, True), world=2, transport="loopback", face_capacity=300)
        mg.setup()
        mg.simulate()
        mg.simulate()
        assert mg.diagnostics()["raw"]["n"] == N
        assert mg.stats().overflow_rounds == 2
        probe()
        mg.close()

    assert growth_over_cycles(cycle) < STREAM_BYTES
