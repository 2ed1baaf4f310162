"""SPH_SWEEP_LINKED: the reference's own neighbour structure (per-cell linked lists
built by atomic pushes, simulator.cu:44-55,133-147) as an alternative backend.

The order of a list is decided by a race, exactly as in the reference, so every
fp32 sum may be taken in a different order from the oracle's canonical one:
results are compared at the north star's tolerance (1e-5 relative), NOT bit for
bit -- except where a sum has at most two terms (fp32 addition is commutative).
The oracle itself is pinned bit for bit to the reference's kernels executed on the host
under the schedule that yields the canonical order; under another schedule those same
kernels differ from it by rounding of this size (tests/test_reference_pin_cpu.py,
DESIGN.md section 2)."""
import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib
from helpers import assert_bit_equal, clustered_state, dense_block
from oracle import oracle as O

pytestmark = pytest.mark.gpu
REL = 1e-5  # BASELINE.json north-star tolerance


def make_pair(n, random_init, flags=0, pos=None, vel=None):
    s = sph.default_settings(n, random_init)
    sim = sph.Simulator(s, sweep="linked", flags=flags)
    ref = O.OracleSim(n, random_init)
    if pos is None:
        sim.setup()
        ref.setup()
    else:
        sim.upload_state(pos, vel)
        ref.upload(pos, vel)
    return sim, ref


def rel_err(got, want, floor):
    return float((np.abs(got - want) / np.maximum(np.abs(want), floor)).max())


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_particles_are_exact(n):
    sim, ref = make_pair(n, False)
    for _ in range(5):
        sim.simulate()
        ref.step()
    g, r = sim.download_state(), ref.download()
    for k in ("pos", "vel", "rho", "prs"):
        assert_bit_equal(g[k], r[k], k)
    sim.close()


def test_one_step_on_clustered_state():
    pos, vel = clustered_state(30000, 7)
    sim, ref = make_pair(len(pos), False, flags=_lib.SPH_FLAG_STORE_FORCE, pos=pos, vel=vel)
    sim.simulate()
    ref.step()
    g, r = sim.download_state(), ref.download(want_force=True)
    assert rel_err(g["rho"], r["rho"], 1e-30) <= REL
    f = sim.download_force()
    scale = np.abs(r["force"]).max()
    assert np.abs(f - r["force"]).max() <= 1e-4 * scale  # sums with cancellation
    assert rel_err(g["pos"], r["pos"], 1e-3) <= REL
    assert rel_err(np.array(sim.getPosition()), r["pos"], 1e-3) <= REL
    sim.close()


def test_pressure_term_dense_block():
    pos = dense_block(16)
    sim, ref = make_pair(len(pos), False, pos=pos)
    for _ in range(3):
        sim.simulate()
        ref.step()
    g, r = sim.download_state(), ref.download()
    assert (r["prs"] > 0).sum() > 1000
    assert rel_err(g["rho"], r["rho"], 1e-30) <= REL
    assert rel_err(g["pos"], r["pos"], 1e-3) <= 1e-4  # three steps of a pressure blast
    sim.close()


def test_north_star_grid_100_steps():
    sim, ref = make_pair(8192, False)
    times = sph.Times()
    for _ in range(100):
        sim.simulateAndTime(times)
    ref.step(100)
    got, want = np.array(sim.getPosition()), ref.download()["pos"]
    assert rel_err(got, want, 1e-30) <= REL
    assert times.iters == 100 and times.sphUpdate > 0 and times.buildGrid > 0
    sim.close()


def test_pair_test_count_equals_the_oracles():
    sim, ref = make_pair(20000, True, flags=_lib.SPH_FLAG_COUNT_PAIRS)
    sim.simulate()
    ref.step()
    sim.sync()
    assert sim.kernel_times().pair_tests == ref.last_pair_tests()
    sim.close()


def test_unsupported_calls_fail_loudly():
    sim, _ = make_pair(1000, True)
    sim.simulate()
    with pytest.raises(sph.SphError):
        sim.moveParticles((400, 300))
    with pytest.raises(sph.SphError):
        sim.download_grid()
    with pytest.raises(sph.SphError):
        sph.Simulator(sph.default_settings(100, True), sweep="linked", math="fast")
    sim.close()
