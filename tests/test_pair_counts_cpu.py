"""tests/pair_counts.py (the CPU restatement of the library's pair counters) against hand counts and against the
oracle's own pair-test count -- two independent derivations -- on every state the GPU file uses.  No GPU."""
import numpy as np
import pytest

import pair_count_states as PS
from helpers import clustered_state, nasty_state
from oracle import oracle as O
from pair_counts import count, pool_outcomes, reference_velocity, waves

H = np.float32(0.1)


def oracle_tests(pos, h=0.1, cells=100):
    """oracle_pair_tests on the oracle's own keys, sort and cell table."""
    n = len(pos)
    if n == 0:
        return 0, np.zeros(0, np.uint32)
    s = O.make_settings(n, False)
    s.h, s.boxDim, s.numCellsPerDim = h, h * cells, cells
    keys = O.cell_keys(s, pos)
    perm = O.stable_sort(keys, cells ** 3)
    cs, ce = O.cell_table(keys[perm], cells ** 3)
    return O.pair_tests(s, pos[perm], cs, ce), perm


def test_one_particle():
    c = count(np.array([[5.05, 5.05, 5.05]], np.float32))
    assert (c["tests"], c["hits"], c["bodies"]) == (1, 1, 1)


@pytest.mark.parametrize("dist,hits", [(H / np.float32(2), 4), (H, 4), (np.nextafter(H, np.float32(1)), 2)])
def test_two_particles_at_half_h_exactly_h_and_the_next_float(dist, hits):
    """x = 0 and x = dist are exact in fp32 and so is their difference: d2 = dist * dist against h * h.
    Both sit in neighbouring cells (or one): 2 x 2 candidate tests."""
    a = np.float32(0)
    b = a + dist
    assert b - a == dist
    pos = np.array([[a, 5.05, 5.05], [b, 5.05, 5.05]], np.float32)
    c = count(pos)
    assert (c["tests"], c["hits"], c["bodies"]) == (4, hits, hits)


def test_lattice_one_particle_per_cell():
    """3 x 3 x 3 particles 0.09 apart at 4.06, 4.15, 4.24: one per cell (40, 41, 42).  Tests: the centre has 27
    candidates, a face 18, an edge 12, a corner 8.  Hits: axis neighbours are 0.09 apart (inside h), diagonal ones
    0.127 and more (outside): 27 self pairs + 2 x 54 axis pairs."""
    g = 4.06 + 0.09 * np.arange(3)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    c = count(pos)
    assert c["tests"] == 27 + 6 * 18 + 12 * 12 + 8 * 8 == 343
    assert c["hits"] == c["bodies"] == 27 + 2 * 54 == 135
    assert sorted(c["tests_i"]) == sorted([27] + [18] * 6 + [12] * 12 + [8] * 8)
    assert sorted(c["hits_i"]) == sorted([7] + [6] * 6 + [5] * 12 + [4] * 8)


def test_corner_cell_has_eight_neighbour_cells():
    """One particle in each of the 8 cells around the grid's corner: each tests all 8; a ninth far away tests 1."""
    g = np.array([0.05, 0.15], np.float32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pos = np.concatenate([pos, np.array([[9.95, 9.95, 9.95]], np.float32)])
    c = count(pos)
    assert c["tests"] == 8 * 8 + 1
    assert c["tests_i"][0] == 8 and c["tests_i"][-1] == 1


def test_filter_counts_by_hand():
    """Four coincident particles (16 hits).  Two share the sampled majority velocity: their 4 mutual pairs (the two
    self pairs included) are dropped; under pressure none is; filter off: none is."""
    pos = np.full((4, 3), 5.05, np.float32)
    vel = np.array([[1, 2, 3], [1, 2, 3], [0, 0, 0], [4, 4, 4]], np.float32)
    rho = np.full(4, 500, np.float32)
    c = count(pos, vel, rho)
    assert (c["tests"], c["hits"], c["bodies"]) == (16, 16, 12) and list(c["quiet"]) == [True, True, False, False]
    assert count(pos, vel, np.full(4, 1500, np.float32))["bodies"] == 16
    assert count(pos, vel, rho, zero_pair_filter=False)["bodies"] == 16
    one_wet = rho.copy(); one_wet[0] = 1001
    assert count(pos, vel, one_wet)["bodies"] == 15          # only the self pair of the other quiet row goes
    assert count(pos, np.zeros((4, 3), np.float32), rho)["bodies"] == 0   # every row quiet
    # the reference velocity is drawn from the order the grid build starts from: ties go to the first sampled row
    v2 = np.array([[7, 7, 7], [1, 2, 3]], np.float32)
    assert list(reference_velocity(v2, np.array([0, 1]))) == [7, 7, 7]
    assert list(reference_velocity(v2, np.array([1, 0]))) == [1, 2, 3]


def test_owned_rows_count_halo_rows_are_candidates_only():
    pos, _ = nasty_state(3000, 1)
    full = count(pos)
    parts = [count(pos, owned=m) for m in (pos[:, 2] < 4.0, pos[:, 2] >= 4.0)]
    assert sum(p["tests"] for p in parts) == full["tests"] and sum(p["hits"] for p in parts) == full["hits"]


def test_cutoff_pairs_by_hand():
    """Isolated pairs at d2 = h*h -1, 0, +1, +2 ulps and coincident pairs.  h = 0.1f, 0.2f: d2 <= h*h.  h = 0.25f:
    sqrtf(h*h + 1 ulp) <= h as well, so that pair is a hit (the force sweep's viscosity term tests r, not r^2)."""
    for h, cells, inside in ((0.1, 100, (-1, 0)), (0.2, 32, (-1, 0)), (0.25, 32, (-1, 0, 1))):
        pos, vel, _, _, picks = PS.cutoff(h, cells, 0)
        c = count(pos, h=h, cells=cells)
        hits = len(pos) + 2 * sum(len(picks[s]) for s in inside) + 2 * len(picks["same"])
        assert c["hits"] == hits, h
        for s in PS.CUT_STEPS:
            for a, b in picks[s]:
                assert c["hits_i"][a] == c["hits_i"][b] == (2 if s in inside else 1), (h, s)


@pytest.mark.parametrize("name", list(PS.STATES))
def test_tests_equal_the_oracles_count_on_every_state_of_the_gpu_file(name):
    pos, vel, h, cells = PS.state(name)
    c = count(pos, h=h, cells=cells)
    want, perm = oracle_tests(pos, h, cells)
    assert c["tests"] == want
    assert np.array_equal(c["order_out"], perm)              # the step's sorted order, derived twice as well
    assert c["tests"] >= c["hits"] >= len(pos) and c["bodies"] == c["hits"]


def test_tests_equal_the_oracles_count_on_the_issues_two_states():
    for pos in (clustered_state(3000, 5)[0], nasty_state(3000, 0)[0]):
        assert count(pos)["tests"] == oracle_tests(pos)[0]


def test_clustered_state_has_runs_longer_than_the_lds_slice():
    """What the two dense states are for: runs (three x-adjacent cells) longer than the 384 candidates a wave stages
    in LDS, so the density sweep walks them from global memory; the block stays below (staged walk, 64 per cell)."""
    c = count(PS.state("clustered")[0])
    assert c["runmax_i"].max() > 384 and (c["runmax_i"] > 384).sum() > 5000
    b = count(PS.state("block")[0])
    assert 128 < b["runmax_i"].max() <= 384
    # and with a 20000-word pool (78 quads per sub-pool) no wave of it fits: every wave reserves 128 quads or more
    assert waves(c)[2].min() >= 128 and pool_outcomes(c, 20000) == {(0, 0)}


def test_mixture_holds_all_four_kinds_of_row():
    """The cut of co_moving_mixture: quiet cloud rows, co-moving rows under pressure, rows with a velocity of their
    own, the particle at rest; the filter drops some pairs and keeps some."""
    pos, vel, h, cells = PS.state("mixture")
    ref = O.OracleSim(len(pos), False)
    ref.upload(pos, vel)
    ref.step()
    rho = ref.download()["rho"]
    c = count(pos, vel, rho)
    assert 0 < c["bodies"] < c["hits"]
    common = (vel == reference_velocity(vel, np.arange(len(pos)))).all(axis=1)
    assert c["quiet"].any() and (common & (rho > 1000)).any() and (~common).any() and (vel == 0).all(axis=1).sum() == 1
    assert (common & (rho > 1000)).sum() > 100 and len(pos) < 5000
