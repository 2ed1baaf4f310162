"""The oracle itself on the grids of tests/grid_states.py, and every precondition tests/test_gpu_grids.py relies on,
without a GPU.

The oracle is pinned by known answers and by the independent restatement on the reference's 100^3 grid only.  Here
its densities after one step are held to tests/step_f64.py -- float64, brute force over all pairs, no grid and no
cell table -- on every grid of GRIDS: e_rho = |rho - rho64| / sum of terms, maximum over the rows.  The yardstick is
the same measure of the same oracle on a state(3001, 0.1, 100) of the 100^3 grid, taken in the same run."""
import functools

import numpy as np
import pytest

import grid_states as G
import step_f64 as S
from oracle import oracle as O

STEPS = 4


@functools.lru_cache(maxsize=None)
def run(name):
    """STEPS oracle steps of a grid's state (one for D1): the start, and rho / pos after every step"""
    if name == "yardstick":
        pos, vel = G.state(3001, 0.1, 100, 1)
        g = dict(cells=100, h=0.1, n=3001)
    else:
        pos, vel, g = G.grid_state(name)
    s = G.settings_for(g["n"], g["h"], g["cells"])
    ref = G.oracle_sim(s)
    ref.upload(pos, vel)
    out = []
    for _ in range(1 if name == "D1" else STEPS):
        ref.step()
        out.append(ref.download())
    ref.close()
    return s, pos, out


def max_e_rho(name):
    s, pos, out = run(name)
    rho64, Sd = S.density64(pos, **S.settings_args(s))
    return float(S.e_rho(out[0]["rho"], rho64, Sd).max()), rho64


# The error of a left-to-right fp32 sum of N terms of one sign is at most (N - 1) u relative to the sum (u = 2^-24 =
# 6e-8) and grows like sqrt(N) u when the roundings are independent; every term carries ~6 roundings of its own on
# top.  The sparse 100^3 state sums 1 to 3 terms per row; the crowded small grids (D2, D3, D6: 60 to 90 rows per
# cell) sum 300 to 700, and every row of D102's cluster sums all 1000 rows of it: sqrt(1000) = 32 times the
# yardstick's error is the most an honest sum may show, and FACTOR allows that (the run shows at most 10.2 times).  A
# missed or doubled neighbour cell drops or repeats whole terms: an error of the order of the sum itself, 1e-2 to 1
# in this measure, four orders of magnitude above the bound.
FACTOR = 32.0


@pytest.mark.parametrize("name", list(G.GRIDS))
def test_oracle_densities_against_float64_on_every_grid(name):
    """Measured (max e_rho over the rows, one step): yardstick 100^3 1.549e-07; D1 3.438e-07, D2 8.920e-07,
    D3 1.217e-06, D6 1.129e-06, D7 5.379e-07, D10h025 3.175e-07, D11 3.797e-07, D40 2.182e-07, D41 2.030e-07,
    D101 1.653e-07, D102 1.582e-06, D161h005 1.170e-07, D256 8.088e-08, D257 8.088e-08.  Rows above the rest density
    after step 1: D2 72 %, D3 71 %, D6 79 %, D102 33 % (its cluster).  Bound: FACTOR times the yardstick."""
    yard, _ = max_e_rho("yardstick")
    got, rho64 = max_e_rho(name)
    print(f"{name}: max e_rho {got:.3e}; yardstick (100^3) {yard:.3e}; bound {FACTOR * yard:.3e}")
    assert 0 < yard < 1e-6
    assert got <= FACTOR * yard
    g = G.GRIDS[name]
    if g["crowded"]:      # the share the GPU test's "pressure is on" assertion rests on
        rho = run(name)[2][0]["rho"]
        print(f"{name}: {100 * (rho > G.REST_DENSITY).mean():.0f} % of the rows above the rest density")
        assert (rho > G.REST_DENSITY).any() and (rho64 > 1000).any()


@pytest.mark.parametrize("name", G.STEP_GRIDS)
def test_no_position_leaves_the_grid_within_four_steps(name):
    s, pos, out = run(name)
    for k, st in enumerate(out, 1):
        G.assert_inside(st["pos"], s.h, int(s.numCellsPerDim), f"{name} after step {k}")


def test_one_cell_grid_loses_every_particle_in_its_first_step():
    """D = 1: the wall planes sit at h and boxDim - h = 0, so the step clamps every coordinate to h, cell 1 of a
    one-cell grid.  One step is all the oracle can take (its counting sort would index past its table)."""
    s, pos, out = run("D1")
    assert len(out) == 1 and (G.cells_of(out[0]["pos"], s.h) >= 1).any(axis=1).all()


def test_two_cell_grid_collapses_into_one_point():
    s, pos, out = run("D2")
    hf = np.float32(s.h)
    assert (out[0]["pos"] == hf).all() and (G.cells_of(out[0]["pos"], s.h) == 1).all()


def test_257_cells_keep_fp32_keys_equal_to_integer_keys():
    s, pos, out = run("D257")        # (grid_state asserted it for the start)
    for k, st in enumerate(out, 1):
        top = G.assert_oracle_keys_are_integer_keys(s, st["pos"], f"D257 after step {k}")
    assert top <= 252
    # ... and the rule is needed: with the top layers occupied the fp32 keys collide
    full, _ = G.state(3001, 0.1, 257, 1)
    assert not np.array_equal(O.cell_keys(s, full), G.integer_keys(full, 0.1, 257))


def test_key_widths_name_every_plan_reachable_from_a_grid():
    plans = {g["plan"] for g in G.GRIDS.values()}
    assert plans == {(8, 1), (10, 1), (8, 2), (10, 2), (8, 3), (10, 3)}
    for name, g in G.GRIDS.items():
        assert G.key_bits(g["cells"]) == g["bits"] and G.plan_of(g["bits"]) == g["plan"], name
    assert G.plan_of(32) == (8, 4) and G.plan_of(31) == (8, 4) and G.key_bits(1024) == 30


@pytest.mark.parametrize("name", list(G.CLICK_GRIDS))
def test_click_layers_without_an_owner_and_with_two(name):
    """click_state asserts the owner pattern; the oracle then shows the impulse applied twice, not at all, and once."""
    pos, vel, info = G.click_state(name)
    s = G.settings_for(len(pos), info["h"], info["cells"])
    plain, clicked = G.oracle_sim(s), G.oracle_sim(s)
    for ref in (plain, clicked):
        ref.upload(pos, vel)
        ref.step()
    clicked.click(*G.CLICK)
    G.assert_click_applied(plain.download()["vel"], clicked.download()["vel"], info)
    for px, py in G.EDGE_CLICKS:
        before = clicked.download()["vel"]
        clicked.click(px, py)
        assert (clicked.download()["vel"] != before).any(axis=1).sum() > 20, "an edge click must move something"
    plain.close(), clicked.close()


@pytest.mark.parametrize("name", list(G.SLABS))
def test_slab_states_never_hop_a_whole_layer(name):
    """max |v_z| dt < h at every step of the single domain (here: the oracle, which the single-domain library
    equals bit for bit), so the whole-slab-hop rule stays out of the slab tests"""
    pos, vel, sl = G.slab_state(name)
    s = G.settings_for(len(pos), sl["h"], sl["cells"])
    ref = G.oracle_sim(s)
    ref.upload(pos, vel)
    assert np.abs(vel[:, 2]).max() * s.timestep < s.h
    for step in range(1, sl["steps"] + 1):
        ref.step()
        if step in sl["clicks"]:
            ref.click(*G.CLICK)
        assert np.abs(ref.download()["vel"][:, 2]).max() * s.timestep < s.h, f"{name} step {step}"
    ref.close()
    if sl["cut_between"]:
        cuts = G.partition_layers(np.bincount(G.cells_of(pos, sl["h"])[:, 2], minlength=sl["cells"]), sl["world"])
        lo, hi = sl["cut_between"]
        assert any(lo < c <= hi for c in cuts[1:-1]), cuts
    if sl["thin"]:
        cuts = G.partition_layers(np.bincount(G.cells_of(pos, sl["h"])[:, 2], minlength=sl["cells"]), sl["world"])
        assert (np.diff(cuts) == 2).all(), cuts
