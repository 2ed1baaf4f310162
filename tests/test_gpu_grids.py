"""Grid build, step, click, slabs and field sample on grids other than the reference's 100^3 (tests/grid_states.py):
one grid per sort plan reachable from a grid (one, two and three passes of 8- and 10-bit digits, so the sorted
stream ends in either buffer), grids too small for a full 3 x 3 x 3 neighbourhood, click layers owned by no
reference thread and by two, slabs exactly two layers thick.  Against the C oracle with the same Settings, bit for
bit; tests/test_grids_cpu.py holds the oracle itself to float64 on the same grids and proves the preconditions."""
import functools

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
import field_sample_restatement as FS
import grid_states as G
from cudafluidsimulator_amd import _lib
from cudafluidsimulator_amd import mgpu as M
from helpers import assert_bit_equal
from oracle import oracle as O
from pair_counts import count
from test_gpu_linked import REL, rel_err
from test_gpu_parity import compare_state

pytestmark = pytest.mark.gpu
SWEEPS = ["list", "lds", "direct"]


def library_settings(n, h, cells):
    return G.settings_for(n, h, cells, factory=sph.default_settings)


def make_pair(pos, vel, h, cells, sweep, flags=0, key_order="flattened"):
    s = library_settings(len(pos), h, cells)
    sim = sph.Simulator(s, sweep=sweep, flags=flags, key_order=key_order)
    sim.upload_state(pos, vel)
    ref = G.oracle_sim(s)
    ref.upload(pos, vel)
    return sim, ref


def grid_pair(name, sweep, **kw):
    pos, vel, g = G.grid_state(name)
    return make_pair(pos, vel, g["h"], g["cells"], sweep, **kw) + (pos, g)


def check_grid_phase(sim, ref, pos, table_cells):
    """ids, keys and the cell table of sph_phase_grid against the oracle's keys -> stable sort -> table"""
    sim.phase("grid")
    g = sim.download_grid()
    keys = O.cell_keys(ref.settings, pos)
    perm = O.stable_sort(keys, table_cells)
    assert sim._L.sph_num_table_cells(sim._h) == table_cells == len(g["cells"])
    assert np.array_equal(g["ids"], perm)
    assert np.array_equal(g["keys"], keys[perm])
    cs, ce = O.cell_table(keys[perm], table_cells)
    occ = ce > cs
    assert np.array_equal(g["cells"][occ, 0], cs[occ]) and np.array_equal(g["cells"][occ, 1], ce[occ])
    assert not g["cells"][~occ].any()
    return keys


# ---- the grid phase on every plan ----

@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("name", list(G.GRIDS))
def test_grid_phase_and_first_step_on_every_sort_plan(name, sweep):
    """The fused first pass (hash, table clear, iota values) as the only pass (D <= 10), the first of two, and the
    first of three; the sorted stream in buffer 1 after one and three passes, in buffer 0 after two.  D1: one step
    is all there is -- it leaves every particle outside the grid."""
    sim, ref, pos, g = grid_pair(name, sweep)
    D = g["cells"]
    keys = check_grid_phase(sim, ref, pos, D ** 3)
    assert np.array_equal(keys, G.integer_keys(pos, g["h"], D))
    assert int(keys.max()).bit_length() <= g["bits"]
    sim.phase("density"); sim.phase("force"); sim.phase("readback")
    ref.step()
    compare_state(sim, ref, f"{name} {sweep}: after the phases")
    sim.close()
    ref.close()


# ---- steps ----

@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("name", G.STEP_GRIDS)
def test_four_steps_on_every_sort_plan(name, sweep):
    """Four steps, the third one timed (it queues the next step's grid build ahead, into the second table).  D2:
    from step 2 on all 700 rows are coincident in one cell.  D2, D3, D6, D102: pressure is on."""
    sim, ref, pos, g = grid_pair(name, sweep)
    t = sph.Times()
    for k in range(1, 5):
        if k == 3:
            sim.simulateAndTime(t)
        else:
            sim.simulate()
        ref.step()
        compare_state(sim, ref, f"{name} {sweep}: step {k}")
        if k == 1 and g["crowded"]:
            assert (sim.download_state()["rho"] > G.REST_DENSITY).any(), "the pressure term must be exercised"
    assert t.iters == 1
    sim.close()
    ref.close()


@pytest.mark.parametrize("name", ["D2", "D7", "D102", "D257"])
def test_pair_counters_off_the_reference_grid(name):
    """SPH_FLAG_COUNT_PAIRS on grids with clipped neighbourhoods everywhere (D2), one pass (D7) and three passes of
    either digit (D102, D257): candidate tests, hits and pair bodies equal the plain CPU count, two steps."""
    sim, ref, pos, g = grid_pair(name, "list", flags=_lib.SPH_FLAG_COUNT_PAIRS)
    order = None
    for k in (1, 2):
        before = ref.download()
        ref.step()
        c = count(before["pos"], before["vel"], ref.download()["rho"], order, h=g["h"], cells=g["cells"])
        assert c["tests"] == ref.last_pair_tests()
        sim.simulate()
        dbg = sim.debug_counters()
        kt = sim.kernel_times(reset=True)
        got = (kt.pair_tests, int(dbg[15]), kt.pair_hits)
        print(f"{name} step {k}: (tests, hits, bodies) = {got}, CPU count {(c['tests'], c['hits'], c['bodies'])}")
        assert kt.pair_tests == c["tests"], f"{name} step {k}: pair_tests"
        assert got == (c["tests"], c["hits"], c["bodies"]), f"{name} step {k}"
        order = c["order_out"]
    compare_state(sim, ref, f"{name}: counted steps")
    sim.close()
    ref.close()


@pytest.mark.parametrize("name", ["D6", "D102"])
def test_linked_sweep_off_the_reference_grid(name):
    """The linked-list backend on a one-pass and a three-pass grid: one step against the oracle at the tolerance
    of tests/test_gpu_linked.py (list order is a race: rounding, not bits)."""
    sim, ref, pos, g = grid_pair(name, "linked")
    sim.simulate()
    ref.step()
    got, want = sim.download_state(), ref.download()
    assert (want["rho"] > G.REST_DENSITY).any()
    assert rel_err(got["rho"], want["rho"], 1e-30) <= REL
    assert rel_err(got["pos"], want["pos"], 1e-3) <= REL
    assert rel_err(np.array(sim.getPosition()), want["pos"], 1e-3) <= REL
    sim.close()
    ref.close()


# ---- Morton keys ----

@pytest.fixture
def morton_oracle():
    O.set_key_order("morton")
    try:
        yield
    finally:
        O.set_key_order("flattened")


MORTON = {"D2": (2, 0.1, 700), "D7": (7, 0.1, 2500), "D33h03": (33, 0.3, 3001), "D129": (129, 0.1, 3001)}


@pytest.mark.parametrize("name", list(MORTON))
def test_morton_keys_off_the_reference_grid(name, morton_oracle):
    """Tables of 8, 512, 64^3 and 256^3 interleaved keys (3, 9, 18 and 24 bits: one pass of either digit, two and
    three passes): the grid phase, then two steps, against the Morton-keyed oracle."""
    D, h, n = MORTON[name]
    pos, vel = G.state(n, h, D, 5)
    sim, ref = make_pair(pos, vel, h, D, "direct", key_order="morton")
    side = 1
    while side < D:
        side *= 2
    assert O.num_keys(D) == side ** 3
    keys = check_grid_phase(sim, ref, pos, side ** 3)
    c = G.cells_of(pos, h)
    assert np.array_equal(keys, sum(((c[:, a] >> b) & 1) << (3 * b + a) for a in range(3) for b in range(10)).astype(np.uint32))
    sim.phase("density"); sim.phase("force"); sim.phase("readback")
    ref.step()
    compare_state(sim, ref, f"morton {name}: step 1")
    sim.simulate(); ref.step()
    compare_state(sim, ref, f"morton {name}: step 2")
    sim.close()
    ref.close()


# ---- the click on layers without an owner and with two ----

@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("name", list(G.CLICK_GRIDS))
def test_click_on_layers_with_no_owner_and_with_two(name, sweep):
    """(h, D) = (0.3, 33) and (0.07, 143): reference threads 14 and 15 both land on z-layer 14 and none on 15 (and so
    on, grid_states.owners).  One step, the click, and the velocities are the oracle's; the ORACLE's velocities show
    the impulse applied twice (-10 on v_z in the centre cell), not at all, and once.  Then the two clicks whose
    footprint leaves the grid (cy = D; cx = 0), and two more steps."""
    pos, vel, info = G.click_state(name)
    sim, ref = make_pair(pos, vel, info["h"], info["cells"], sweep)
    plain = G.oracle_sim(ref.settings)
    plain.upload(pos, vel)
    sim.simulate(); ref.step(); plain.step()
    sim.moveParticles(G.CLICK); ref.click(*G.CLICK)
    want = ref.download()["vel"]
    assert_bit_equal(sim.download_state()["vel"], want, f"{name} {sweep}: vel after the click")
    G.assert_click_applied(plain.download()["vel"], want, info)
    plain.close()
    for px, py in G.EDGE_CLICKS:
        sim.moveParticles((px, py)); ref.click(px, py)
        after = ref.download()["vel"]
        assert (after != want).any(axis=1).sum() > 20, "the edge click moved something"
        assert_bit_equal(sim.download_state()["vel"], after, f"{name} {sweep}: vel after the click at ({px}, {py})")
        want = after
    for k in (2, 3):
        sim.simulate(); ref.step()
        compare_state(sim, ref, f"{name} {sweep}: step {k}")
    sim.close()
    ref.close()


# ---- slabs ----

@functools.lru_cache(maxsize=None)
def single_domain(name):
    """The single domain's run of a slab case (once for all transports), and the precondition that keeps the
    whole-slab-hop rule out of the test: max |v_z| dt < h at every step"""
    pos, vel, sl = G.slab_state(name)
    s = library_settings(len(pos), sl["h"], sl["cells"])
    sim = sph.Simulator(s)
    sim.upload_state(pos, vel)
    assert np.abs(vel[:, 2]).max() * s.timestep < s.h
    for step in range(1, sl["steps"] + 1):
        if step in sl["clicks"]:
            sim.mouseClicked, sim.clickCoords = True, G.CLICK
        sim.simulate()
        assert np.abs(sim.download_state()["vel"][:, 2]).max() * s.timestep < s.h, f"step {step}: a row may hop a whole layer"
    st = sim.download_state()
    host = np.array(sim.getPosition(), copy=True)
    sim.close()
    return st, host


@pytest.mark.parametrize("transport", ["loopback", "streams"])
@pytest.mark.parametrize("name", list(G.SLABS))
def test_thin_slabs_equal_single_domain(name, transport):
    """D8x4: four slabs of exactly two layers, each nothing but its two boundary layers.  D7x3: 2 + 2 + 3 or the
    like.  click33x4: the click state of (0.3, 33), a cut through the layers 14..16 of the owner triple, clicks at
    steps 2 and 4 -- every slab applies the impulse to the layers it owns, twice, never or once."""
    pos, vel, sl = G.slab_state(name)
    want, want_host = single_domain(name)
    world = sl["world"]
    s = library_settings(len(pos), sl["h"], sl["cells"])
    mg = M.MultiGpuSimulator(s, world=world, transport=transport)
    mg.upload_state(pos, vel)
    hist = np.bincount(G.cells_of(pos, sl["h"])[:, 2], minlength=sl["cells"])
    cuts = G.partition_layers(hist, world)
    cum = np.concatenate([[0], np.cumsum(hist)])
    owned = list(mg.stats().owned[:world])
    assert owned == [int(cum[b] - cum[a]) for a, b in zip(cuts, cuts[1:])], "the slabs hold the rows of the expected layers"
    if sl["thin"]:
        assert cuts == [0, 2, 4, 6, 8] and min(owned) > 0
    if sl["cut_between"]:
        lo, hi = sl["cut_between"]
        inside = [c for c in cuts[1:-1] if lo < c <= hi]
        assert inside and hist[lo:hi + 1].min() >= 25 * G.PER_CELL, cuts
    for step in range(1, sl["steps"] + 1):
        if step in sl["clicks"]:
            mg.mouseClicked, mg.clickCoords = True, G.CLICK
        mg.simulate()
    got = mg.download_state()
    assert got["written"] == len(pos)
    for k in ("pos", "vel", "rho"):
        assert_bit_equal(got[k], want[k], f"{name} {transport}: {k}")
    assert_bit_equal(np.array(mg.getPosition()), want_host, f"{name} {transport}: getPosition()")
    assert mg.stats().steps == sl["steps"]
    mg.close()


def test_too_many_slabs_for_the_grid_is_an_error():
    pos, vel = G.state(2500, 0.1, 7, 3)
    mg = M.MultiGpuSimulator(library_settings(len(pos), 0.1, 7), world=4, transport="loopback")
    with pytest.raises(sph.SphError, match="too many slabs for the grid"):
        mg.upload_state(pos, vel)
    mg.close()


# ---- the field sample ----

@pytest.mark.parametrize("name", ["D7", "D2"])
def test_field_sample_on_a_small_grid(name, monkeypatch):
    """A 9 x 9 x 9 lattice, seven points per axis inside the box and one outside on either side, so that every
    point's neighbourhood is clipped on some axis (D2: on every axis): density and speed, tile path and plain path,
    against the numpy restatement fed by the grid the sampler walked."""
    pos, vel, g = G.grid_state(name)
    D, h = g["cells"], g["h"]
    sim = sph.Simulator(library_settings(len(pos), h, D))
    sim.upload_state(pos, vel)
    sp = float(G.box_of(h, D)) / 7
    origin, spacing, shape = (-sp / 2,) * 3, (sp,) * 3, (9, 9, 9)
    axis, outside = FS.cells_of(FS.lattice_axis(origin[0], sp, 9), h, D)
    assert outside.tolist() == [True] + [False] * 7 + [True] and axis[1] == 0 and axis[7] == D - 1
    grid = None
    for field in ("density", "speed"):
        out = {}
        for plain in ("0", "1"):
            monkeypatch.setenv("SPH_SAMPLE_PLAIN", plain)
            out[plain] = sim.sample_field(field, origin, spacing, shape)
        if grid is None:
            gr, st = sim.download_grid(), sim.download_state()
            ids = gr["ids"].astype(np.int64)
            grid = (st["pos"][ids], st["vel"][ids], st["rho"][ids], gr["cells"])
        s = sim.settings
        want = FS.sample(*grid, s.h, s.d_kernel_coeff, D, field, origin, spacing, shape)
        assert (want[1:8, 1:8, 1:8] > 0).all() and not want[0].any() and not want[:, :, 8].any()
        for plain in ("0", "1"):
            assert out[plain].dtype == want.dtype and np.array_equal(out[plain].view(np.uint32), want.view(np.uint32)), \
                f"{name} {field}: SPH_SAMPLE_PLAIN={plain}"
    sim.close()
