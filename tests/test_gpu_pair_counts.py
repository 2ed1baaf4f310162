"""The three numbers the library reports about its own work -- SphKernelTimes.pair_tests, sph_debug_counters()[15]
(hits recorded) and SphKernelTimes.pair_hits (pair bodies evaluated), what bench.py's roofline fractions divide by --
as exact integers against a plain CPU count (tests/pair_counts.py), step by step, on the smallest states at which
the density sweep's candidate walk, the hit stream, the zero-pair filter and the host's bookkeeping can go wrong.
Every tolerance is zero."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in test_slab.py: the slab test drives torch-owned buffers)

import cudafluidsimulator_amd as sph
import pair_count_states as PS
import slab_rehearsal as S
from cudafluidsimulator_amd import _lib
from oracle import oracle as O
from pair_counts import count, pool_outcomes

pytestmark = pytest.mark.gpu
COUNT = _lib.SPH_FLAG_COUNT_PAIRS


def settings_for(n, h, cells, cls=sph.default_settings):
    s = cls(n, False)
    if (h, cells) != (0.1, 100):   # test_gpu_parity._custom_pair's settings
        s.h, s.boxDim, s.numCellsPerDim = h, h * cells, cells
        hf = np.float32(s.h)
        s.v_kernel_coeff = float(np.float32(45.0) / (np.float32(3.14159265) * np.float32(float(hf) ** 6)))
        s.d_kernel_coeff = float(np.float32(315.0) / (np.float32(64.0) * np.float32(3.14159265) * np.float32(float(hf) ** 9)))
    return s


def make(name, sweep="list", flags=COUNT):
    pos, vel, h, cells = PS.state(name)
    n = len(pos)
    s = settings_for(n, h, cells)
    sim = sph.Simulator(s, sweep=sweep, flags=flags)
    sim.upload_state(pos, vel)
    ref = O.OracleSim(n, False)
    if (h, cells) != (0.1, 100):
        C.memmove(C.byref(ref.settings), C.byref(s), C.sizeof(s))
        ref.close()
        ref._h = O.lib().oracle_sim_create(C.byref(ref.settings))
    ref.upload(pos, vel)
    return sim, ref, h, cells


def cpu_step(ref, order, h, cells, filter_on=True, advance=True):
    """The CPU count of the step the oracle is about to take (and takes)."""
    before = ref.download()
    if advance:
        ref.step()
    rho = ref.download()["rho"]
    c = count(before["pos"], before["vel"], rho, order, h=h, cells=cells, zero_pair_filter=filter_on)
    if advance and len(rho):
        assert c["tests"] == ref.last_pair_tests()      # (the oracle's own count: a third derivation)
    return c


def read(sim, reset=True):
    dbg = sim.debug_counters()
    kt = sim.kernel_times(reset=reset)
    assert dbg[0] == kt.pair_tests and dbg[14] == kt.pair_hits and not any(dbg[1:14])
    return kt.pair_tests, int(dbg[15]), kt.pair_hits, kt.steps


def check_steps(sim, ref, h, cells, steps, sweep="list", filter_on=True, order=None, what="", do_step=None):
    for k in range(1, steps + 1):
        c = cpu_step(ref, order, h, cells, filter_on)
        (do_step or sim.simulate)()
        got = read(sim)
        want = (c["tests"], c["hits"], c["bodies"]) if sweep == "list" else (c["tests"], 0, 0)
        print(f"{what} step {k}: (tests, hits, bodies) = {got[:3]}, CPU count {want}")
        assert got == want + (1,), f"{what}, step {k}"
        order = c["order_out"]
    return order


# ---- edges of a wave and a launch; clipped runs; long runs; the cut-off ----

LIST_STATES = ["cube0", "cube1", "cube2", "cube63", "cube64", "cube65", "cube129", "shell", "nasty0", "nasty1", "nasty2",
               "clustered", "block", "cut0.1", "cut0.2", "cut0.25"]


@pytest.mark.parametrize("name", LIST_STATES)
def test_list_sweep_counts_are_the_cpu_counts(name):
    """cube*: waves with 1..64 valid lanes, one and several launches' worth, nothing at all.  shell / nasty*: runs
    clipped by the walls (8 / 12 / 18 neighbour cells), coincident particles, positions on cell boundaries.
    clustered: runs longer than the LDS slice (the walk from global memory).  block: pressure on (rows that are
    never quiet).  cut*: pairs at d2 = h*h and one ulp either side, on the sign-bit path (h = 0.1, 0.2) and the
    general hit-bit path (h = 0.25, where d2 = h*h + 1 ulp is a hit)."""
    sim, ref, h, cells = make(name)
    check_steps(sim, ref, h, cells, 1 if name == "clustered" else 2, what=name)
    sim.close()


@pytest.mark.parametrize("sweep", ["lds", "direct", "linked"])
@pytest.mark.parametrize("name", LIST_STATES)
def test_every_sweep_counts_the_same_candidates(name, sweep):
    """pair_tests is a property of the state, not of the sweep; pair_hits and [15] are the list sweep's and stay 0.
    Same states and steps as the list sweep's test, except linked: it matches the oracle to rounding only, so only
    its first step starts from a known state."""
    sim, ref, h, cells = make(name, sweep)
    check_steps(sim, ref, h, cells, 1 if sweep == "linked" or name == "clustered" else 2, sweep=sweep, what=f"{name} {sweep}")
    sim.close()


# ---- the zero-pair filter ----

@pytest.mark.parametrize("filt", ["1", "0"])
@pytest.mark.parametrize("name", ["mixture", "at_rest"])
def test_filter_drops_exactly_the_pairs_of_two_quiet_rows(name, filt, monkeypatch):
    """mixture: quiet cloud rows, co-moving rows under pressure (kept), rows with velocities of their own, one at
    rest: 0 < bodies < hits.  at_rest: every row quiet, bodies == 0 (the shortcut), hits exact.  Filter off: bodies
    == hits.  Three steps: the reference velocity is drawn from the previous step's sorted order."""
    monkeypatch.setenv("SPH_ZERO_PAIR_FILTER", filt)
    sim, ref, h, cells = make(name)
    if name == "mixture":
        c = count(*PS.state(name)[:2], rho=_rho_of_first_step(name), zero_pair_filter=filt == "1")
        assert (0 < c["bodies"] < c["hits"]) if filt == "1" else (c["bodies"] == c["hits"])
    check_steps(sim, ref, h, cells, 3, filter_on=filt == "1", what=f"{name} filter {filt}")
    if name == "at_rest" and filt == "1":
        sim.simulate()
        assert read(sim)[2] == 0
    sim.close()


def _rho_of_first_step(name):
    pos, vel, h, cells = PS.state(name)
    ref = O.OracleSim(len(pos), False)
    ref.upload(pos, vel)
    ref.step()
    return ref.download()["rho"]


# ---- pool exhaustion ----

def test_waves_without_a_stream_report_no_hits(monkeypatch):
    """SPH_MASK_POOL_WORDS=20000: 64 sub-pools of 78 quads.  A wave reserves 64 Q quads from sub-pool (wave mod 64),
    first come first served, and every arrival moves the cursor: at most the FIRST wave to arrive at a sub-pool fits,
    and only if its Q is 1.  A wave without a stream reports 0 hits and 0 bodies (its rows go through the fallback
    sweep); pair_tests does not change.  Which wave arrives first is a race, so [15] and pair_hits must be ONE of the
    sums the header allows: per sub-pool either one of its Q = 1 waves, or nothing if some wave of it has Q > 1.
    (The set stays small: at most one wave of ~64 rows per sub-pool, a few thousand hits in all.)  On this state the
    answer is ONE value: every wave has a row with three non-empty runs, Q >= 2, nothing fits -- (0, 0), which
    tests/test_pair_counts_cpu.py establishes for the state and this test asserts."""
    monkeypatch.setenv("SPH_MASK_POOL_WORDS", "20000")
    sim, ref, h, cells = make("clustered")
    monkeypatch.delenv("SPH_MASK_POOL_WORDS")
    c = cpu_step(ref, None, h, cells)
    sim.simulate()
    tests, hits, bodies, _ = read(sim)
    assert tests == c["tests"]
    reach = pool_outcomes(c, 20000)
    print(f"pool exhausted: hits {hits} of {c['hits']}, bodies {bodies} of {c['bodies']}; {len(reach)} sums allowed")
    assert reach == {(0, 0)} and (hits, bodies) == (0, 0)
    # one more step: the fallback's rows moved like everyone else's, and the next step counts as exactly
    c = cpu_step(ref, c["order_out"], h, cells)
    sim.simulate()
    tests, hits, bodies, _ = read(sim)
    assert tests == c["tests"] and (hits, bodies) in pool_outcomes(c, 20000)
    sim.close()
    ref.close()


# ---- host paths ----

def test_unreset_counters_are_the_sum_over_steps():
    sim, ref, h, cells = make("nasty1")
    order, total = None, np.zeros(3, np.int64)
    for _ in range(4):
        c = cpu_step(ref, order, h, cells)
        order = c["order_out"]
        total += (c["tests"], c["hits"], c["bodies"])
        sim.simulate()
    assert read(sim, reset=False) == tuple(int(x) for x in total) + (4,)
    assert read(sim, reset=True) == tuple(int(x) for x in total) + (4,)      # reading does not consume; reset does
    assert read(sim) == (0, 0, 0, 0)
    sim.close()


def test_six_plain_steps_on_the_second_nasty_state():
    sim, ref, h, cells = make("nasty2")
    check_steps(sim, ref, h, cells, 6, what="nasty2")
    sim.close()


def test_timed_steps_with_the_grid_built_ahead(monkeypatch):
    monkeypatch.setenv("SPH_PIPELINE", "1")
    sim, ref, h, cells = make("mixture")
    t = sph.Times()
    check_steps(sim, ref, h, cells, 4, what="pipeline, timed", do_step=lambda: sim.simulateAndTime(t))
    assert t.iters == 4
    sim.close()


def test_click_reupload_and_snapshot_do_not_disturb_the_counters(tmp_path):
    """A click changes velocities only (the next step's filter sees them).  A new state -- upload, load_state,
    setup -- neither resets the counters nor adds to them: they are sums over the steps since the last reset."""
    sim, ref, h, cells = make("mixture")
    order = check_steps(sim, ref, h, cells, 1, what="before the click")
    sim.mouseClicked, sim.clickCoords = True, (400, 300)
    c = cpu_step(ref, order, h, cells)
    ref.click(400, 300)
    sim.simulate()
    assert read(sim) == (c["tests"], c["hits"], c["bodies"], 1)
    order = check_steps(sim, ref, h, cells, 2, order=c["order_out"], what="after the click")
    sim.save_state(tmp_path / "s.sphsnap")
    # not reset: one more step, then a new state, then its step -- the sum of the two
    a = cpu_step(ref, order, h, cells)
    sim.simulate()
    pos, vel, _, _ = PS.state("mixture")
    pos = pos[::-1].copy()
    sim.upload_state(pos, vel)
    ref2 = O.OracleSim(len(pos), False)
    ref2.upload(pos, vel)
    assert read(sim, reset=False) == (a["tests"], a["hits"], a["bodies"], 1)
    b = cpu_step(ref2, None, h, cells)                      # (a fresh upload: rows in id order)
    sim.simulate()
    ab = (a["tests"] + b["tests"], a["hits"] + b["hits"], a["bodies"] + b["bodies"])
    assert read(sim, reset=False) == ab + (2,)
    # the snapshot continues where it was taken, rows in the order they had: the step after it counts as it did; the
    # load itself, with a count pending, changes nothing
    sim.load_state(tmp_path / "s.sphsnap")
    assert read(sim, reset=False) == ab + (2,)
    sim.simulate()
    assert read(sim) == (ab[0] + a["tests"], ab[1] + a["hits"], ab[2] + a["bodies"], 3)
    check_steps(sim, ref, h, cells, 1, order=a["order_out"], what="after load_state")
    # setup() with a count pending: the reference's lattice start, rows in id order again
    ref3 = O.OracleSim(len(pos), False)
    ref3.upload(*PS.state("mixture")[:2])
    c1 = cpu_step(ref3, None, h, cells)
    sim.upload_state(*PS.state("mixture")[:2])
    sim.simulate()
    sim.setup()
    ref3.setup()
    assert read(sim, reset=False) == (c1["tests"], c1["hits"], c1["bodies"], 1)
    c2 = cpu_step(ref3, None, h, cells)
    sim.simulate()
    assert read(sim) == (c1["tests"] + c2["tests"], c1["hits"] + c2["hits"], c1["bodies"] + c2["bodies"], 2)
    sim.close()


# ---- slabs ----

@pytest.mark.parametrize("filt", ["0", "1"])
@pytest.mark.parametrize("name,world,steps", [("nasty_slabs", 2, 1), ("nasty_slabs", 3, 1), ("nasty_slabs", 4, 1),
                                              ("mixture", 2, 2), ("mixture", 3, 2)])
def test_slab_counters_sum_to_the_single_domain(name, world, steps, filt, monkeypatch):
    """The multi-GPU driver exposes no counters, so the slab entry points are driven through the rehearsal protocol
    (tests/slab_rehearsal.py) with SPH_FLAG_COUNT_PAIRS per slab.  Per slab and step, all three numbers are the CPU
    count over the slab's combined array: owned rows count, halo rows are candidates only and never quiet, and the
    reference velocity is drawn from the rows sph_slab_sort starts from (their ids are read from the buffer just before
    the call).  tests and hits sum over the slabs to the single domain's.
    nasty_slabs: no two rows share a velocity, so a slab's filter can drop one row's pair with itself and nothing else
    (one step: its fast rows cross several layers).  mixture: 14 z-layers cut in 2 and 3, the filter at work in every
    slab (0 < bodies < hits), second step with rows migrating between slabs."""
    monkeypatch.setenv("SPH_ZERO_PAIR_FILTER", filt)
    pos, vel, h, cells = PS.state(name)
    n = len(pos)
    settings = sph.default_settings(n, False)
    ref = O.OracleSim(n, False)
    ref.upload(pos, vel)
    p4, v4 = S.pack_state(pos, vel)
    bounds, parts = S.split_initial(p4, v4, settings.h, 100, world)
    slabs, started_from = [], {}
    for r, ((zlo, zhi), (pp, vv)) in enumerate(zip(bounds, parts)):
        sl = S.Slab(S.HipSlabBackend(settings, n, device=0, flags=COUNT), r, world, zlo, zhi, 100)
        sl.load(torch.from_numpy(pp).cuda(), torch.from_numpy(vv).cuda())

        def sort(src_buf, offset, count_, thresholds, b=sl.b, r=r, inner=sl.b.sort):
            rows = b.pos[src_buf][offset:offset + count_, 3].cpu().numpy()
            started_from[r] = rows.view(np.uint32).astype(np.int64)      # ids, in the order the sort starts from
            return inner(src_buf, offset, count_, thresholds)
        sl.b.sort = sort
        slabs.append(sl)
    for step in range(1, steps + 1):
        before = ref.download()
        ref.step()
        rho = ref.download()["rho"]
        S.run_loopback(slabs, 1)
        single = count(before["pos"])
        layer = S.layer_of(before["pos"][:, 2], settings.h, 100)
        got = np.zeros(2, np.int64)
        for r, (sl, (zlo, zhi)) in enumerate(zip(slabs, bounds)):
            dbg = (C.c_uint64 * 16)()
            sl.b._check(sl.b._L.sph_debug_counters(sl.b._h, dbg), "sph_debug_counters")
            kt = sl.b.kernel_times(reset=True)
            ids = started_from[r]
            own = (layer[ids] >= zlo) & (layer[ids] < zhi)
            assert own.sum() == ((layer >= zlo) & (layer < zhi)).sum() and len(np.unique(ids)) == len(ids)
            c = count(before["pos"][ids], before["vel"][ids], rho[ids], zero_pair_filter=filt == "1", owned=own)
            want = (c["tests"], c["hits"], c["bodies"])
            print(f"{name} x{world} step {step} slab [{zlo}, {zhi}): {(kt.pair_tests, int(dbg[15]), kt.pair_hits)}, CPU {want}")
            assert (kt.pair_tests, int(dbg[15]), kt.pair_hits) == want and dbg[14] == kt.pair_hits and dbg[0] == kt.pair_tests
            if name == "mixture":
                assert (0 < c["bodies"] < c["hits"]) if filt == "1" else c["bodies"] == c["hits"]
            elif filt == "1":   # distinct velocities: the tie goes to the first sampled row, which is quiet if it is owned and dry
                assert c["bodies"] == c["hits"] - int(own[0] and rho[ids[0]] <= 1000)
            got += (kt.pair_tests, int(dbg[15]))
        assert tuple(got) == (single["tests"], single["hits"])
    for sl in slabs:
        sl.b.close()
