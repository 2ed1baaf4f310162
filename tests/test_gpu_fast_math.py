"""SPH_MATH_FAST (Simulator(math="fast"), MultiGpuSimulator(math="fast")) on every kernel path, one kernel at
a time against the float64 reference of tests/step_f64.py.

A tolerance mode cannot be held to the oracle bit for bit, and "close to the oracle after many steps" would
not notice a wrong coefficient.  So for ONE step of an uploaded state each case takes the pre-step state, that
step's rho and that step's force (SPH_FLAG_STORE_FORCE) from the handle and measures
  * e_rho  of the fast densities against density64(pos),
  * e_F    of the fast forces against force64(pos, vel, rho_fast)  (the code's own densities: an error in rho
           does not leak in through max(0, rho - 1000)),
  * e_pos, e_vel of the post-step state against integrate64(pos, vel, F_fast, rho_fast) outside its `fragile`
           mask (<= 1 % of the particles),
each relative to the sum of the magnitudes of the terms (step_f64.e_rho / e_F / e_integrate).

THE BOUND IS NOT A LITERAL.  The strict oracle runs the same input on the CPU and goes through the same
measures; for the maximum and for the mean of every measure, e(fast) <= FACTOR * e(oracle) with FACTOR = 4
(8 * 2^-24 where the oracle's error is exactly 0).  Why 4: the fast body replaces two correctly rounded
operations (divide, square root) by ~1-ulp approximations and regroups the coefficient product, so a term can
carry a few times the strict body's rounding error; the accumulation over ~100 neighbours, which dominates,
is the same.  A coefficient off by 1e-3 is three orders of magnitude above this bound.

Bit-for-bit identities hold in fast mode too wherever the kernels and the neighbour order are the same
(slabs == single domain, tiny mask pool == default pool, zero-pair filter off == on, run == rerun, re-upload
and snapshot resume == fresh handle) and are asserted as such.  list == lds is NOT one of them.

Measured on an MI355X (max / mean; `fast` first, the oracle's in brackets):
                 e_rho                  e_F                    e_pos                  e_vel
  block    list  1.081e-06 / 2.112e-07  4.088e-07 / 7.684e-08  5.966e-08 / 4.137e-08  1.041e-07 / 3.104e-08
           lds   (the same figures as list to every digit shown, in every state)
        (oracle) 9.870e-07 / 2.129e-07  3.948e-07 / 7.633e-08  5.967e-08 / 4.137e-08  9.719e-08 / 3.082e-08
  cloud    list  5.441e-07 / 1.520e-07  6.504e-07 / 6.702e-08  5.880e-08 / 3.090e-08  9.859e-08 / 2.405e-08
   (pool exhausted: the same bits as list)
        (oracle) 5.621e-07 / 1.236e-07  7.081e-07 / 6.696e-08  5.880e-08 / 3.091e-08  7.943e-08 / 2.396e-08
  evolved  list  1.033e-06 / 2.106e-07  8.962e-07 / 1.062e-07  5.949e-08 / 3.798e-08  9.219e-08 / 3.419e-08
        (oracle) 9.450e-07 / 2.133e-07  9.066e-07 / 1.061e-07  5.949e-08 / 3.798e-08  1.031e-07 / 3.371e-08
  h025     list  1.696e-07 / 5.464e-08  4.100e-05 / 2.818e-07  5.815e-08 / 3.206e-08  9.693e-08 / 2.671e-08
        (oracle) 1.818e-07 / 5.267e-08  4.094e-05 / 2.940e-07  5.815e-08 / 3.206e-08  1.143e-07 / 2.652e-08
(h025's max e_F belongs to a row whose only neighbour sits on the rim of the support: h - dist cancels, in the
strict body too.)  Before force_pair_fast refined dist with a Newton step (sweep_common.h) the same cases gave max
e_F 2.124e-06 on cloud (3.0 x the oracle's) and 1.901e-04 / mean 6.749e-07 on h025 (4.6 x: over the bound).
With 0.5f * SPH_MASS in force_pair_fast changed to 0.5005f the list cases fail on e_F alone (block 3.264e-04 /
1.211e-04, evolved 5.931e-04 / 2.499e-04; e_rho unchanged); with the FAST density constant scaled by 1.001 all
four fail on e_rho (1.001e-03 / 1.000e-03).
"""
import ctypes as C

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
import step_f64 as S
from cudafluidsimulator_amd import _lib
from cudafluidsimulator_amd import mgpu as M
from helpers import assert_bit_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 8.0 * 2.0 ** -24
FLAGS = _lib.SPH_FLAG_STORE_FORCE


def settings_for(name, n):
    return S.h025_settings(sph.default_settings) if name == "h025" else sph.default_settings(n, False)


class States:
    """Inputs, their float64 densities and the oracle's errors: each computed once, never modified."""

    def __init__(self):
        self._inputs, self._rho64, self._oracle = {}, {}, {}

    def inputs(self, name):
        if name not in self._inputs:
            out = {"block": S.build_block, "cloud": S.build_cloud, "evolved": S.build_evolved,
                   "h025": S.build_h025}[name]()
            pos, vel = out[0], out[1]
            pos.setflags(write=False)
            vel.setflags(write=False)
            self._inputs[name] = (pos, vel)
        return self._inputs[name]

    def rho64(self, name):
        if name not in self._rho64:
            pos, _ = self.inputs(name)
            self._rho64[name] = S.density64(pos, **S.settings_args(settings_for(name, len(pos))))
        return self._rho64[name]

    def oracle(self, name):
        """the strict oracle's one step of this input through the same measures"""
        if name not in self._oracle:
            pos, vel = self.inputs(name)
            s = settings_for(name, len(pos))
            ref = O.OracleSim(len(pos), False)
            if name == "h025":   # (as test_non_default_settings does)
                C.memmove(C.byref(ref.settings), C.byref(s), C.sizeof(s))
                ref.close()
                ref._h = O.lib().oracle_sim_create(C.byref(ref.settings))
            ref.upload(pos, vel)
            ref.step()
            d = ref.download(want_force=True)
            ref.close()
            self._oracle[name] = S.summary(measure(self, name, d["rho"], d["force"], d["pos"], d["vel"]))
        return self._oracle[name]


def measure(states, name, rho_x, F_x, pos_x, vel_x):
    pos, vel = states.inputs(name)
    kw = S.settings_args(settings_for(name, len(pos)))
    rho64, Sd = states.rho64(name)
    F64, Sf = S.force64(pos, vel, rho_x, **kw)
    ep, ev, frag = S.e_integrate(pos_x, vel_x, pos, vel, F_x, rho_x, **kw)
    return {"rho": S.e_rho(rho_x, rho64, Sd), "F": S.e_F(F_x, F64, Sf), "pos": ep, "vel": ev, "fragile": frag}


@pytest.fixture(scope="module")
def states():
    return States()


def fast_step(name, pos, vel, sweep, flags=FLAGS):
    """One fast step of an uploaded state: what the handle held before it, and that step's rho, force, pos, vel."""
    sim = sph.Simulator(settings_for(name, len(pos)), sweep=sweep, flags=flags, math="fast")
    sim.upload_state(pos, vel)
    pre = sim.download_state()
    assert_bit_equal(pre["pos"], pos, "pre-step pos")
    assert_bit_equal(pre["vel"], vel, "pre-step vel")
    sim.simulate()
    st = sim.download_state()
    st["force"] = sim.download_force()
    st["counters"] = sim.debug_counters()
    sim.close()
    return st


def check_against_float64(states, name, what, st):
    pos, _ = states.inputs(name)
    s = settings_for(name, len(pos))
    h, hi = np.float32(s.h), np.float32(s.boxDim) - np.float32(s.h)
    for k in ("pos", "vel", "rho", "force"):
        assert np.isfinite(st[k]).all(), f"{what}: {k} not finite"
    assert (st["pos"] >= h).all() and (st["pos"] <= hi).all(), f"{what}: a position outside [h, boxDim - h]"
    m = measure(states, name, st["rho"], st["force"], st["pos"], st["vel"])
    fast, ref = S.summary(m), states.oracle(name)
    print(S.format_summary(what, fast), f" fragile {m['fragile']:.4f}")
    print(S.format_summary("(oracle)", ref))
    assert m["fragile"] <= 0.01
    bad = []
    for k in S.MEASURES:
        for stat, f, r in zip(("max", "mean"), fast[k], ref[k]):
            bound = FACTOR * r if r > 0 else FLOOR
            if not f <= bound:
                bad.append(f"{stat} e_{k}: fast {f:.3e} > {FACTOR:g} x oracle {r:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)


# list: k_density_mask_lds<true,true> + k_force_dealt<true,true>;  lds: k_density_lds<true> + k_force_lds<true,.>;
# h025 (cut2 != h2, non-reference coefficients): k_density_mask_lds<true,false>
@pytest.mark.parametrize("name,sweep", [("block", "list"), ("cloud", "list"), ("evolved", "list"),
                                        ("block", "lds"), ("cloud", "lds"), ("h025", "list"), ("h025", "lds")])
def test_fast_step_against_float64(states, name, sweep):
    pos, vel = states.inputs(name)
    st = fast_step(name, pos, vel, sweep)
    check_against_float64(states, name, f"{name}/{sweep}", st)
    if name in ("block", "evolved"):
        assert (st["rho"] > 1000).sum() > 100, "pressure must be on"
    if name == "h025":   # the force cut-off (largest dist2 with sqrtf(dist2) <= h) lies above h*h: SAMECUT is false
        h = np.float32(settings_for(name, len(pos)).h)
        assert np.sqrt(np.nextafter(h * h, np.float32(1))) <= h


def test_fast_with_an_exhausted_mask_pool(states, monkeypatch):
    """SPH_MASK_POOL_WORDS=4096 is 1,024 quads, 16 per sub-pool; a wave needs at least 64 (one per lane), so
    EVERY wave finds its sub-pool exhausted and k_force_fallback<true,true> computes every row: no hit is
    recorded through a mask (debug counter 15, SPH_FLAG_COUNT_PAIRS), where the default pool records them all.
    Same float64 bounds, and the same bits as the default pool."""
    pos, vel = states.inputs("cloud")
    flags = FLAGS | _lib.SPH_FLAG_COUNT_PAIRS
    monkeypatch.setenv("SPH_MASK_POOL_WORDS", "4096")
    tiny = fast_step("cloud", pos, vel, "list", flags)
    monkeypatch.delenv("SPH_MASK_POOL_WORDS")
    full = fast_step("cloud", pos, vel, "list", flags)
    assert tiny["counters"][15] == 0 and full["counters"][15] > len(pos), "the tiny pool must send every wave to the fallback"
    assert tiny["counters"][0] == full["counters"][0] > 0, "same candidates tested"
    check_against_float64(states, "cloud", "cloud/list, mask pool exhausted", tiny)
    for k in ("pos", "vel", "rho", "force"):
        assert_bit_equal(tiny[k], full[k], f"tiny pool vs default pool: {k}")


def run_steps(sim, steps):
    for _ in range(steps):
        sim.simulate()
    return sim.download_state()


@pytest.mark.parametrize("world", [2, 3])
def test_fast_slabs_equal_the_fast_single_domain(states, world):
    """The slab entry points (sph_slab_density / sph_slab_force_ranges / the halo patch) with math_mode fast:
    the same kernels on the same neighbour order as the single domain, which the cases above hold to float64 --
    so the same bits, after each of three steps."""
    pos, vel = states.inputs("cloud")
    s = sph.default_settings(len(pos), False)
    sim = sph.Simulator(s, math="fast")
    sim.upload_state(pos, vel)
    mg = M.MultiGpuSimulator(s, world=world, transport="loopback", math="fast")
    mg.upload_state(pos, vel)
    strict = sph.Simulator(s)
    strict.upload_state(pos, vel)
    for step in (1, 2, 3):
        sim.simulate()
        mg.simulate()
        strict.simulate()
        want, got = sim.download_state(), mg.download_state()
        assert got["written"] == len(pos)
        for k in ("pos", "vel", "rho"):
            assert np.isfinite(got[k]).all()
            assert_bit_equal(got[k], want[k], f"{world} slabs, step {step}: {k}")
        assert_bit_equal(np.array(mg.getPosition()), want["pos"], f"{world} slabs, step {step}: getPosition()")
    # (the slabs really ran the fast kernels: strict mode gives other bits on this state)
    assert (strict.download_state()["rho"].view(np.uint32) != want["rho"].view(np.uint32)).any()
    assert sum(mg.stats().owned[:world]) == len(pos) and min(mg.stats().owned[:world]) > 0
    sim.close(); mg.close(); strict.close()


def test_fast_zero_pair_filter_on_equals_off(monkeypatch):
    """A dropped pair would have added fma(d, 0, F) = F: SPH_ZERO_PAIR_FILTER=0 and 1 give the same bits in
    fast mode too, and the counters show that the filter dropped pairs (co_moving_mixture cut to 4,000
    particles: its co-moving block -- without the other 36,000 particles below the rest density, so its
    mutual pairs are all dropped -- and a sparse cloud in which one row in twelve has a velocity of its own,
    whose pairs must be kept)."""
    from test_gpu_parity import co_moving_mixture
    pos, vel = co_moving_mixture(3)
    pos, vel = pos[:4000].copy(), vel[:4000].copy()
    s = sph.default_settings(len(pos), False)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SPH_ZERO_PAIR_FILTER", mode)
        sim = sph.Simulator(s, flags=_lib.SPH_FLAG_COUNT_PAIRS, math="fast")
        sim.upload_state(pos, vel)
        st = run_steps(sim, 3)
        out[mode] = (st, sim.kernel_times().pair_hits, sim.debug_counters()[15])
        sim.close()
    for k in ("pos", "vel", "rho"):
        assert_bit_equal(out["1"][0][k], out["0"][0][k], f"filter on vs off: {k}")
    assert out["0"][1] == out["0"][2] == out["1"][2], "hits recorded do not depend on the filter"
    assert 0 < out["1"][1] < out["0"][1], "the filter dropped pairs and kept some"


def test_fast_handle_reruns_reuploads_and_resumes_with_the_same_bits(states, tmp_path):
    """Two runs of one configuration are bit-identical; so is a handle that stepped another state before
    this one was uploaded, and one that continues from a snapshot."""
    pos, vel = states.inputs("block")
    other_pos, other_vel = states.inputs("cloud")
    s = sph.default_settings(len(pos), False)

    def fresh():
        sim = sph.Simulator(s, math="fast")
        sim.upload_state(pos, vel)
        return sim

    a = fresh()
    want = run_steps(a, 3)
    b = fresh()
    again = run_steps(b, 1)
    snap = tmp_path / "fast.sphsnap"
    b.save_state(snap)
    again = run_steps(b, 2)
    # a handle that has run something else first (same particle count, other state)
    c = sph.Simulator(s, math="fast")
    c.upload_state(other_pos[:len(pos)], other_vel[:len(pos)])
    run_steps(c, 2)
    c.upload_state(pos, vel)
    reup = run_steps(c, 3)
    # ... and is then sent back to step 1 by the snapshot
    c.load_state(snap)
    resumed = run_steps(c, 2)
    for k in ("pos", "vel", "rho"):
        assert_bit_equal(again[k], want[k], f"rerun: {k}")
        assert_bit_equal(reup[k], want[k], f"after a re-upload: {k}")
        assert_bit_equal(resumed[k], want[k], f"resumed from a snapshot: {k}")
    assert (want["rho"] > 1000).sum() > 100
    a.close(); b.close(); c.close()


def test_fast_needs_a_sweep_that_has_it():
    with pytest.raises(sph.SphError, match="SPH_MATH_FAST"):
        sph.Simulator(sph.default_settings(100, True), sweep="direct", math="fast")
