"""Pins tests/step_f64.py, the float64 reference that test_gpu_fast_math.py holds SPH_MATH_FAST to:
hand-derived answers first, then the two strict-fp32 implementations the project already trusts (the C
oracle and restated_step of test_oracle_independent_restatement.py) measured against it.  No GPU.

The fp32 implementations must stay under the project's stated tolerance (1e-5, BASELINE.json's north
star) in every measure; the printed maxima and means are the yardstick for the fast-math bound.
Measured (max / mean; oracle and restatement are bit-identical, so one line each):

   block: e_rho 9.870e-07 / 2.129e-07  e_F 3.948e-07 / 7.633e-08  e_pos 5.967e-08 / 4.137e-08  e_vel 9.719e-08 / 3.082e-08
   cloud: e_rho 5.621e-07 / 1.236e-07  e_F 7.081e-07 / 6.696e-08  e_pos 5.880e-08 / 3.091e-08  e_vel 7.943e-08 / 2.396e-08
 evolved: e_rho 9.450e-07 / 2.133e-07  e_F 9.066e-07 / 1.061e-07  e_pos 5.949e-08 / 3.798e-08  e_vel 1.031e-07 / 3.371e-08
"""
import math

import numpy as np
import pytest

import step_f64 as S
from helpers import assert_bit_equal
from oracle import oracle as O
from test_oracle_independent_restatement import restated_step

TOL = 1e-5   # BASELINE.json: the north star's relative tolerance


# ---- hand-derived answers ----

H, DT, BOX = 0.1, 0.01, 10.0
DC = 315.0 / (64.0 * math.pi * H ** 9)
VC = 45.0 / (math.pi * H ** 6)
KW = dict(h=H, dcoef=DC, vcoef=VC, dt=DT, box=BOX)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_two_particles_closed_formulas():
    """Two particles 0.05 apart, densities 1500 and 900 given, velocities given: every quantity from the
    closed formulas of simulator.cu:84-130, :223-249 and :269-276 written out as scalars."""
    r = 0.05
    u = np.array([2.0, -1.0, 2.0]) / 3.0                 # unit vector
    p0 = np.array([5.0, 5.0, 5.0])
    pos = np.stack([p0, p0 + r * u])
    vel = np.array([[0.5, -0.25, 1.0], [-1.5, 0.75, 0.25]])
    rho = np.array([1500.0, 900.0])

    # density: the particle itself (dist = 0) and its neighbour
    w_self, w_pair = DC * (H * H) ** 3, DC * (H * H - r * r) ** 3
    got_rho, Sd = S.density64(pos, **KW)
    assert rel(got_rho, [S.MASS * (w_self + w_pair)] * 2) < 1e-12 and rel(Sd, got_rho) < 1e-12

    # forces: p_0 = 500, p_1 = 0
    F, Sf = S.force64(pos, vel, rho, **KW)
    scale = -VC * (H - r) ** 2 / r
    lap = VC * (H - r)
    want = np.zeros((2, 3))
    want_s = np.zeros(2)
    for i, j in ((0, 1), (1, 0)):
        d = pos[i] - pos[j]
        tp = d * scale * (-S.MASS * (500.0 + 0.0) / (2.0 * rho[j]))
        tv = (vel[j] - vel[i]) * (1.0 * S.MASS * lap / rho[j])
        want[i] = tp + tv
        want_s[i] = math.sqrt(tp @ tp) + math.sqrt(tv @ tv)
    assert rel(F, want) < 1e-12 and rel(Sf, want_s) < 1e-12
    # the pressure term pushes the two apart along u, with magnitude MASS 500 / (2 rho_j) * vcoef (h-r)^2
    tp0 = F[0] - (vel[1] - vel[0]) * (S.MASS * lap / rho[1])
    assert rel(tp0, -u * S.MASS * 500.0 / (2.0 * 900.0) * VC * (H - r) ** 2) < 1e-12
    j, dist, tp, tv = S.force64_pairs(pos, vel, rho, 0, **KW)
    assert list(j) == [1] and rel(dist, [r]) < 1e-12 and rel(tp[0], tp0) < 1e-12

    # integration, nowhere near a wall
    p, v, fragile = S.integrate64(pos, vel, F, rho, **KW)
    wv = vel + DT * (want / rho[:, None] + np.array([0.0, S.GRAVITY, 0.0]))
    assert rel(v, wv) < 1e-12 and rel(p, pos + DT * wv) < 1e-12 and not fragile.any()


def test_a_particle_alone():
    """The reference's density loop visits the particle itself (dist2 = 0 <= h^2, simulator.cu:178-182), so a
    particle alone holds its own term MASS dcoef h^6, not EPS_F; the clamp at EPS_F is reached only when that
    term is below it (a vanishing coefficient here).  No force in either case."""
    pos = np.array([[3.0, 4.0, 5.0]])
    rho, Sd = S.density64(pos, **KW)
    assert rel(rho, [S.MASS * DC * H ** 6]) < 1e-12 and rel(Sd, rho) < 1e-12
    rho0, Sd0 = S.density64(pos, h=H, dcoef=0.0)
    assert rho0[0] == S.EPS_F and Sd0[0] == 0.0
    F, Sf = S.force64(pos, np.ones((1, 3)), rho, **KW)
    assert not F.any() and Sf[0] == 0.0
    # the error measures leave such rows out of the ratios and demand the exact values
    assert S.e_rho(np.array([1e-4], np.float32), rho0, Sd0).size == 0
    assert S.e_F(np.zeros((1, 3), np.float32), F, Sf).size == 0
    with pytest.raises(AssertionError):
        S.e_rho(np.array([2e-4], np.float32), rho0, Sd0)
    with pytest.raises(AssertionError):
        S.e_F(np.full((1, 3), 1e-30, np.float32), F, Sf)


def test_coincident_and_sub_eps_pairs_are_gated():
    pos = np.array([[5.0, 5.0, 5.0], [5.0, 5.0, 5.0], [5.0, 5.0 + 0.5 * S.EPS_F, 5.0]])
    vel = np.array([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    rho, _ = S.density64(pos, **KW)
    assert rel(rho[:2], [S.MASS * DC * (2 * H ** 6 + (H * H - (0.5 * S.EPS_F) ** 2) ** 3)] * 2) < 1e-12
    F, Sf = S.force64(pos, vel, np.full(3, 2000.0), **KW)
    assert not F.any() and not Sf.any()


def test_pair_at_exactly_h_is_included_and_contributes_nothing():
    h = 0.125                                            # (exact in binary, and so is 5 + h)
    kw = dict(h=h, dcoef=315.0 / (64.0 * math.pi * h ** 9), vcoef=45.0 / (math.pi * h ** 6))
    pos = np.array([[5.0, 5.0, 5.0], [5.0 + h, 5.0, 5.0]])
    assert pos[1, 0] - pos[0, 0] == h, "the pair must sit exactly on the radius"
    vel = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    rho, Sd = S.density64(pos, **kw)
    assert rel(rho, [S.MASS * kw["dcoef"] * h ** 6] * 2) < 1e-12
    F, Sf = S.force64(pos, vel, np.full(2, 2000.0), **kw)
    assert not F.any() and not Sf.any()
    j, dist, tp, tv = S.force64_pairs(pos, vel, np.full(2, 2000.0), 0, **kw)
    assert len(j) == 0
    # ... just inside it contributes, just outside it is not there at all
    for x, inside in ((5.0 + 0.999 * h, True), (5.0 + 1.001 * h, False)):
        pos[1, 0] = x
        F, Sf = S.force64(pos, vel, np.full(2, 2000.0), **kw)
        assert (F[0, 0] < 0 and F[1, 0] > 0 and Sf.all()) if inside else (not F.any() and not Sf.any())
        assert (S.density64(pos, **kw)[1] > Sd).all() == inside


def test_walls_dead_zone_and_fragile_mask():
    """Clamp on either side, the bounce, the velocity dead zone, and the mask around each discontinuity."""
    hi = float(np.float32(BOX) - np.float32(S.H))
    kw = dict(h=S.H, dt=DT, box=BOX)
    pos = np.array([[S.H + 0.001, 5.0, hi - 0.001],     # x hits the low wall, z the high one
                    [5.0, 5.0, 5.0],                    # y velocity ends inside the dead zone
                    [S.H + 0.01 + 5e-6, 5.0, 5.0],      # lands 5e-6 from the low plane: fragile
                    [5.0, 5.0, 5.0]])                   # x velocity 5e-7 from the dead zone: fragile
    vel = np.array([[-1.0, 0.0, 2.0], [0.0, -S.GRAVITY * DT + 5e-5, 0.0], [-1.0, 0.0, 0.0],
                    [S.EPS_F + 5e-7, 0.0, 0.0]])
    p, v, fragile = S.integrate64(pos, vel, np.zeros((4, 3)), np.ones(4), **kw)
    assert p[0, 0] == S.H and p[0, 2] == hi and v[0, 0] == 0.5 and v[0, 2] == -1.0
    assert v[1, 1] == 0.0 and abs(p[1, 1] - (5.0 + DT * 5e-5)) < 1e-15
    assert list(fragile) == [False, False, True, True]


# ---- the strict fp32 implementations against float64 ----

@pytest.fixture(scope="module")
def inputs():
    out = {"block": S.build_block(), "cloud": S.build_cloud()}
    pos, vel, moved = S.build_evolved()
    print(f"evolved: {moved} of {len(pos)} particles moved off the EPS_F gate")
    out["evolved"] = (pos, vel)
    return out


def oracle_one_step(pos, vel):
    sim = O.OracleSim(len(pos), False)
    sim.upload(pos, vel)
    sim.step()
    d = sim.download(want_force=True)
    sim.close()
    return d


@pytest.mark.parametrize("name", ["block", "cloud", "evolved"])
def test_strict_fp32_step_against_float64(inputs, name):
    pos, vel = inputs[name]
    d = oracle_one_step(pos, vel)
    p, v, rho, force = restated_step(pos, vel)
    for k, a in (("rho", rho), ("force", force), ("vel", v), ("pos", p)):
        assert_bit_equal(d[k], a, f"{name}: oracle vs restatement, {k}")
    for who, (rx, fx, px, vx) in (("oracle", (d["rho"], d["force"], d["pos"], d["vel"])),
                                  ("restated", (rho, force, p, v))):
        m = S.measure_step(pos, vel, rx, fx, px, vx)
        s = S.summary(m)
        print(S.format_summary(name, s), f" fragile {m['fragile']:.4f}  ({who})")
        assert m["fragile"] <= 0.01
        for k in S.MEASURES:
            assert s[k][0] <= TOL, f"{name} ({who}): max e_{k} = {s[k][0]:.3e} exceeds {TOL}"
    # (the cloud is a viscosity-and-edges state: 2,000 particles in its floor layer reach rho ~ 550)
    assert name == "cloud" or (d["rho"] > 1000).sum() > 100, "pressure must be on"
    assert np.abs(d["force"]).max() > 0
