"""One step of the reference's update (simulator.cu:84-130, :149-318) in float64, one kernel
at a time, for the tolerance mode (SPH_MATH_FAST) that cannot be held to the oracle bit for bit.

Plain numpy, float64 throughout, brute force over ALL pairs in row chunks: no neighbour grid,
no cell table, no summation order -- nothing shared with the HIP kernels, the C oracle or
test_oracle_independent_restatement.py.  n <= 4096 keeps a sweep to a second or two.

Three functions, one per kernel; a test compares ONE kernel's output with that kernel's own
inputs (force64 takes the densities the code under test produced, integrate64 its forces):

  density64(pos)               -> rho, Sd          Sd[i] = sum_j |term_ij| (= the unclamped sum)
  force64(pos, vel, rho)       -> F, Sf            Sf[i] = sum_j (|pressure term_ij| + |viscosity term_ij|)
  integrate64(pos, vel, F, rho)-> pos, vel, fragile

The settings a kernel reads (h, the two kernel coefficients, timestep, boxDim) are arguments;
`settings_args(s)` takes them from a Settings struct.  They are the fp32 values the code under
test was given, widened -- and so is the upper wall plane, which the reference computes as the
fp32 difference boxDim - h (simulator.cu:283).  Everything derived from them (h^2, h - r, ...) is
float64.
"""
import numpy as np

from helpers import clustered_state, dense_block

F32 = np.float32
# simulator.h:6-12 / simulator.cu:13-14, the fp32 constants widened
MASS = float(F32(0.02))
GAS_CONSTANT = 1.0
REST_DENSITY = 1000.0
VISCOSITY = 1.0
GRAVITY = float(F32(-9.8))
ELASTICITY = 0.5
EPS_F = float(F32(1e-4))
# main.cpp:57-63
H = float(F32(0.1))
_PI = F32(3.14159265)
V_COEFF = float(F32(45.0) / (_PI * F32(float(F32(0.1)) ** 6)))
D_COEFF = float(F32(315.0) / (F32(64.0) * _PI * F32(float(F32(0.1)) ** 9)))
DT = float(F32(0.01))
BOX = float(F32(10.0))

CHUNK = 256          # rows per block of the all-pairs sweeps
WALL_BAND = 1e-5     # integrate64: "fragile" distance from a wall plane
DEAD_BAND = 1e-6     # ... and from the +-EPS_F velocity dead zone
NEAR_GATE = 1e-3     # builders: no pair with 0 < dist < NEAR_GATE


def settings_args(s):
    """The keyword arguments of the three kernels from a Settings struct (library or oracle)."""
    return dict(h=float(F32(s.h)), dcoef=float(F32(s.d_kernel_coeff)), vcoef=float(F32(s.v_kernel_coeff)),
                dt=float(F32(s.timestep)), box=float(F32(s.boxDim)))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _pair_blocks(pos):
    """(i0, i1, d, dist2) over row blocks: d[a, j] = pos[i0 + a] - pos[j]"""
    n = len(pos)
    for i0 in range(0, n, CHUNK):
        i1 = min(i0 + CHUNK, n)
        d = pos[i0:i1, None, :] - pos[None, :, :]
        yield i0, i1, d, np.einsum("ijk,ijk->ij", d, d)


def density64(pos, h=H, dcoef=D_COEFF, **_):
    """densityKernel (simulator.cu:84-97) summed as at :162-186: every particle with dist2 <= h^2
    counts, the particle itself included.  Returns rho (clamped at EPS_F) and Sd."""
    pos = _f64(pos)
    h2 = h * h
    Sd = np.zeros(len(pos))
    for i0, i1, _d, dist2 in _pair_blocks(pos):
        diff = np.where(dist2 <= h2, h2 - dist2, 0.0)
        Sd[i0:i1] = (MASS * (dcoef * diff * diff * diff)).sum(axis=1)
    return np.maximum(Sd, EPS_F), Sd


def _force_terms(d, dist2, dv, rho_i, rho_j, h, vcoef):
    """pressure and viscosity terms of pairs: d = p_i - p_j, dv = v_j - v_i, any broadcastable shapes
    with a trailing axis of 3 on d / dv (simulator.cu:99-130, :223-249)"""
    prs_i = np.maximum(0.0, GAS_CONSTANT * (rho_i - REST_DENSITY))
    prs_j = np.maximum(0.0, GAS_CONSTANT * (rho_j - REST_DENSITY))
    dist = np.sqrt(dist2)
    tiny = dist < EPS_F
    safe = np.where(tiny, 1.0, dist)
    hd = h - dist
    in_p = (dist2 <= h * h) & ~tiny
    in_v = (dist <= h) & ~tiny
    f_pressure = -MASS * (prs_i + prs_j) / (2.0 * rho_j)
    scale = np.where(in_p, (-vcoef) * hd * hd / safe, 0.0)
    f_visc = np.where(in_v, VISCOSITY * MASS * (vcoef * hd) / rho_j, 0.0)
    return d * (scale * f_pressure)[..., None], dv * f_visc[..., None]


def force64(pos, vel, rho, h=H, vcoef=V_COEFF, **_):
    """kernelUpdateForces (simulator.cu:192-256) with `rho` GIVEN: pressures are max(0, rho - 1000) of
    exactly these densities, so an error in rho does not reach the comparison through that
    cancellation.  Gates as in the reference: pressure on dist2 <= h^2, viscosity on dist <= h, both
    off for dist < EPS_F.  Returns F (n, 3) and Sf."""
    pos, vel, rho = _f64(pos), _f64(vel), _f64(rho)
    n = len(pos)
    Fo, Sf = np.zeros((n, 3)), np.zeros(n)
    for i0, i1, d, dist2 in _pair_blocks(pos):
        dv = vel[None, :, :] - vel[i0:i1, None, :]
        tp, tv = _force_terms(d, dist2, dv, rho[i0:i1, None], rho[None, :], h, vcoef)
        Fo[i0:i1] = tp.sum(axis=1) + tv.sum(axis=1)
        Sf[i0:i1] = np.sqrt((tp * tp).sum(axis=2)).sum(axis=1) + np.sqrt((tv * tv).sum(axis=2)).sum(axis=1)
    return Fo, Sf


def force64_pairs(pos, vel, rho, i, h=H, vcoef=V_COEFF, **_):
    """Row i of force64 pair by pair, to locate a wrong term: (j, dist, pressure term, viscosity term) of
    every j that contributes."""
    pos, vel, rho = _f64(pos), _f64(vel), _f64(rho)
    d = pos[i] - pos
    dist2 = (d * d).sum(axis=1)
    tp, tv = _force_terms(d, dist2, vel - vel[i], rho[i], rho, h, vcoef)
    j = np.nonzero(tp.any(axis=1) | tv.any(axis=1))[0]
    return j, np.sqrt(dist2[j]), tp[j], tv[j]


def integrate64(pos, vel, Fo, rho, h=H, dt=DT, box=BOX, **_):
    """kernelUpdatePositions (simulator.cu:258-318).  Returns new pos, vel and `fragile`: particles whose
    pre-clamp coordinate lies within WALL_BAND of a wall plane, or one of whose velocity components lies
    within DEAD_BAND of the +-EPS_F dead zone -- the clamp and the zeroing are discontinuities that an
    fp32 and an fp64 evaluation may take differently."""
    pos, vel, Fo, rho = _f64(pos), _f64(vel), _f64(Fo), _f64(rho)
    hi = float(F32(box) - F32(h))
    v = vel.copy()
    v[:, 0] += dt * Fo[:, 0] / rho
    v[:, 1] += dt * (Fo[:, 1] / rho + GRAVITY)
    v[:, 2] += dt * Fo[:, 2] / rho
    p = pos + dt * v
    fragile = ((np.abs(p - h) < WALL_BAND) | (np.abs(p - hi) < WALL_BAND)).any(axis=1)
    low = p < h
    high = ~low & (p > hi)
    p = np.where(low, h, np.where(high, hi, p))
    v = np.where(low | high, v * -ELASTICITY, v)
    fragile |= (np.abs(np.abs(v) - EPS_F) < DEAD_BAND).any(axis=1)
    v = np.where(np.abs(v) < EPS_F, 0.0, v)
    return p, v, fragile


# ---- error measures: every test uses these ----

def e_rho(rho_x, rho64, Sd):
    """|rho_x - rho64| / Sd over the rows with Sd > 0; a row with Sd == 0 must carry exactly EPS_F."""
    rho_x = np.asarray(rho_x)
    assert rho_x.shape == rho64.shape and np.isfinite(rho_x).all()
    live = Sd > 0
    assert (rho_x[~live] == F32(1e-4)).all(), "a row without any density term must hold exactly EPS_F"
    return np.abs(rho_x[live].astype(np.float64) - rho64[live]) / Sd[live]


def e_F(F_x, F64, Sf):
    """max_a |F_x[i, a] - F64[i, a]| / Sf[i] over the rows with Sf > 0; a row with Sf == 0 must be exactly 0."""
    F_x = np.asarray(F_x)
    assert F_x.shape == F64.shape and np.isfinite(F_x).all()
    live = Sf > 0
    assert (F_x[~live] == 0).all(), "a row without any force term must hold exactly 0"
    return np.abs(F_x[live].astype(np.float64) - F64[live]).max(axis=1) / Sf[live]


def e_integrate(pos_x, vel_x, pos, vel, Fo, rho, h=H, dt=DT, box=BOX, **_):
    """The integration's error against integrate64 on the SAME inputs, each coordinate over the sum of the
    magnitudes of the terms it is made of:
      e_vel = |v_x - v64| / (|v| + dt (|F| / rho + |g|)),   e_pos = |p_x - p64| / (|p| + dt |v64|)
    per particle the maximum over the three axes, outside `fragile`.  Returns e_pos, e_vel and the fragile
    fraction."""
    pos, vel, Fo, rho = _f64(pos), _f64(vel), _f64(Fo), _f64(rho)
    p64, v64, fragile = integrate64(pos, vel, Fo, rho, h=h, dt=dt, box=box)
    assert np.isfinite(pos_x).all() and np.isfinite(vel_x).all()
    grav = np.array([0.0, abs(GRAVITY), 0.0])
    sv = np.abs(vel) + dt * (np.abs(Fo) / rho[:, None] + grav)
    sp = np.abs(pos) + dt * sv
    keep = ~fragile
    ev = (np.abs(np.asarray(vel_x, dtype=np.float64) - v64) / sv).max(axis=1)[keep]
    ep = (np.abs(np.asarray(pos_x, dtype=np.float64) - p64) / sp).max(axis=1)[keep]
    return ep, ev, float(fragile.mean())


def measure_step(pre_pos, pre_vel, rho_x, F_x, pos_x, vel_x, **kw):
    """All three kernels of one step of some fp32 implementation against float64, each on its own inputs:
    {"rho": errors, "F": errors, "pos": errors, "vel": errors, "fragile": fraction}"""
    rho64, Sd = density64(pre_pos, **kw)
    F64, Sf = force64(pre_pos, pre_vel, rho_x, **kw)
    ep, ev, frag = e_integrate(pos_x, vel_x, pre_pos, pre_vel, F_x, rho_x, **kw)
    return {"rho": e_rho(rho_x, rho64, Sd), "F": e_F(F_x, F64, Sf), "pos": ep, "vel": ev, "fragile": frag}


MEASURES = ("rho", "F", "pos", "vel")


def summary(m):
    """{measure: (max, mean)}"""
    return {k: (float(m[k].max()), float(m[k].mean())) for k in MEASURES}


def format_summary(name, s):
    return f"{name:>8}: " + "  ".join(f"e_{k} max {s[k][0]:.3e} mean {s[k][1]:.3e}" for k in MEASURES)


# ---- seeded inputs; every builder asserts its own precondition ----

def near_gate_pairs(pos):
    """pairs (i < j) with 0 < dist < NEAR_GATE, distances taken as the fp32 code sees them (float64 of the
    fp32 coordinates)"""
    pos = _f64(pos)
    out = []
    for i0, _i1, _d, dist2 in _pair_blocks(pos):
        a, j = np.nonzero((dist2 > 0) & (dist2 < NEAR_GATE * NEAR_GATE))
        out.extend((int(i0 + x), int(y)) for x, y in zip(a, j) if i0 + x < y)
    return out


def clear_eps_gate(pos, max_moved=None):
    """The pressure term does not vanish at the dist < EPS_F gate, so a pair sitting on it is a finite jump
    that no tolerance covers: move the later particle of every pair with 0 < dist < NEAR_GATE by 2e-3 along
    x and check again.  Returns the new positions and the number of particles moved."""
    pos = np.array(pos, dtype=F32)
    moved = set()
    for _ in range(8):
        pairs = near_gate_pairs(pos)
        if not pairs:
            break
        for j in sorted({j for _i, j in pairs}):
            pos[j, 0] += F32(2e-3)
            moved.add(j)
    assert not near_gate_pairs(pos), "pairs remain next to the EPS_F gate"
    if max_moved is not None:
        assert len(moved) <= max_moved, f"{len(moved)} particles moved off the EPS_F gate, at most {max_moved} allowed"
    return pos, len(moved)


def build_block():
    """dense_block(14, jitter=0.004) with velocities in +-2: 2,744 particles; the interior (61 %) is above the
    rest density, so all but the outermost rows carry a pressure term (p_i + p_j > 0)"""
    pos = dense_block(14, jitter=0.004)
    vel = np.random.default_rng(71).uniform(-2, 2, pos.shape).astype(F32)
    pos, moved = clear_eps_gate(pos, max_moved=0)
    rho, _ = density64(pos)
    assert len(pos) == 2744 and (rho > REST_DENSITY).mean() > 0.55, "the block's interior must be under pressure"
    return pos, vel


CLOUD_CORNERS = ((0.04, 0.05, 0.04), (9.95, 9.96, 9.95), (0.05, 9.95, 0.04))   # cells 0 / 99: outside the walls, inside the grid


def build_cloud():
    """4,000 particles: half in a thin floor layer (clustered_state), 30 moved into three corner cells of the
    grid (cells 0 and 99, beyond the wall planes: neighbour rows fall outside the grid, and the step clamps them), 20 exactly coincident pairs (dist = 0: every term gated in every
    mode)."""
    pos, vel = clustered_state(4000, 72)
    rng = np.random.default_rng(73)
    for k, c in enumerate(CLOUD_CORNERS):
        rows = slice(2000 + 10 * k, 2010 + 10 * k)
        pos[rows] = (np.asarray(c, F32) + rng.uniform(-0.02, 0.02, (10, 3))).astype(F32)
    pos, _ = clear_eps_gate(pos, max_moved=40)
    pos[3000:3020] = pos[100:120]          # floor-layer particles, exactly duplicated
    assert not near_gate_pairs(pos)
    d = _f64(pos[3000:3020]) - _f64(pos[100:120])
    assert not d.any(), "20 coincident pairs"
    cells = np.floor(_f64(pos) / H).astype(int)
    assert ((cells == 0).any(axis=1) | (cells == 99).any(axis=1)).sum() >= 30, "rows next to the box faces"
    assert len(pos) == 4000
    return pos, vel


EVOLVED_STEPS = 46


def build_evolved():
    """The strict oracle's own state after EVOLVED_STEPS steps of the block released at rest from y = 1, i.e. in
    the middle of its landing: free fall over 0.9 takes 43 steps (after 30 the block is still in mid-air and,
    relaxed, nowhere above the rest density: max rho 866).  Organic: the bottom layers lie on the floor or rebound
    at +2 while the top still falls at -4.5, rho runs from ~450 to ~2000 on both sides of the rest density.
    Computed on the CPU (seconds at this size).  Measured: 6 of the 2,744 particles are moved off the EPS_F gate;
    at most 1 % may be."""
    from oracle import oracle as O
    pos, _ = build_block()
    sim = O.OracleSim(len(pos), False)
    sim.upload(pos, None)
    sim.step(EVOLVED_STEPS)
    st = sim.download()
    sim.close()
    pos, moved = clear_eps_gate(st["pos"], max_moved=len(st["pos"]) // 100)
    rho, _ = density64(pos)
    assert 0.25 < (rho > REST_DENSITY).mean() < 0.75, "rho must straddle the rest density"
    vy = st["vel"][:, 1]
    assert (pos[:, 1] == F32(0.1)).any() and (vy > 1).any() and (vy < -1).any(), "on the floor, rebounding and still falling"
    return pos, np.ascontiguousarray(st["vel"]), moved


def h025_settings(settings_factory):
    """the 32-cell, h = 0.25, box = 8, dt = 0.004 settings of test_non_default_settings"""
    s = settings_factory(3001, False)
    s.h = 0.25
    s.boxDim = 8.0
    s.numCellsPerDim = 32
    s.timestep = 0.004
    from grid_states import kernel_coeffs
    s.v_kernel_coeff, s.d_kernel_coeff = kernel_coeffs(s.h)
    return s


def build_h025():
    """n = 3001 in the h = 0.25 box of test_non_default_settings (same seed, same distributions)"""
    hh, box, n = 0.25, 8.0, 3001
    rng = np.random.default_rng(3)
    pos = rng.uniform(1.5 * hh, box - 1.5 * hh, (n, 3)).astype(F32)
    vel = rng.uniform(-2, 2, (n, 3)).astype(F32)
    pos, _ = clear_eps_gate(pos, max_moved=30)
    return pos, vel
