"""The field sample's numpy restatement (tests/field_sample_restatement.py) against the CPU oracle and against
hand-derived values.  A density sample at a point is the sum kernelUpdatePressureAndDensity forms for a particle
at that point: oracle_density, asked for query rows appended behind the particles, must give max(sample, EPS_F)
bit for bit.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import field_sample_restatement as FS
from oracle import oracle as O

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_grid(s, pos, vel=None, rho=None):
    """the oracle's grid of a state in particle-id order: sorted pos, vel, rho and the (D^3, 2) cell ranges"""
    pos = np.ascontiguousarray(pos, dtype=F)
    D = int(s.numCellsPerDim)
    keys = O.cell_keys(s, pos)
    perm = O.stable_sort(keys, D ** 3)
    cs, ce = O.cell_table(keys[perm], D ** 3)
    vel = np.zeros_like(pos) if vel is None else np.ascontiguousarray(vel, dtype=F)
    rho = np.zeros(len(pos), F) if rho is None else np.ascontiguousarray(rho, dtype=F)
    return pos[perm], vel[perm], rho[perm], np.stack([cs, ce], axis=1)


def restate(s, grid, field, origin, spacing, shape):
    pos, vel, rho, cells = grid
    return FS.sample(pos, vel, rho, cells, s.h, s.d_kernel_coeff, s.numCellsPerDim, field, origin, spacing, shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# (origin, spacing, (nz, ny, nx)); `a` is a point inside the fluid
def lattices(a):
    ax, ay, az = (float(v) for v in a)
    return [((ax - 0.1, ay - 0.05, az - 0.05), (0.001, 0.05, 0.05), (3, 3, 200)),    # 64 points in a row share a cell
            ((ax - 1.5, ay - 0.15, az - 0.15), (0.15, 0.15, 0.15), (3, 3, 65)),      # every point a cell of its own
            ((-0.05, 0.03, 0.03), (0.0506, 4.98, 4.98), (3, 3, 200)),               # cells 0 and D - 1, x below 0 and past 10
            ((ax, ay, az), (0.1, 0.1, 0.1), (1, 1, 1))]


@pytest.mark.parametrize("name", ["random4096", "dense4096"])
def test_density_restatement_is_the_oracles_density_sum(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    n = len(data["pos_1"])
    s = O.make_settings(n, True)
    grid = oracle_grid(s, data["pos_1"])
    pos, cells = grid[0], grid[3]
    seen_fluid = 0
    for origin, spacing, shape in lattices(data["pos_1"][7]):
        got = restate(s, grid, "density", origin, spacing, shape).reshape(-1)
        pts = FS.lattice_points(origin, spacing, shape).reshape(-1, 3)
        c, outside = FS.cells_of(pts, s.h, s.numCellsPerDim)
        inside = ~outside.any(axis=1)
        assert (got[~inside].view(np.uint32) == 0).all()                  # +0 outside the grid
        q = np.ascontiguousarray(pts[inside])
        # the restatement's cell of a point is the cell hash's
        D = int(s.numCellsPerDim)
        assert np.array_equal(O.cell_keys(s, q), ((c[inside, 2] * D + c[inside, 1]) * D + c[inside, 0]).astype(np.uint32))
        both = np.ascontiguousarray(np.concatenate([pos, q]))
        rho, _ = O.density(s, both, np.ascontiguousarray(cells[:, 0]), np.ascontiguousarray(cells[:, 1]), n, n + len(q))
        want = rho[n:]
        assert np.array_equal(bits(np.maximum(got[inside], FS.EPS_F)), bits(want)), f"{name} {origin} {spacing} {shape}"
        seen_fluid += int((got > 0).sum())
    assert seen_fluid > 100, "the lattices miss the fluid: nothing is compared but zeros"


def _settings():
    return O.make_settings(2, False)


def _m(s, d2):
    """MASS * (((d_kernel_coeff * diff) * diff) * diff), diff = h*h - d2, written out in float32 scalars"""
    h2 = F(s.h) * F(s.h)
    diff = h2 - F(d2)
    return F(0.02) * (((F(s.d_kernel_coeff) * diff) * diff) * diff)


def test_known_answer_distance_zero():
    s = _settings()
    p = np.array([[0.55, 0.55, 0.55]], F)
    grid = oracle_grid(s, p, vel=np.array([[3, 4, 12]], F), rho=np.array([1234.5], F))
    at = tuple(float(v) for v in p[0])
    m = _m(s, 0.0)
    assert m > 0
    assert bits(restate(s, grid, "density", at, (1, 1, 1), (1, 1, 1))).item() == bits(m).item()
    # Shepard of one particle: (m a) / m, a = 13 and 234.5
    assert bits(restate(s, grid, "speed", at, (1, 1, 1), (1, 1, 1))).item() == bits((m * F(13)) / m).item()
    assert bits(restate(s, grid, "pressure", at, (1, 1, 1), (1, 1, 1))).item() == bits((m * F(234.5)) / m).item()


def test_known_answer_d2_equal_to_h2_adds_a_zero_term():
    s = _settings()
    h = F(s.h)
    # the point (h, y, z) is exactly h away from the particle at (0, y, z): d2 = (h*h + 0) + 0 == h*h, not > h*h,
    # diff = 0 and the term is +0; the second particle sits on the point and gives m(0)
    p = np.array([[0.0, 0.55, 0.55], [float(h), 0.55, 0.55]], F)
    one = oracle_grid(s, p[:1], vel=np.array([[1, 0, 0]], F))
    at = (float(h), float(p[0, 1]), float(p[0, 2]))
    assert bits(restate(s, one, "density", at, (1, 1, 1), (1, 1, 1))).item() == 0
    assert bits(restate(s, one, "speed", at, (1, 1, 1), (1, 1, 1))).item() == 0      # den is not > 0
    two = oracle_grid(s, p)
    assert bits(restate(s, two, "density", at, (1, 1, 1), (1, 1, 1))).item() == bits(F(0) + _m(s, 0.0)).item()
    # one ulp further the candidate is rejected, one ulp nearer it counts
    near = float(np.nextafter(h, F(0)))
    d2 = F(near) * F(near)
    assert d2 < h * h
    assert bits(restate(s, one, "density", (near, at[1], at[2]), (1, 1, 1), (1, 1, 1))).item() == bits(_m(s, d2)).item() != 0


def test_known_answer_outside_points_are_zero():
    s = _settings()
    p = np.array([[0.01, 0.01, 0.01], [9.99, 9.99, 9.99]], F)
    grid = oracle_grid(s, p, vel=np.ones((2, 3), F), rho=np.full(2, 1500, F))
    for field in FS.FIELDS:
        # x = -0.05 and x = 0.01: the first is outside although the particle is well within h of it
        got = restate(s, grid, field, (-0.05, 0.01, 0.01), (0.06, 1, 1), (1, 1, 2)).reshape(-1)
        assert bits(got)[0] == 0 and got[1] > 0
        # 10.0 / 0.1f rounds to 100: cell D, outside; 9.99 is cell D - 1
        got = restate(s, grid, field, (9.99, 9.99, 9.99), (0.01, 1, 1), (1, 1, 2)).reshape(-1)
        assert got[0] > 0 and bits(got)[1] == 0
        for axis in range(3):
            o = [0.01, 0.01, 0.01]
            o[axis] = float("-0.0")                                    # -0 >= 0: inside, cell 0
            assert restate(s, grid, field, tuple(o), (1, 1, 1), (1, 1, 1)).item() > 0
            o[axis] = -1e-30
            assert bits(restate(s, grid, field, tuple(o), (1, 1, 1), (1, 1, 1))).item() == 0


def test_known_answer_shepard_of_two_particles():
    s = _settings()
    # both in cell (5, 5, 5); stream order = id order (stable sort); the point lies between them on the x axis
    p = np.array([[0.52, 0.55, 0.55], [0.58, 0.55, 0.55]], F)
    v = np.array([[3, 0, 4], [0, 0, 2]], F)                            # speeds 5 and 2
    rho = np.array([1500, 1002], F)                                    # pressures 500 and 2
    grid = oracle_grid(s, p, v, rho)
    x = F(0.54)
    d = [x - p[0, 0], x - p[1, 0]]
    m = [_m(s, (dx * dx + F(0)) + F(0)) for dx in d]
    den = (F(0) + m[0]) + m[1]
    at = (float(x), 0.55, 0.55)
    assert bits(restate(s, grid, "density", at, (1, 1, 1), (1, 1, 1))).item() == bits(den).item()
    for field, a in (("speed", (F(5), F(2))), ("pressure", (F(500), F(2)))):
        num = (F(0) + m[0] * a[0]) + m[1] * a[1]
        got = restate(s, grid, field, at, (1, 1, 1), (1, 1, 1)).item()
        assert bits(F(got)).item() == bits(num / den).item()
        assert a[1] < got < a[0] and m[0] != m[1]


def test_lattice_index_order_and_position_rounding():
    # index (iz * ny + iy) * nx + ix; p = origin + (float)i * spacing, the product rounded before the sum
    pts = FS.lattice_points((0.1, 0.2, 0.3), (0.7, 0.11, 0.013), (4, 3, 5))
    assert pts.shape == (4, 3, 5, 3)
    flat = pts.reshape(-1, 3)
    for ix, iy, iz in ((0, 0, 0), (4, 2, 3), (3, 1, 2)):
        want = [F(o) + F(i) * F(sp) for o, i, sp in zip((0.1, 0.2, 0.3), (ix, iy, iz), (0.7, 0.11, 0.013))]
        assert [bits(w).item() for w in want] == bits(flat[(iz * 3 + iy) * 5 + ix]).tolist()
