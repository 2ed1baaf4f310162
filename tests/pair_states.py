"""The particle states of the pair statistics' tests (tests/test_pairs_cpu.py, tests/test_gpu_pairs.py): those of
body_states.py, grid_states.py and neighbour_states.py with random non-zero velocities where they have none, and the
few the pass needs of its own.  state(name) -> (pos, vel, h, cells), built once per process, never written to."""
import numpy as np

import body_states as BS
import neighbour_states as NS
import pair_restatement as PR

F = np.float32
H = F(0.1)
SLICE = 192          # pairs.hip's PAIR_SLICE (kPairSlice): the longest run the walk stages
EDGE_BINS = 8
_cache = {}


def velocities(n, seed, scale=2.0):
    """n velocities uniform in +-scale per axis, none zero"""
    v = np.random.default_rng(seed).uniform(-scale, scale, (n, 3)).astype(F)
    v[v == 0] = F(0.5)
    return v


def on_the_edges(bins=EDGE_BINS):
    """Particle 0 at the origin corner -- e = p_j exactly -- and for every edge of the `bins`-bin table of radius h
    seven particles on the x axis, within +-3 ulps of the fp32 square root of the edge; the last edge with them: taken
    and not taken.  -> (pos, the edges)"""
    edges = PR.edges2(0.0, H, bins)
    xs = [F(0)]
    for e in edges:
        x = np.sqrt(e)
        assert type(x) is F
        for _ in range(3):
            x = np.nextafter(x, F(0))
        for _ in range(7):
            xs.append(x)
            x = np.nextafter(x, F(1))
    pos = np.zeros((len(xs), 3), F)
    pos[:, 0] = xs
    return pos, edges


def assert_edges_straddled(pos, edges):
    """on_the_edges() holds what it says: the origin's pairs fall on both sides of every edge, one of them within an ulp
    of it; the last edge -- r2 -- has them taken and not taken"""
    assert (pos[0] == 0).all() and not pos[:, 1:].any() and len(pos) == 1 + 7 * len(edges)
    x = pos[1:, 0]
    d2 = x * x
    assert d2.dtype == F
    for k, e in enumerate(edges):
        mine = d2[7 * k:7 * k + 7]
        assert (mine <= e).any() and (mine > e).any(), k
        assert (np.abs(mine.view(np.int32).astype(np.int64) - int(e.view(np.int32))) <= 1).any(), k
    assert edges[-1] == H * H and (d2 > edges[-1]).any() and (d2[-7:] <= edges[-1]).any()


def saturating(seed=21):
    """48 particles in a cube of side 0.08: velocities of +-1e6 (|dv|^2 and u_par^2 beyond 2^31), one NaN velocity
    component, two coincident particles and one at rest among slow ones"""
    pos = BS.cluster(48, seed, lo=(3.01, 3.01, 3.01), side=0.08)
    vel = velocities(48, seed + 1)
    vel[5] = (1e6, -1e6, 1e6)
    vel[9] = (-1e6, 1e6, -1e6)
    vel[17, 1] = np.nan
    vel[30] = 0
    pos[41] = pos[40]
    return pos, vel


def saturating_tiles(seed=31):
    """300 particles in a cube of side 0.2 -- five tiles of 64 rows -- with velocities of +-1e12 and +-1e6 among slow
    ones: dozens of |dv|^2 terms clamped at the top, e.dv terms clamped at the top and at the bottom, in every bin of
    a coarse table"""
    pos = BS.cluster(300, seed, lo=(6.01, 6.01, 6.01), side=0.2)
    vel = velocities(300, seed + 1)
    for k, i in enumerate(range(3, 300, 37)):
        big = F(1e12) if k % 2 else F(1e6)
        vel[i] = (big, -big, big) if k % 4 < 2 else (-big, big, -big)
    return pos, vel


def build(name):
    if name.startswith("tail"):
        n = int(name[4:])
        return BS.cluster(n, n), velocities(n, 100 + n), H, 100
    if name == "far_pair":
        return NS.far_pair(), velocities(2, 7), H, 100
    if name == "coincident":
        return np.array([[5.05, 5.05, 5.05]] * 2, F), velocities(2, 8), H, 100
    if name == "edges":
        pos, _ = on_the_edges()
        return pos, velocities(len(pos), 9), H, 100
    if name == "saturating":
        return saturating() + (H, 100)
    if name == "saturating_tiles":
        return saturating_tiles() + (H, 100)
    if name == "slice":
        pos, _ = NS.balls((SLICE, SLICE + 1), 12)
        return pos, velocities(len(pos), 13), H, 100
    if name in ("dense4096", "random4096"):
        pos, vel = BS.big(name)
        if not vel.any():
            vel = velocities(len(pos), 14)
        return pos, vel, H, 100
    if name in ("D1", "D2", "D3"):
        pos, vel, g = NS.on_the_walls(name)
        return pos, vel, F(g["h"]), g["cells"]
    if name == "D10h025":
        import grid_states as G
        pos, vel, g = G.grid_state(name)
        return pos, vel, F(g["h"]), g["cells"]
    raise KeyError(name)


def state(name):
    if name not in _cache:
        pos, vel, h, cells = build(name)
        _cache[name] = (np.ascontiguousarray(pos, F), np.ascontiguousarray(vel, F), h, cells)
    return _cache[name]


TAILS = ("tail1", "tail2", "tail63", "tail64", "tail65", "tail130")
SMALL = TAILS + ("far_pair", "coincident", "edges", "saturating", "saturating_tiles", "D1", "D2", "D3", "D10h025")
ALL = SMALL + ("slice", "dense4096", "random4096")
