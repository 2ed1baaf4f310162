"""The particle states of the bodies' tests (tests/test_bodies_cpu.py, tests/test_gpu_bodies.py), all for the default
grid (h = 0.1, 100^3 cells): built once per process, shared, never written to."""
import os

import numpy as np

F = np.float32
H = F(0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
_cache = {}


def golden(name):
    data = np.load(os.path.join(GOLD, name + ".npz"))
    return np.ascontiguousarray(data["pos_1"], dtype=F), np.ascontiguousarray(data["vel_1"], dtype=F)


def uniform4096():
    """4,096 points uniform in the cube of side 1.5 at (2, 2, 2), seed 1: a giant body, several of >= 64 and
    hundreds of singletons, depending on the link length"""
    rng = np.random.default_rng(1)
    return (F(2) + rng.uniform(0, 1.5, (4096, 3))).astype(F), np.zeros((4096, 3), F)


def big(name):
    if name not in _cache:
        _cache[name] = uniform4096() if name == "uniform4096" else golden(name)
    return _cache[name]


# (state, link): link 0 is h
BIG = [(s, l) for s in ("dense4096", "random4096", "uniform4096") for l in (0.0, 0.08, 0.025)] + [("uniform4096", 0.06)]


def d2_of(p, q):
    e = [F(q[a]) - F(p[a]) for a in range(3)]
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert type(d2) is F
    return d2


def boundary_pairs():
    """Four particles: a pair with d2 == r2 exactly (linked), found by walking the second particle outwards one float
    at a time until the link breaks, and beside it the pair one float further apart (not linked).  -> (pos, d2 of the
    two pairs, r2)"""
    r2 = H * H
    a = np.array([0.0, 5.05, 5.05], F)   # on the wall plane x = 0: e = q - a is q itself
    q = a.copy()
    q[0] = H * F(0.999)
    assert d2_of(a, q) < r2
    while True:
        nxt = q.copy()
        nxt[0] = np.nextafter(q[0], F(1))
        if d2_of(a, nxt) > r2:
            break
        q = nxt
    b = np.array([0.0, 7.05, 5.05], F)
    far = nxt.copy()
    far[1] = b[1]
    pos = np.stack([a, q, b, far]).astype(F)
    return pos, (d2_of(a, q), d2_of(b, far)), r2


def chain(without_middle=False, seed=3):
    """257 particles 0.09 apart along a path with three long rows 0.27 apart (the box is too short for a straight
    line), particle ids shuffled.  -> (pos by id, the path position of every id)"""
    moves = [(1, 0)] * 80 + [(0, 1)] * 3 + [(-1, 0)] * 80 + [(0, 1)] * 3 + [(1, 0)] * 80 + [(0, 1)] * 3 + [(-1, 0)] * 7
    at = np.cumsum(np.array([(0, 0)] + moves), axis=0)
    assert len(at) == 257
    path = np.stack([F(1) + F(0.09) * at[:, 0].astype(F), F(1) + F(0.09) * at[:, 1].astype(F), np.full(257, 5.05, F)], axis=1)
    where = np.arange(257)
    if without_middle:
        where = np.delete(where, 128)
    rng = np.random.default_rng(seed)
    where = rng.permutation(where)        # where[id] = path position of particle id
    return path[where].astype(F), where


def blobs(bridge=True, seed=11):
    """two blobs of 200 in cubes of side 0.2 that are 0.16 apart, each with one particle at the middle of the facing
    side, and (bridge) one particle half way between those two, 0.09 from either"""
    rng = np.random.default_rng(seed)
    a = (np.array([5.0, 5.0, 5.0]) + rng.uniform(0, 0.2, (200, 3))).astype(F)
    b = (np.array([5.36, 5.0, 5.0]) + rng.uniform(0, 0.2, (200, 3))).astype(F)
    a[7] = (5.19, 5.1, 5.1)
    b[9] = (5.37, 5.1, 5.1)
    parts = [a, b] + ([np.array([[5.28, 5.1, 5.1]], F)] if bridge else [])
    pos = np.concatenate(parts).astype(F)
    order = rng.permutation(len(pos))
    return pos[order], order              # order[id] = index into (blob a, blob b, bridge)


def cluster(n, seed, lo=(0.5, 0.5, 0.5), side=0.25):
    """n particles in a cube of `side` at `lo`: a few cells"""
    rng = np.random.default_rng(seed)
    return (np.asarray(lo) + rng.uniform(0, side, (n, 3))).astype(F)


def one_cell(n, seed, cell):
    """n particles inside one cell of the 100^3 grid, away from its faces"""
    rng = np.random.default_rng(seed)
    return ((np.asarray(cell) + rng.uniform(0.1, 0.9, (n, 3))) * 0.1).astype(F)
