"""The particle states the neighbour lists' tests add to those of body_states.py and grid_states.py
(tests/test_neighbours_cpu.py, tests/test_gpu_neighbours.py): built by the caller, never written to afterwards."""
import numpy as np

import grid_states as G

F = np.float32


def put_on_the_walls(pos, g, what, first=0):
    """rows first .. of pos moved (in place) onto the wall planes: coordinates 0 and the largest float below the box"""
    top = np.nextafter(G.box_of(g["h"], g["cells"]), F(0))
    k = min(len(pos) // 4, 24)
    assert first + k + 1 < len(pos)
    for i in range(k):
        pos[first + i, i % 3] = F(0) if (i // 3) % 2 == 0 else top
    pos[first + k] = (F(0), F(0), F(0))
    pos[first + k + 1] = (top, top, top)
    G.assert_inside(pos, g["h"], g["cells"], what)
    return pos


def on_the_walls(name):
    """a grid_states state with rows moved onto the wall planes: coordinates 0 and the largest float below the box"""
    pos, vel, g = G.grid_state(name)
    return put_on_the_walls(pos, g, name), vel, g


def far_pair():
    """two cells of one particle each, further than any radius apart"""
    return np.array([[1.05, 1.05, 1.05], [5.05, 5.05, 5.05]], F)


def balls(sizes, seed):
    """len(sizes) balls of radius 0.01 (every particle of a ball within 0.035 of every other) in cells far from each
    other, sizes[k] particles in ball k, the particle ids shuffled over all of them: lists of exactly sizes[k] - 1
    -> (pos by id, the ball of every id)"""
    rng = np.random.default_rng(seed)
    parts, ball = [], []
    for k, m in enumerate(sizes):
        centre = np.array([2.05 + 2.0 * k, 5.05, 5.05])
        parts.append(centre + rng.uniform(-0.01, 0.01, (m, 3)))
        ball += [k] * m
    order = rng.permutation(len(ball))
    return np.concatenate(parts).astype(F)[order], np.array(ball)[order]
