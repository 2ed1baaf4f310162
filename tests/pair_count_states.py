"""The states tests/test_gpu_pair_counts.py counts pairs on, by name, so that tests/test_pair_counts_cpu.py can hold
the CPU restatement to the oracle's own pair-test count on every one of them without a GPU.
Each builder returns (pos, vel, h, cells); h = 0.1, cells = 100 are the reference settings."""
import numpy as np

from helpers import clustered_state, dense_block, nasty_state


def cube(n):
    """n particles in a 0.6-wide cube (test_odd_particle_counts): waves with 1..64 valid lanes."""
    rng = np.random.default_rng(100 + n)
    return (rng.uniform(4.0, 4.6, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32), 0.1, 100)


def shell():
    """The 8 corner cells, the 12 edges and the 6 faces of the grid occupied, positions on 0.1 and 9.9 (clipped runs:
    8, 12 and 18 existing neighbour cells), a handful per cell."""
    rng = np.random.default_rng(7)
    lo, hi = np.float32(0.1), np.float32(9.9)
    pts = []
    for fixed in range(1, 8):                              # which axes sit on a wall: 1-2 bits faces/edges, 3 corners
        for walls in range(8):
            p = rng.uniform(0.1, 9.9, (40, 3)).astype(np.float32)
            for ax in range(3):
                if fixed >> ax & 1:
                    p[:, ax] = hi if walls >> ax & 1 else lo
            pts.append(p)
    pos = np.concatenate(pts)
    pos[-64:] = np.repeat(pos[:8], 8, axis=0)[:64]          # coincident particles in corner / edge cells
    pos[:50, 0] = (hi - rng.uniform(0, 0.09, 50)).astype(np.float32)   # neighbours inside the last cell of an edge
    vel = rng.uniform(-1, 1, pos.shape).astype(np.float32)
    return np.ascontiguousarray(pos), vel, 0.1, 100


CUT_STEPS = (-1, 0, 1, 2)   # d2 = h*h moved by this many ulps


def cutoff(h, cells, n_total, per_step=12, seed=5):
    """Isolated pairs whose fp32 d2 = (dx dx + dy dy) + dz dz is EXACTLY h*h, one ulp below, one and two ulps
    above (found by search: d2 depends on the rounded coordinates), coincident pairs, and random filler up to
    n_total.  -> pos, vel, h, cells, picks {ulps: [(a, b)]} (indices of the pairs found)."""
    rng = np.random.default_rng(seed)
    hf = np.float32(h)
    h2 = hf * hf
    box = float(hf) * cells
    side = int((box - 4 * h) / (4 * h))
    m = 60000
    site = np.arange(m) % side ** 3
    base = np.stack([site % side, site // side % side, site // side ** 2], axis=1) * (4 * h) + 2 * h
    a = (base + rng.uniform(0, h, (m, 3))).astype(np.float32)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = (a + d * (float(hf) * (1 + rng.uniform(-3e-7, 3e-7, (m, 1))))).astype(np.float32)
    e = a - b
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    target = {0: h2}
    target[-1] = np.nextafter(h2, np.float32(0))
    target[1] = np.nextafter(h2, np.float32(np.inf))
    target[2] = np.nextafter(target[1], np.float32(np.inf))
    used, rows, picks = set(), [], {}
    for s in CUT_STEPS:
        picks[s] = []
        for k in np.nonzero(d2 == target[s])[0]:
            if site[k] not in used and len(picks[s]) < per_step:
                used.add(int(site[k]))
                picks[s].append((len(rows), len(rows) + 1))
                rows += [a[k], b[k]]
        assert len(picks[s]) == per_step, "search too short"
    free = [s for s in range(side ** 3) if s not in used][:per_step]
    picks["same"] = []
    for s in free:                                          # coincident pairs, isolated as well
        p = (np.array([s % side, s // side % side, s // side ** 2]) * (4 * h) + 2.5 * h).astype(np.float32)
        picks["same"].append((len(rows), len(rows) + 1))
        rows += [p, p]
    pos = np.array(rows, np.float32)
    picks["isolated"] = len(pos)
    if n_total > len(pos):                                  # filler: anywhere (may land next to a pair)
        pos = np.concatenate([pos, rng.uniform(1.5 * h, box - 1.5 * h, (n_total - len(pos), 3)).astype(np.float32)])
    vel = rng.uniform(-2, 2, pos.shape).astype(np.float32)
    return pos, vel, float(h), cells, picks


def mixture(seed=3):
    """test_gpu_parity.co_moving_mixture's recipe at the smallest size that holds all four kinds of row: a cloud
    that shares ONE velocity (quiet rows), a block moving with the same velocity that IS under pressure (spacing
    0.025: rho > 1000 inside; the 0.03 of co_moving_mixture stays at rho = 820 and never switches pressure on),
    rows with velocities of their own scattered through the cloud, and one particle at rest."""
    rng = np.random.default_rng(seed)
    blk = dense_block(14, spacing=0.025, origin=(3.0, 3.0, 3.0), jitter=0.003, seed=seed)
    n = len(blk) + 2000
    pos = rng.uniform(2.6, 4.0, (n, 3)).astype(np.float32)
    vel = np.tile(np.array([0.25, -1.5, 0.125], np.float32), (n, 1))
    pos[:len(blk)] = blk
    odd = rng.choice(np.arange(len(blk), n), 150, replace=False)
    vel[odd] = rng.uniform(-1, 1, (len(odd), 3)).astype(np.float32)
    vel[odd[0]] = 0.0
    return pos, vel, 0.1, 100


def at_rest():
    """default_settings(20000, True): the reference's random start, every velocity zero."""
    from oracle import oracle as O
    return O.init_positions(O.make_settings(20000, True)), np.zeros((20000, 3), np.float32), 0.1, 100


def _plain(f, *a):
    return lambda: f(*a) + (0.1, 100)


STATES = {
    **{f"cube{n}": (lambda n=n: cube(n)) for n in (0, 1, 2, 63, 64, 65, 129)},
    "shell": shell,
    **{f"nasty{s}": _plain(nasty_state, 3000, s) for s in (0, 1, 2)},
    "clustered": _plain(clustered_state, 30000, 5),
    "block": lambda: (dense_block(14, jitter=0.003), None, 0.1, 100),
    "cut0.1": lambda: cutoff(0.1, 100, 0)[:4],
    "cut0.2": lambda: cutoff(0.2, 32, 3001)[:4],
    "cut0.25": lambda: cutoff(0.25, 32, 3001)[:4],
    "mixture": mixture,
    "at_rest": at_rest,
    "nasty_slabs": _plain(nasty_state, 12000, 50),
}


def state(name):
    pos, vel, h, cells = STATES[name]()
    if vel is None:
        vel = np.zeros_like(pos)
    return pos, vel, h, cells
