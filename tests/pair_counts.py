"""CPU restatement of the three numbers the library reports about its own work (include/sph_c_api.h,
"What the pair counters report"): candidate pair tests, hits, and pair bodies of ONE step.  Plain numpy, per
cell, written from the header's wording; shares no code with the library or the oracle.

    c = count(pos, vel, rho, order_in, h=0.1, cells=100)

pos / vel: the state the step starts from, particle-id order.  rho: the densities of THAT step (the oracle's),
needed for the filter only.  order_in: the order of the rows the step's grid build starts from (ids; None = id
order, i.e. a freshly uploaded state; afterwards the previous step's `order_out`)."""
import numpy as np

GAS_CONSTANT = np.float32(1.0)
REST_DENSITY = np.float32(1000.0)


def cells_of(pos, h, cells):
    """Cell of a position: fp32 divide by h, truncate, clamped to the grid."""
    c = (np.asarray(pos, np.float32) / np.float32(h)).astype(np.float32).astype(np.int64)
    return np.clip(c, 0, int(cells) - 1)


def reference_velocity(vel, order_in):
    """The zero-pair filter's reference velocity: the most common bit pattern among the velocities of the 64 rows
    floor(k n / 64), k = 0..63, of the order the grid build starts from; ties go to the lowest k."""
    n = len(vel)
    rows = (np.arange(64, dtype=np.int64) * n) // 64
    sample = np.ascontiguousarray(vel[order_in[rows]], dtype=np.float32).view(np.uint32)
    votes = (sample[:, None, :] == sample[None, :, :]).all(axis=2).sum(axis=1)
    return np.ascontiguousarray(vel[order_in[rows[int(np.argmax(votes))]]], dtype=np.float32)  # (argmax: first maximum)


def _expand(starts, lens):
    """(i, j) for every i and every j in [starts[i], starts[i] + lens[i])."""
    total = int(lens.sum())
    i = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    first = np.repeat(np.cumsum(lens) - lens, lens)
    j = np.repeat(starts, lens) + (np.arange(total, dtype=np.int64) - first)
    return i, j


def count(pos, vel=None, rho=None, order_in=None, h=0.1, cells=100, zero_pair_filter=True, owned=None):
    """-> dict: tests, hits, bodies (ints); tests_i, hits_i, bodies_i (per particle, id order); order_out (ids in the
    step's cell-sorted order); words_i (per particle: sum over its nine runs of ceil(candidates / 32), what a row's
    hit stream can take); runmax_i (the longest of those runs); quiet (bool per particle, None without vel / rho).
    owned: bool mask of the rows that count (slabs: the others are candidates only and never quiet; pos / vel /
    rho are then the slab's combined array, in the order its sort starts from)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    n, D = len(pos), int(cells)
    hf = np.float32(h)
    h2 = hf * hf
    order_in = np.arange(n, dtype=np.int64) if order_in is None else np.asarray(order_in, dtype=np.int64)
    own = np.ones(n, bool) if owned is None else np.asarray(owned, bool)
    zero = np.zeros(n, np.int64)
    out = dict(tests=0, hits=0, bodies=0, tests_i=zero, hits_i=zero.copy(), bodies_i=zero.copy(), words_i=zero.copy(), runmax_i=zero.copy(),
               order_out=order_in.copy(), quiet=None)
    if n == 0:
        return out
    c = cells_of(pos, hf, D)
    key = c[:, 0] + c[:, 1] * D + c[:, 2] * D * D
    order = order_in[np.argsort(key[order_in], kind="stable")]      # the step's sorted order
    skey = key[order]
    occupied, start, occ = np.unique(skey, return_index=True, return_counts=True)

    quiet = None
    if vel is not None and rho is not None and zero_pair_filter:
        vel = np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)
        prs = np.maximum(np.float32(0), GAS_CONSTANT * (np.asarray(rho, np.float32) - REST_DENSITY))
        vref = reference_velocity(vel, order_in)
        quiet = (prs == 0) & (vel == vref).all(axis=1)               # (float compare: -0 equals +0)
        if owned is not None:
            quiet &= own                                              # slabs: a halo row is never quiet

    tests_i, hits_i, drop_i = zero.copy(), zero.copy(), zero.copy()
    words_i, runmax_i = zero.copy(), zero.copy()
    ps = pos[order]
    qs = quiet[order] if quiet is not None else None
    rows = np.nonzero(own[order])[0]                                 # sorted rows that count
    cr = c[order][rows]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            run = np.zeros(len(rows), np.int64)                      # one run: the x-neighbours of one (y, z)
            for dx in (-1, 0, 1):
                x, y, z = cr[:, 0] + dx, cr[:, 1] + dy, cr[:, 2] + dz
                inside = (x >= 0) & (x < D) & (y >= 0) & (y < D) & (z >= 0) & (z < D)
                nk = np.where(inside, x + y * D + z * D * D, -1)
                at = np.searchsorted(occupied, nk)
                at = np.minimum(at, len(occupied) - 1)
                found = inside & (occupied[at] == nk)
                lens = np.where(found, occ[at], 0)
                run += lens
                np.add.at(tests_i, rows, lens)
                i, j = _expand(start[at], lens)
                if len(i) == 0:
                    continue
                i = rows[i]
                # fp32, every operation rounded on its own
                ex = ps[i, 0] - ps[j, 0]
                ey = ps[i, 1] - ps[j, 1]
                ez = ps[i, 2] - ps[j, 2]
                d2 = (ex * ex + ey * ey) + ez * ez
                hit = (d2 <= h2) | (np.sqrt(d2) <= hf)
                hits_i += np.bincount(i[hit], minlength=n)
                if qs is not None:
                    drop_i += np.bincount(i[hit & qs[i] & qs[j]], minlength=n)
            np.add.at(words_i, rows, (run + 31) // 32)
            np.maximum.at(runmax_i, rows, run)

    def by_id(a):
        b = np.zeros(n, np.int64)
        b[order] = a
        return b
    out.update(tests_i=by_id(tests_i), hits_i=by_id(hits_i), bodies_i=by_id(hits_i - drop_i), words_i=by_id(words_i), runmax_i=by_id(runmax_i),
               order_out=order, quiet=quiet)
    out["tests"], out["hits"] = int(tests_i.sum()), int(hits_i.sum())
    out["bodies"] = int((hits_i - drop_i).sum())
    return out


def waves(c):
    """Per wave (64 consecutive rows of the step's sorted order): hits, bodies, and the 16-byte quads its hit stream
    reserves: 64 Q, Q = ceil(W / 2), W = the largest words_i among its rows."""
    o = c["order_out"]
    nw = (len(o) + 63) // 64
    pad = nw * 64 - len(o)
    def per(a, red):
        return red(np.concatenate([a[o], np.zeros(pad, np.int64)]).reshape(nw, 64), axis=1)
    return per(c["hits_i"], np.sum), per(c["bodies_i"], np.sum), 64 * ((per(c["words_i"], np.max) + 1) // 2)


def pool_outcomes(c, pool_words):
    """The (hits, bodies) a step may report when the hit-stream pool holds `pool_words` 32-bit words: 64 equal
    sub-pools of pool_words / 4 / 64 quads, wave w reserves from sub-pool w mod 64 in arrival order, every arrival
    advances the cursor, a wave that does not fit reports nothing.  For a sub-pool smaller than two reservations
    (< 128 quads): at most the first arrival fits, and only if it needs 64 quads."""
    hw, bw, need = waves(c)
    sub = pool_words // 4 // 64
    assert 64 <= sub < 128
    reach = {(0, 0)}
    for shard in range(64):
        w = np.arange(shard, len(hw), 64)
        opts = {(int(hw[k]), int(bw[k])) for k in w if need[k] <= sub}
        if (need[w] > sub).any() or not len(w):
            opts.add((0, 0))
        reach = {(a + x, b + y) for a, b in reach for x, y in opts}
    return reach
