"""The neighbour lists ("Neighbour lists") restated in numpy, twice and independently of
each other; the test itself is bodies_restatement's (every operation one np.float32 ufunc call, rounded on its own).

all_pairs(): every pair of particles tested, in chunks of rows; no grid, no walk.  Lists come out ascending.

walk_order(): the 27-cell walk over a grid -- the cell-sorted positions, the particle id of every row and the cell
table's {start, end} ranges (sph_download_grid + sph_download_state, or grid_of() below) -- with the lists in the order
of the walk, put back in particle-id order.

Both return CSR: (offsets (n + 1,) uint64, neighbours (entries,) uint32).  Imports nothing from the product."""
import numpy as np

import bodies_restatement as BR

F = np.float32


def csr(lists):
    """lists[i]: the neighbours of particle id i -> (offsets, neighbours)"""
    offsets = np.zeros(len(lists) + 1, np.uint64)
    if len(lists):
        offsets[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    flat = np.concatenate(lists).astype(np.uint32) if len(lists) and int(offsets[-1]) else np.zeros(0, np.uint32)
    return offsets, flat


def lists_of(offsets, neighbours):
    o = offsets.astype(np.int64)
    return [neighbours[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def all_pairs(pos, h, radius, chunk=512):
    """pos (n, 3) in particle-id order"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = len(pos)
    r2 = BR.link_r2(h, radius)
    everyone = np.arange(n)
    lists = []
    for k in range(0, n, chunk):
        take = BR.linked(pos[k:k + chunk], pos, r2)
        take &= everyone[None, :] != everyone[k:k + chunk, None]
        lists += [np.flatnonzero(row) for row in take]
    return csr(lists)


def walk_order(pos_rows, ids, cell_ranges, h, D, radius):
    """pos_rows (n, 3): the SORTED stream, ids (n,): the particle id of every row, cell_ranges (D^3, 2) int32"""
    pos = np.ascontiguousarray(pos_rows, dtype=F).reshape(-1, 3)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    cell_ranges = np.asarray(cell_ranges, dtype=np.int32).reshape(-1, 2)
    n, D = len(pos), int(D)
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n))
    r2 = BR.link_r2(h, radius)
    lists = [np.zeros(0, np.int64)] * n
    c = BR.row_cells(pos, h, D)
    key = (c[:, 2] * D + c[:, 1]) * D + c[:, 0]
    for k in (np.unique(key) if n else ()):
        who = np.flatnonzero(key == k)
        cand = BR.neighbourhood(cell_ranges, D, int(k % D), int(k // D % D), int(k // (D * D)))
        take = BR.linked(pos[who], pos[cand], r2) & (ids[cand][None, :] != ids[who][:, None])
        for row, t in zip(who, take):
            lists[ids[row]] = ids[cand[t]]
    return csr(lists)


def grid_of(pos, h, D):
    """a grid of positions in particle-id order, built on the CPU: (pos_rows, ids, cell_ranges) -- the rows of a cell in
    id order (the definition holds for any order: it goes through the grid it is given)"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    D = int(D)
    c = BR.row_cells(pos, h, D)
    key = (c[:, 2] * D + c[:, 1]) * D + c[:, 0]
    ids = np.argsort(key, kind="stable")
    start = np.searchsorted(key[ids], np.arange(D ** 3), side="left")
    end = np.searchsorted(key[ids], np.arange(D ** 3), side="right")
    ranges = np.stack([start, end], axis=1).astype(np.int32)
    ranges[start == end] = 0   # an empty cell holds {0, 0}
    return pos[ids], ids, ranges
