"""The bodies ("Bodies") restated in numpy and plain Python.

bodies(): the link test of the definition through the cell table, every operation one np.float32 ufunc call (rounded on
its own, no FMA), then a SEQUENTIAL union-find over the links, then the table.  Imports nothing from the product and
nothing from the other restatements.  It is fed by the grid the sweep walked: the cell-sorted positions, the particle
id of every row and the cell table's {start, end} ranges (sph_download_grid + sph_download_state, or the oracle's sort
and table).

all_pairs_components(): the same graph without the cell table -- an O(n^2) fp32 link matrix handed to scipy -- for
tests/test_bodies_cpu.py, which holds the two against each other."""
import numpy as np

F = np.float32
U = np.uint32


def row_cells(pos, h, D):
    """sweep_cell: (int)(x / h) per axis, clamped to 0 .. D - 1"""
    q = np.asarray(pos, dtype=F) / F(h)
    assert q.dtype == F
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(q, nan=0.0, posinf=1e9, neginf=-1e9).astype(np.int64), 0, int(D) - 1)


def neighbourhood(cell_ranges, D, cx, cy, cz):
    """stream rows of the 27 cells around (cx, cy, cz), in the order of the walk: dz, dy, dx nesting"""
    runs = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sx, sy, sz = cx + dx, cy + dy, cz + dz
                if min(sx, sy, sz) < 0 or max(sx, sy, sz) >= D:
                    continue
                s, e = cell_ranges[(sz * D + sy) * D + sx]
                runs.append(np.arange(s, e, dtype=np.int64))
    return np.concatenate(runs) if runs else np.zeros(0, np.int64)


def link_r2(h, link):
    """r2 = link * link in fp32; link 0 means h"""
    l = F(h) if F(link) == F(0) else F(link)
    assert np.isfinite(l) and F(0) < l <= F(h), l
    r2 = l * l
    assert type(r2) is F
    return r2


def linked(pa, pb, r2):
    """the link test between every row of pa (m, 3) and every row of pb (k, 3) -> (m, k) bool; a NaN d2 is no link"""
    with np.errstate(all="ignore"):
        e = [pb[None, :, a] - pa[:, None, a] for a in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert d2.dtype == F
    return d2 <= r2


def order_key(b):
    """the diagnostics' ordering key of fp32 bit patterns (section 10c)"""
    b = np.asarray(b, dtype=U)
    return b ^ np.where(b >> U(31), U(0xFFFFFFFF), U(0x80000000)).astype(U)


def links_of(pos, cell_ranges, h, D, r2):
    """every ordered pair (i, j), i != j, of stream rows that the 27-cell walk of row i finds linked: (m, 2) int64"""
    c = row_cells(pos, h, D)
    key = (c[:, 2] * D + c[:, 1]) * D + c[:, 0]
    found = []
    for k in np.unique(key):
        who = np.flatnonzero(key == k)
        cand = neighbourhood(cell_ranges, D, int(k % D), int(k // D % D), int(k // (D * D)))
        if not len(cand):
            continue
        take = linked(pos[who], pos[cand], r2) & (cand[None, :] != who[:, None])
        a, b = np.nonzero(take)
        found.append(np.stack([who[a], cand[b]], axis=1))
    return np.concatenate(found) if found else np.zeros((0, 2), np.int64)


def union_find(n, pairs):
    """sequential union-find (path halving, the smaller root wins) -> the root of every element"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            if ra < rb:
                parent[rb] = ra
            else:
                parent[ra] = rb
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def table_of(pos_by_id, labels):
    """the body table from positions and labels in particle-id order -> ((k, 8) uint32, largest)"""
    bits = np.ascontiguousarray(pos_by_id, dtype=F).view(U).reshape(-1, 3)
    keys = order_key(bits)
    which, inverse, count = np.unique(labels, return_inverse=True, return_counts=True)
    k = len(which)
    table = np.zeros((k, 8), U)
    table[:, 0] = which
    table[:, 1] = count
    lo = np.full((k, 3), 0xFFFFFFFF, U)
    hi = np.zeros((k, 3), U)
    np.minimum.at(lo, inverse, keys)
    np.maximum.at(hi, inverse, keys)
    # a key back to its bit pattern: the key function's inverse
    unkey = lambda q: q ^ np.where(q >> U(31), U(0x80000000), U(0xFFFFFFFF)).astype(U)
    table[:, 2:5] = unkey(lo)
    table[:, 5:8] = unkey(hi)
    largest = int(which[np.argmax(count)]) if k else 0   # (argmax: the first maximum, and the labels ascend)
    return table, largest


def bodies(pos, ids, cell_ranges, h, D, link):
    """pos (n, 3): the SORTED stream, ids (n,): the particle id of every row, cell_ranges (D^3, 2) int32.
    -> {"labels" (n,) uint32 in particle-id order, "table" (k, 8) uint32, "num_bodies", "largest", "links" (unordered
    linked pairs), "degree" (n,) int64 in particle-id order: links of every particle}"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    cell_ranges = np.asarray(cell_ranges, dtype=np.int32).reshape(-1, 2)
    n, D = len(pos), int(D)
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n))
    if n == 0:
        return dict(labels=np.zeros(0, U), table=np.zeros((0, 8), U), num_bodies=0, largest=0, links=0, degree=np.zeros(0, np.int64))
    pairs = links_of(pos, cell_ranges, h, D, link_r2(h, link))
    # the test is bitwise symmetric and so is the walk: every link is found from both of its ends
    fwd = pairs[pairs[:, 0] > pairs[:, 1]]
    bwd = pairs[pairs[:, 0] < pairs[:, 1]][:, ::-1]
    order = lambda p: p[np.lexsort((p[:, 1], p[:, 0]))]
    assert np.array_equal(order(fwd), order(bwd)), "the link graph is not symmetric"
    root = union_find(n, fwd)
    # label: the smallest particle id of the component
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, root, ids)
    labels = np.empty(n, U)
    labels[ids] = smallest[root]
    pos_by_id = np.empty_like(pos)
    pos_by_id[ids] = pos
    degree = np.zeros(n, np.int64)
    np.add.at(degree, ids[pairs[:, 0]], 1)
    table, largest = table_of(pos_by_id, labels)
    return dict(labels=labels, table=table, num_bodies=len(table), largest=largest, links=len(fwd), degree=degree)


def all_pairs_components(pos, h, link):
    """(number of components, component of every particle, unordered links) from the O(n^2) fp32 link matrix: no
    cells, no walk"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    take = linked(pos, pos, link_r2(h, link))
    np.fill_diagonal(take, False)
    assert np.array_equal(take, take.T)
    k, comp = connected_components(csr_matrix(take), directed=False)
    return k, comp, int(take.sum()) // 2
