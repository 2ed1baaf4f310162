"""The pair statistics ("Pair statistics") restated in numpy and plain Python, twice.

all_pairs(): every pair of particles tested, in chunks of rows; no grid, no walk.  The fp32 steps are np.float32 ufunc
calls one at a time, the fp64 terms np.float64 ufunc calls one at a time (numpy fuses nothing), q(t) and the sums are
Python ints.

from_lists(): the same statistics through the neighbour lists of neighbour_restatement.all_pairs, filtered to j > i --
and with the roles swapped, the row the greater id: the definition says every term is the same word either way.

edges2() restates sph_pair_edges, values() sph_pair_values.  Imports nothing from the product."""
import math

import numpy as np

import neighbour_restatement as NR

F = np.float32
D = np.float64
SUMS = ("d2", "w2", "a", "l2")
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
ROW_DTYPE = np.dtype([("pairs", "<u8"), ("sums", "<u8", (4, 2)), ("saturated", "<u8")])
VALUE_FIELDS = ("r_lo", "r_hi", "pairs", "mean_r2", "s2", "s2_par", "approach", "g", "saturated")


def radius_of(h, radius):
    r = F(h) if F(radius) == F(0) else F(radius)
    assert np.isfinite(r) and F(0) < r <= F(h), r
    return r


def edges2(radius, h, bins):
    """sph_pair_edges: (B,) float32; bins 0 means 32"""
    r = radius_of(h, radius)
    B = int(bins) if bins else 32
    assert 1 <= B <= 128
    out = np.empty(B, F)
    for k in range(B):
        t = (float(r) * float(k + 1)) / float(B)
        out[k] = F(t * t)          # (a Python float to float32: one rounding to nearest even)
    r2 = r * r
    assert type(r2) is F
    out[B - 1] = r2
    return out


def bins_of(d2, edges):
    """the number of k < B - 1 with edges[k] < d2, for every d2"""
    d2 = np.asarray(d2, F).reshape(-1)
    return (edges[None, :len(edges) - 1] < d2[:, None]).sum(axis=1).astype(np.int64)


def q_terms(t):
    """q(t) of every entry of the float64 array t as Python ints, and which took one of the three special branches"""
    t = np.asarray(t, D).reshape(-1)
    nan, top, bottom = np.isnan(t), t >= 2.0**31, t < -(2.0**31)
    special = nan | top | bottom
    q = [0 if s else math.floor(x * 4294967296.0) for x, s in zip(t.tolist(), special.tolist())]
    for i in np.flatnonzero(top):
        q[i] = INT64_MAX
    for i in np.flatnonzero(bottom):
        q[i] = INT64_MIN
    return q, special


def pair_terms(pos, vel, rows, cands):
    """the definition for the pairs (rows[k], cands[k]): e = p_cand - p_row, w = v_cand - v_row in fp32, then fp64
    -> (d2 (m,) float32, [four (m,) float64 arrays: d2, w2, a, l2])"""
    with np.errstate(all="ignore"):
        e = [pos[cands, a] - pos[rows, a] for a in range(3)]
        w = [vel[cands, a] - vel[rows, a] for a in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert d2.dtype == F and w[0].dtype == F
        ex, ey, ez = (x.astype(D) for x in e)
        wx, wy, wz = (x.astype(D) for x in w)
        w2 = (wx * wx + wy * wy) + wz * wz
        a = (ex * wx + ey * wy) + ez * wz
        d = d2.astype(D)
        l2 = np.where(d2 == F(0), D(0), (a * a) / np.where(d2 == F(0), D(1), d))
    return d2, [d, w2, a, l2]


class Pairs:
    """the taken pairs (rows[k], cands[k]) with their d2 and their four lists of q terms: binned by table()"""

    def __init__(self, pos, vel, rows, cands):
        self.d2, terms = pair_terms(pos, vel, rows, cands)
        self.q, self.special = [], []
        for t in terms:
            q, special = q_terms(t)
            self.q.append(np.array(q, np.int64))   # (every q fits 64 bits; they are summed as Python ints)
            self.special.append(special)

    def table(self, edges):
        B = len(edges)
        which = bins_of(self.d2, edges)
        sums = np.empty((B, 4), object)
        saturated = np.zeros(B, np.uint64)
        for b in range(B):
            mine = np.flatnonzero(which == b)
            for s in range(4):
                sums[b, s] = sum(self.q[s][mine].tolist())
                saturated[b] += np.uint64(int(self.special[s][mine].sum()))
        return dict(pairs=np.bincount(which, minlength=B).astype(np.uint64), sums=sums, saturated=saturated, edges2=edges)


def table_of(pos, vel, rows, cands, edges):
    """the table of the pairs (rows[k], cands[k]) over the bins of `edges`"""
    return Pairs(pos, vel, rows, cands).table(edges)


def taken_pairs(pos, r2, chunk=512):
    """every pair (i, j), i < j, with d2 <= r2: all pairs tested, no grid"""
    n = len(pos)
    everyone = np.arange(n)
    I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for k in range(0, n, chunk):
        with np.errstate(all="ignore"):
            e = [pos[None, :, a] - pos[k:k + chunk, None, a] for a in range(3)]
            d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert d2.dtype == F
        take = (d2 <= r2) & (everyone[None, :] > everyone[k:k + chunk, None])   # (a NaN d2 compares false)
        i, j = np.nonzero(take)
        I.append(i + k)
        J.append(j)
    return np.concatenate(I), np.concatenate(J)


def prepared(pos, vel, h, radius=0.0):
    """restatement (a) up to the binning: .table(edges2(radius, h, bins)) for any number of bins"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    r = radius_of(h, radius)
    I, J = taken_pairs(pos, r * r)
    return Pairs(pos, vel, I, J)


def all_pairs(pos, vel, h, radius=0.0, bins=0):
    """restatement (a): pos, vel (n, 3) in particle-id order"""
    return prepared(pos, vel, h, radius).table(edges2(radius, h, bins))


def from_lists(pos, vel, h, radius=0.0, bins=0):
    """restatement (b): the neighbour lists' pairs with j > i, the row the GREATER id"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    lists = NR.lists_of(*NR.all_pairs(pos, h, radius))
    I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for i, l in enumerate(lists):
        greater = l[l > i].astype(np.int64)
        I.append(np.full(len(greater), i, np.int64))
        J.append(greater)
    return table_of(pos, vel, np.concatenate(J), np.concatenate(I), edges2(radius, h, bins))


def to_rows(t):
    """a table as raw rows (ROW_DTYPE): every sum as its low and high 64-bit words, two's complement"""
    B = len(t["pairs"])
    rows = np.zeros(B, ROW_DTYPE)
    rows["pairs"] = t["pairs"]
    rows["saturated"] = t["saturated"]
    for k in range(B):
        for s in range(4):
            u = int(t["sums"][k, s]) % (1 << 128)
            rows["sums"][k, s] = (u & ((1 << 64) - 1), u >> 64)
    return rows


def from_rows(rows, edges):
    rows = np.asarray(rows, ROW_DTYPE).reshape(-1)
    sums = np.empty((len(rows), 4), object)
    for k in range(len(rows)):
        for s in range(4):
            u = int(rows["sums"][k, s, 0]) | (int(rows["sums"][k, s, 1]) << 64)
            sums[k, s] = u - (1 << 128) if u >> 127 else u
    return dict(pairs=rows["pairs"].copy(), sums=sums, saturated=rows["saturated"].copy(), edges2=np.asarray(edges, F))


def values(t, box, n):
    """sph_pair_values in Python floats: a list of dicts, one per bin"""
    edges = t["edges2"]
    assert not np.isnan(edges).any() and (np.diff(edges.astype(D)) >= 0).all()
    nd = float(n)
    couples = (nd * (nd - 1.0)) / 2.0
    box = float(F(box))
    volume = (box * box) * box
    out = []
    for k in range(len(edges)):
        r_lo = math.sqrt(float(edges[k - 1])) if k else 0.0
        r_hi = math.sqrt(float(edges[k]))
        pairs = float(int(t["pairs"][k]))
        mean = lambda s: (int(t["sums"][k, s]) / 2**32) / pairs if pairs else 0.0
        shell = ((4.0 * math.pi) / 3.0) * ((r_hi * r_hi) * r_hi - (r_lo * r_lo) * r_lo)
        ideal = (couples * shell) / volume
        out.append(dict(r_lo=r_lo, r_hi=r_hi, pairs=pairs, mean_r2=mean(0), s2=mean(1), s2_par=mean(3), approach=mean(2),
                        g=pairs / ideal if ideal > 0.0 else 0.0, saturated=int(t["saturated"][k])))
    return out


def describe_difference(got, want):
    lines = []
    if not np.array_equal(got["edges2"].view(np.uint32), want["edges2"].view(np.uint32)):
        lines.append(f"edges2 differ: {got['edges2']} vs {want['edges2']}")
        return lines
    for k in range(len(want["pairs"])):
        if int(got["pairs"][k]) != int(want["pairs"][k]):
            lines.append(f"bin {k}: pairs {int(got['pairs'][k])} vs {int(want['pairs'][k])}")
        if int(got["saturated"][k]) != int(want["saturated"][k]):
            lines.append(f"bin {k}: saturated {int(got['saturated'][k])} vs {int(want['saturated'][k])}")
        for s, name in enumerate(SUMS):
            if int(got["sums"][k, s]) != int(want["sums"][k, s]):
                lines.append(f"bin {k}: sum {name} {int(got['sums'][k, s])} vs {int(want['sums'][k, s])}")
    return lines


def assert_same_table(got, want, what):
    """got, want: dicts with pairs, sums (Python ints), saturated, edges2"""
    assert len(got["pairs"]) == len(want["pairs"]) == len(got["edges2"]) == len(want["edges2"]), what
    lines = describe_difference(got, want)
    assert not lines, f"{what}: {len(lines)} differences, the first: " + "; ".join(lines[:4])
