"""Per-body moments restated with numpy and Python ints, fed with what download_state returns
and the labels of the bodies' restatement.

The terms are np.floor(t * 2.0**32) of float64 arrays, then Python ints, then sum() per label: no accumulator of the
device code, no 128-bit word, no shared line with the HIP or C++ side, and nothing imported from the product.  The
derived values are the expressions of section 10k in Python floats, in the written order."""
import math

import numpy as np

F = np.float32
SUMS = ("x", "y", "z", "vx", "vy", "vz", "rho", "prs", "v2", "xx", "yy", "zz", "xy", "xz", "yz", "lx", "ly", "lz")
INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)
MASS = float(F(0.02))
GAS_CONSTANT, REST_DENSITY = F(1), F(1000)
ROW_DTYPE = np.dtype([("label", "<u4"), ("count", "<u4"), ("saturated", "<u8"), ("sum", "<u8", (18, 2))])
VALUE_FIELDS = ("mass", "com", "velocity", "momentum", "kinetic", "kinetic_internal", "mean_rho", "mean_prs", "covariance",
                "gyration", "angular", "saturated")


def q_terms(t):
    """(q(t) of every entry of the float64 array t as Python ints, bool array: the entry took a special branch):
    NaN -> 0, t >= 2^31 -> INT64_MAX, t < -2^31 -> INT64_MIN, else floor(t 2^32)"""
    t = np.asarray(t, np.float64).reshape(-1)
    nan, top, bottom = np.isnan(t), t >= 2.0**31, t < -(2.0**31)
    special = nan | top | bottom
    q = np.floor(np.where(special, 0.0, t) * 2.0**32).astype(np.int64).tolist()
    for i in np.flatnonzero(top):
        q[i] = INT64_MAX
    for i in np.flatnonzero(bottom):
        q[i] = INT64_MIN
    return q, special


def row_terms(pos, vel, rho):
    """the eighteen float64 terms of every row, by name"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    rho = np.ascontiguousarray(rho, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        prs = np.fmax(F(0), GAS_CONSTANT * (rho - REST_DENSITY))  # fp32, as sph_download_state; fmaxf drops a NaN
        assert prs.dtype == F
        x, y, z = (pos[:, a].astype(np.float64) for a in range(3))
        vx, vy, vz = (vel[:, a].astype(np.float64) for a in range(3))
        t = dict(x=x, y=y, z=z, vx=vx, vy=vy, vz=vz, rho=rho.astype(np.float64), prs=prs.astype(np.float64))
        t["v2"] = (vx * vx + vy * vy) + vz * vz
        t.update(xx=x * x, yy=y * y, zz=z * z, xy=x * y, xz=x * z, yz=y * z)
        t.update(lx=y * vz - z * vy, ly=z * vx - x * vz, lz=x * vy - y * vx)
    return t


def restate(pos, vel, rho, labels):
    """pos, vel, rho and labels in particle-id order -> the list of bodies in ascending label order, each
    dict(label, count, saturated, sums {name: int})"""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    terms = row_terms(pos, vel, rho)
    assert len(labels) == len(terms["x"])
    which, inverse = np.unique(labels, return_inverse=True)
    members = [np.flatnonzero(inverse == k).tolist() for k in range(len(which))]
    bodies = [dict(label=int(l), count=len(m), saturated=0, sums={}) for l, m in zip(which, members)]
    for name in SUMS:
        q, special = q_terms(terms[name])
        for b, m in zip(bodies, members):
            b["sums"][name] = sum(q[i] for i in m)
            b["saturated"] += int(special[m].sum())
    return bodies


def size_hist(bodies):
    """size_hist[b] = the number of bodies with floor(log2(count)) == b"""
    hist = np.zeros(32, np.uint32)
    for b in bodies:
        hist[b["count"].bit_length() - 1] += 1
    return hist


def to_rows(bodies):
    """the restated bodies as raw rows (for byte-for-byte comparisons): low word, high word of the two's complement sum"""
    rows = np.zeros(len(bodies), ROW_DTYPE)
    for r, b in zip(rows, bodies):
        r["label"], r["count"], r["saturated"] = b["label"], b["count"], b["saturated"]
        for k, name in enumerate(SUMS):
            S = b["sums"][name] & (2**128 - 1)
            r["sum"][k] = (S & (2**64 - 1), S >> 64)
    return rows


def from_rows(rows):
    """raw rows back to the list of bodies"""
    out = []
    for r in np.asarray(rows).reshape(-1):
        sums = {}
        for k, name in enumerate(SUMS):
            S = (int(r["sum"][k][1]) << 64) | int(r["sum"][k][0])
            sums[name] = S - 2**128 if S >> 127 else S
        out.append(dict(label=int(r["label"]), count=int(r["count"]), saturated=int(r["saturated"]), sums=sums))
    return out


def values(b):
    """the derived doubles of one body, section 10k's expressions in its order, as Python floats"""
    S = {k: v / 2**32 for k, v in b["sums"].items()}  # (int / int is correctly rounded)
    nd = float(b["count"])
    div = lambda s: s / nd if b["count"] else 0.0
    out = dict(mass=nd * MASS)
    com = out["com"] = tuple(div(S[k]) for k in ("x", "y", "z"))
    v = out["velocity"] = tuple(div(S[k]) for k in ("vx", "vy", "vz"))
    out["momentum"] = tuple(MASS * S[k] for k in ("vx", "vy", "vz"))
    out["kinetic"] = (0.5 * MASS) * S["v2"]
    out["kinetic_internal"] = out["kinetic"] - (0.5 * out["mass"]) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    out["mean_rho"], out["mean_prs"] = div(S["rho"]), div(S["prs"])
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    cov = out["covariance"] = tuple(div(S[k]) - com[a] * com[c] for k, (a, c) in zip(("xx", "yy", "zz", "xy", "xz", "yz"), pairs))
    trace = (cov[0] + cov[1]) + cov[2]
    out["gyration"] = math.sqrt(trace if trace > 0.0 else 0.0)
    c = (com[1] * v[2] - com[2] * v[1], com[2] * v[0] - com[0] * v[2], com[0] * v[1] - com[1] * v[0])
    out["angular"] = tuple(MASS * (S[k] - nd * c[a]) for a, k in enumerate(("lx", "ly", "lz")))
    out["saturated"] = b["saturated"]
    return out


def describe_difference(got, want):
    """which words of two arrays of raw rows differ (for assertion messages)"""
    if len(got) != len(want):
        return f"{len(got)} rows, not {len(want)}"
    out = []
    for g, w in zip(from_rows(got), from_rows(want)):
        for f in ("label", "count", "saturated"):
            if g[f] != w[f]:
                out.append(f"body {w['label']}: {f} {g[f]} vs {w[f]}")
        out += [f"body {w['label']}: sum {k} {g['sums'][k]} vs {w['sums'][k]}" for k in SUMS if g["sums"][k] != w["sums"][k]]
    return f"{len(out)} words differ; " + "; ".join(out[:6])


def assert_same_rows(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == ROW_DTYPE, (got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), f"{what}: {describe_difference(got, want)}"
