"""Run diagnostics restated with numpy and Python ints, fed with what download_state returns.

The terms are np.floor(t * 2.0**32) as int64, then Python ints, then sum(): no accumulator of the device code, no
128-bit word, no shared line with the HIP or C++ side.  The histogram's bin is the field frame's q
(field_frame_restatement.quantise).  The derived values are the expressions of section 10c in Python floats."""
import ctypes as C

import numpy as np

import field_frame_restatement as FF

F = np.float32
SUMS = ("x", "y", "z", "vx", "vy", "vz", "rho", "prs", "v2")
EXTREMA = ("x", "y", "z", "speed", "rho", "prs")
FIELDS = {"speed": 0, "density": 1, "pressure": 2}
EXT_OF_FIELD = {"speed": "speed", "density": "rho", "pressure": "prs"}
INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)
MIN_IDENTITY, MAX_IDENTITY = 0x7F800000, 0xFF800000  # the extrema of no rows
MASS = float(F(0.02))
MINUS_GRAVITY = float(F(9.8))
GAS_CONSTANT, REST_DENSITY = F(1), F(1000)


def q_terms(t):
    """(terms, saturated): q(t) of every entry of the float64 array t as a list of Python ints, and how many took
    one of the three special branches (NaN -> 0, t >= 2^31 -> INT64_MAX, t < -2^31 -> INT64_MIN)"""
    t = np.asarray(t, np.float64).reshape(-1)
    nan, top, bottom = np.isnan(t), t >= 2.0**31, t < -(2.0**31)
    special = nan | top | bottom
    q = np.floor(np.where(special, 0.0, t) * 2.0**32).astype(np.int64).tolist()
    for i in np.flatnonzero(top):
        q[i] = INT64_MAX
    for i in np.flatnonzero(bottom):
        q[i] = INT64_MIN
    return q, int(special.sum())


def key(bits):
    """the ordering key of fp32 bit patterns: b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000)"""
    b = np.asarray(bits, np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def extrema(values):
    """(min bits, max bits) of an fp32 array by the key; the identities for no rows"""
    b = np.ascontiguousarray(values, dtype=F).view(np.uint32).reshape(-1)
    if not len(b):
        return MIN_IDENTITY, MAX_IDENTITY
    k = key(b)
    return int(b[np.argmin(k)]), int(b[np.argmax(k)])


def columns(pos, vel, rho):
    """the fp32 columns of the rows: x, y, z, vx, vy, vz, rho and the two derived scalars speed and prs"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    rho = np.ascontiguousarray(rho, dtype=F).reshape(-1)
    c = dict(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2], vx=vel[:, 0], vy=vel[:, 1], vz=vel[:, 2], rho=rho)
    with np.errstate(all="ignore"):
        c["speed"] = np.sqrt((c["vx"] * c["vx"] + c["vy"] * c["vy"]) + c["vz"] * c["vz"])
        c["prs"] = np.fmax(F(0), GAS_CONSTANT * (rho - REST_DENSITY))  # fmaxf: a NaN gives the other operand
    assert all(v.dtype == F for v in c.values())
    return c


def restate(pos, vel, rho, hist=None, value_range=None):
    """the words of sph_diagnose for these rows: dict(n, sums {name: int}, min_bits / max_bits {name: int},
    saturated, hist_field, hist_lo_bits, hist_hi_bits, hist (256 np.uint64))"""
    c = columns(pos, vel, rho)
    n = len(c["x"])
    d = dict(n=n, sums={}, min_bits={}, max_bits={}, saturated=0)
    with np.errstate(all="ignore"):
        vx, vy, vz = (c[k].astype(np.float64) for k in ("vx", "vy", "vz"))
        terms = {k: c[k].astype(np.float64) for k in SUMS[:8]}
        terms["v2"] = (vx * vx + vy * vy) + vz * vz
    for name in SUMS:
        q, sat = q_terms(terms[name])
        d["sums"][name] = sum(q)
        d["saturated"] += sat
    for name in EXTREMA:
        d["min_bits"][name], d["max_bits"][name] = extrema(c[name])
    d["hist_field"] = -1 if hist is None else FIELDS[hist]
    d["hist_lo_bits"] = d["hist_hi_bits"] = 0
    d["hist"] = np.zeros(256, np.uint64)
    if hist is not None:
        s = c[EXT_OF_FIELD[hist]]
        lo, hi = (F(0), F(0)) if value_range is None else (F(value_range[0]), F(value_range[1]))
        if lo == 0 and hi == 0:  # automatic: the extrema of the scalar over these rows
            e = EXT_OF_FIELD[hist]
            lo, hi = np.array([d["min_bits"][e], d["max_bits"][e]], np.uint32).view(F)
        d["hist_lo_bits"], d["hist_hi_bits"] = (int(v) for v in np.array([lo, hi], F).view(np.uint32))
        if n:
            d["hist"] = np.bincount(FF.quantise(s, lo, hi), minlength=256).astype(np.uint64)
    return d


def value(S):
    """value(S) = S 2^-32, rounded once (Python's int / int is correctly rounded)"""
    return S / 2**32


def values(d, settings):
    """the derived doubles of section 10c, in its order, as Python floats"""
    n = d["n"]
    v = {k: value(S) for k, S in d["sums"].items()}
    as_float = lambda bits: float(np.array([bits], np.uint32).view(F)[0])
    out = dict(n=n, mass=n * MASS)
    out["com"] = tuple(v[k] / n if n else 0.0 for k in ("x", "y", "z"))
    out["momentum"] = tuple(MASS * v[k] for k in ("vx", "vy", "vz"))
    out["kinetic"] = 0.5 * MASS * v["v2"]
    out["potential"] = MASS * MINUS_GRAVITY * v["y"]
    out["mean_rho"] = v["rho"] / n if n else 0.0
    out["mean_prs"] = v["prs"] / n if n else 0.0
    out["min_rho"], out["max_rho"] = as_float(d["min_bits"]["rho"]), as_float(d["max_bits"]["rho"])
    out["max_speed"] = as_float(d["max_bits"]["speed"])
    out["cfl"] = out["max_speed"] * float(F(settings.timestep)) / float(F(settings.h))
    out["box_min"] = tuple(as_float(d["min_bits"][k]) for k in ("x", "y", "z"))
    out["box_max"] = tuple(as_float(d["max_bits"][k]) for k in ("x", "y", "z"))
    out["saturated"] = d["saturated"]
    return out


def to_struct(d):
    """the restated words as the library's SphDiagnosticsRaw (for byte-for-byte comparisons)"""
    from cudafluidsimulator_amd import _lib
    r = _lib.SphDiagnosticsRaw()
    r.struct_size = C.sizeof(_lib.SphDiagnosticsRaw)
    r.n = d["n"]
    for k, name in enumerate(SUMS):
        S = d["sums"][name]
        r.sum[k].lo = S & (2**64 - 1)
        r.sum[k].hi = S >> 64  # (arithmetic: the sign lives here)
    for k, name in enumerate(EXTREMA):
        r.min_bits[k], r.max_bits[k] = d["min_bits"][name], d["max_bits"][name]
    r.saturated = d["saturated"]
    r.hist_field, r.hist_lo_bits, r.hist_hi_bits = d["hist_field"], d["hist_lo_bits"], d["hist_hi_bits"]
    for k in range(256):
        r.hist[k] = int(d["hist"][k])
    return r


def describe_difference(got, want):
    """which words of two SphDiagnosticsRaw differ (for assertion messages)"""
    out = []
    for k, name in enumerate(SUMS):
        a, b = ((s.sum[k].hi << 64) | s.sum[k].lo for s in (got, want))
        if a != b:
            out.append(f"sum {name}: {a} vs {b}")
    for k, name in enumerate(EXTREMA):
        if got.min_bits[k] != want.min_bits[k]:
            out.append(f"min {name}: {got.min_bits[k]:#x} vs {want.min_bits[k]:#x}")
        if got.max_bits[k] != want.max_bits[k]:
            out.append(f"max {name}: {got.max_bits[k]:#x} vs {want.max_bits[k]:#x}")
    for f in ("n", "saturated", "hist_field", "hist_lo_bits", "hist_hi_bits", "struct_size", "pad_", "pad2_"):
        if getattr(got, f) != getattr(want, f):
            out.append(f"{f}: {getattr(got, f)} vs {getattr(want, f)}")
    bad = [k for k in range(256) if got.hist[k] != want.hist[k]]
    if bad:
        out.append(f"hist: {len(bad)} bins differ, first {bad[0]}: {got.hist[bad[0]]} vs {want.hist[bad[0]]}")
    return "; ".join(out) or "(padding bytes)"


def assert_same_words(got, want, what):
    assert bytes(got) == bytes(want), f"{what}: {describe_difference(got, want)}"
