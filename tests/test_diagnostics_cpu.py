"""Run diagnostics without a GPU: hand-derived known answers of the restatement (tests/diagnostics_restatement.py),
the two pure host functions sph_diagnostics_values / sph_diagnostics_add through ctypes held against it -- words
byte for byte, doubles with == --, the struct layouts, and the same two functions under the host sanitizers in a
stand-alone program (tests/diagnostics_selftest.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import diagnostics_restatement as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SPH_EINVAL = -1


def settings():
    return sph.default_settings(1000, True)


# ---- the restatement's own known answers, derived by hand ----

def test_q_known_answers():
    q, sat = D.q_terms([-(2.0**-33), 1.5, 2.0**31, np.nan, -(2.0**31), -(2.0**31) - 1.0, 0.0, -0.0, 2.0**-32])
    assert q == [-1, 3 * 2**31, D.INT64_MAX, 0, -(2**63), D.INT64_MIN, 0, 0, 1]
    assert sat == 3  # 2^31, the NaN, and the one below -2^31; -2^31 itself is in range: floor(-2^31 2^32) = INT64_MIN exactly


def test_three_rows_by_hand():
    vel = np.array([[3, 4, 0], [-3, -4, 0], [0, 0, -0.5]], F)
    d = D.restate(np.full((3, 3), 5, F), vel, np.full(3, 1000, F))
    assert d["sums"]["v2"] == int(50.25 * 2**32) == 201 * 2**30
    assert d["sums"]["vx"] == 0 and d["sums"]["vy"] == 0
    assert d["sums"]["vz"] == -(2**31)
    assert d["sums"]["x"] == 15 * 2**32 and d["sums"]["rho"] == 3000 * 2**32 and d["sums"]["prs"] == 0
    assert d["saturated"] == 0 and d["n"] == 3
    assert d["max_bits"]["speed"] == int(F(5).view(np.uint32)) and d["min_bits"]["speed"] == int(F(0.5).view(np.uint32))
    v = D.values(d, settings())
    assert v["kinetic"] == 0.5 * D.MASS * 50.25 and v["momentum"] == (0.0, 0.0, D.MASS * -0.5)
    assert v["com"] == (5.0, 5.0, 5.0) and v["max_speed"] == 5.0 and v["mass"] == 3 * D.MASS


def test_key_order_and_the_identities():
    bits = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], F).view(np.uint32)
    k = D.key(bits)
    assert k[1] < k[0], "-0 < +0"
    assert list(np.argsort(k)) == [5, 3, 1, 0, 2, 4]
    nan_pos, nan_neg = np.uint32(0x7FC00000), np.uint32(0xFFC00000)
    assert D.key(nan_pos) > k[4] and D.key(nan_neg) < k[5], "a NaN sorts where its bits put it"
    assert D.extrema(np.array([0.0, -0.0], F)) == (0x80000000, 0x00000000)
    d = D.restate(np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F), hist="speed")
    assert all(S == 0 for S in d["sums"].values()) and d["saturated"] == 0
    assert set(d["min_bits"].values()) == {0x7F800000} and set(d["max_bits"].values()) == {0xFF800000}
    assert (d["hist_lo_bits"], d["hist_hi_bits"]) == (0x7F800000, 0xFF800000) and not d["hist"].any()
    v = D.values(d, settings())
    assert v["com"] == (0.0, 0.0, 0.0) and v["mean_rho"] == 0.0 and v["mean_prs"] == 0.0 and v["mass"] == 0.0


# ---- the library's pure host functions against the restatement ----

def seeded_state(n=1000, seed=7):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.1, 9.9, (n, 3)).astype(F)
    vel = (rng.uniform(-3, 3, (n, 3)) * rng.choice([1.0, 2.0**-30, 1e-3], (n, 1))).astype(F)
    vel[17] = (1e6, -2.5, 0.125)  # v2 = 1e12 + ... >= 2^31: one saturating term
    rho = rng.uniform(900, 1100, n).astype(F)
    return pos, vel, rho


def lib_values(raw, s):
    out = _lib.SphDiagnostics()
    assert sph.load_library().sph_diagnostics_values(C.byref(raw), C.byref(s), C.byref(out)) == 0
    return out


@pytest.mark.parametrize("hist", [None, ("density", (950.0, 1050.0))])
def test_add_merges_parts_into_the_whole_byte_for_byte(hist):
    L = sph.load_library()
    pos, vel, rho = seeded_state()
    kw = dict(hist=hist[0], value_range=hist[1]) if hist else {}
    whole = D.restate(pos, vel, rho, **kw)
    assert whole["saturated"] == 1 and whole["sums"]["vx"] != 0 and min(whole["sums"].values()) < 0
    want = D.to_struct(whole)
    for cuts in [(1, 333, 999), (0, 500, 1000), (17, 18, 640)]:  # (an empty part at either end included)
        edges = (0,) + cuts + (1000,)
        parts = [D.to_struct(D.restate(pos[a:b], vel[a:b], rho[a:b], **kw)) for a, b in zip(edges[:-1], edges[1:])]
        for order in (parts, parts[::-1]):
            got = _lib.SphDiagnosticsRaw.from_buffer_copy(bytes(order[0]))
            for p in order[1:]:
                assert L.sph_diagnostics_add(C.byref(got), C.byref(p)) == 0
            D.assert_same_words(got, want, f"parts cut at {cuts}")
    if hist:
        assert int(want.hist[0]) > 0 and int(want.hist[255]) > 0 and sum(want.hist) == 1000


def test_add_refuses_histograms_that_do_not_match():
    L = sph.load_library()
    pos, vel, rho = seeded_state(100)
    a = D.to_struct(D.restate(pos, vel, rho, hist="speed", value_range=(0.0, 2.0)))
    for other in (D.restate(pos, vel, rho), D.restate(pos, vel, rho, hist="density", value_range=(0.0, 2.0)),
                  D.restate(pos, vel, rho, hist="speed", value_range=(0.0, 3.0)),
                  D.restate(pos[:50], vel[:50], rho[:50], hist="speed")):  # (its own automatic range)
        b = D.to_struct(other)
        before = bytes(a)
        assert L.sph_diagnostics_add(C.byref(a), C.byref(b)) == SPH_EINVAL
        assert bytes(a) == before
    assert L.sph_diagnostics_add(None, C.byref(a)) == SPH_EINVAL and L.sph_diagnostics_add(C.byref(a), None) == SPH_EINVAL


def test_values_equal_the_python_expressions():
    s = settings()
    pos, vel, rho = seeded_state()
    for sl in (slice(0, 1000), slice(0, 1), slice(17, 18), slice(0, 0), slice(100, 900)):
        d = D.restate(pos[sl], vel[sl], rho[sl])
        got, want = lib_values(D.to_struct(d), s), D.values(d, s)
        for name, w in want.items():
            g = getattr(got, name)
            g = tuple(g) if isinstance(w, tuple) else g
            assert g == w, f"{name} of rows {sl}: {g!r} vs {w!r}"
        assert got.struct_size == C.sizeof(_lib.SphDiagnostics)
    assert sph.load_library().sph_diagnostics_values(None, C.byref(s), C.byref(_lib.SphDiagnostics())) == SPH_EINVAL


def test_a_128_bit_carry_by_repeated_add():
    L = sph.load_library()
    one = dict(D.restate(np.full((1, 3), 5, F), np.zeros((1, 3), F), np.full(1, 1000, F)))
    one["sums"] = {k: D.INT64_MAX for k in D.SUMS}
    acc = D.to_struct(one)
    for _ in range(20):  # doubling: 2^20 terms
        copy = _lib.SphDiagnosticsRaw.from_buffer_copy(bytes(acc))
        assert L.sph_diagnostics_add(C.byref(acc), C.byref(copy)) == 0
    total = D.INT64_MAX * 2**20
    assert total >= 2**64
    for k in range(9):
        assert (acc.sum[k].hi << 64) | acc.sum[k].lo == total
    assert acc.n == 2**20
    got = lib_values(acc, settings())
    assert got.kinetic == 0.5 * D.MASS * (total / 2**32)
    assert got.com[0] == (total / 2**32) / 2**20


def test_python_front_end_without_a_gpu():
    pos, vel, rho = seeded_state()
    d = D.restate(pos, vel, rho, hist="density", value_range=(950.0, 1050.0))
    out = _lib.diagnostics_dict(D.to_struct(d), settings())
    want = D.values(d, settings())
    for name in ("kinetic", "potential", "momentum", "com", "max_speed", "cfl", "mean_rho", "saturated"):
        assert out[name] == want[name], name
    raw = out["raw"]
    assert raw["sums"] == d["sums"] and raw["saturated"] == 1 and raw["n"] == 1000
    assert raw["hist"].dtype == np.uint64 and (raw["hist"] == d["hist"]).all()
    assert raw["max"]["speed"].dtype == F and raw["max"]["speed"].view(np.uint32) == d["max_bits"]["speed"]
    assert raw["hist_range"] == (F(950), F(1050))


# ---- layouts and the stand-alone sanitizer run ----

@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/diagnostics_selftest.cpp + csrc/sph_diag_values.cpp under ASan + UBSan, run once: {name: [values]}"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("diag") / "diagnostics_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "diagnostics_selftest.cpp"),
                    os.path.join(ROOT, "cudafluidsimulator_amd", "csrc", "sph_diag_values.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and not p.stderr, f"sanitizer report or failure:\n{p.stderr}"
    out = {}
    for line in p.stdout.splitlines():
        name, val = line.split()
        out.setdefault(name, []).append(val)
    return out


def test_struct_sizes_and_offsets_match_the_ctypes_mirrors(selftest):
    one = lambda name: int(selftest[name][0])
    assert one("sizeof_options") == C.sizeof(_lib.SphDiagnosticsOptions) == 16
    assert one("sizeof_sum128") == C.sizeof(_lib.SphSum128) == 16
    assert one("sizeof_raw") == C.sizeof(_lib.SphDiagnosticsRaw) == 2280
    assert one("sizeof_values") == C.sizeof(_lib.SphDiagnostics)
    for f in ("n", "sum", "min_bits", "max_bits", "saturated", "hist_field", "hist_lo_bits", "hist_hi_bits", "hist"):
        assert one("raw_" + f) == getattr(_lib.SphDiagnosticsRaw, f).offset, f
    for f, _ in _lib.SphDiagnostics._fields_[2:]:
        assert one("values_" + f) == getattr(_lib.SphDiagnostics, f).offset, f


def test_host_functions_under_the_sanitizers(selftest):
    h = lambda name: float.fromhex(selftest[name][0])
    words = lambda tag: (int(selftest[tag + "_sum_hi"][0]) << 64) | int(selftest[tag + "_sum_lo"][0])
    dt, hh = float(F(0.004)), float(F(0.1))
    cases = dict(carry=(D.INT64_MAX * 2**20, 2**20, 3.0), neg=(-3, 3, -1.0), low=(D.INT64_MIN * 2**20, 2**20, 1.0),
                 tie_down=(2**53 + 1, 1, 1.0), tie_up=(2**53 + 3, 1, 1.0), empty=(0, 0, None))
    for tag, (S, n, speed) in cases.items():
        assert selftest[tag + "_rc"] == ["0"]
        assert words(tag) == S, tag
        v = S / 2**32
        assert h(tag + "_kinetic") == 0.5 * D.MASS * v, tag
        assert h(tag + "_potential") == D.MASS * D.MINUS_GRAVITY * v, tag
        assert h(tag + "_momentum_x") == D.MASS * v, tag
        assert h(tag + "_com_x") == (v / n if n else 0.0), tag
        assert h(tag + "_mass") == n * D.MASS, tag
        if speed is not None:
            assert h(tag + "_cfl") == speed * dt / hh, tag
    assert float(2**53 + 1) / 2**32 == 2.0**21 and (2**53 + 3) / 2**32 == (2.0**53 + 4) / 2**32  # the two ties
    assert selftest["carry_add_rc"] == ["0"] * 20 and selftest["carry_n"] == [str(2**20)]
    assert selftest["empty_add_rc"] == ["0"] and selftest["empty_then_bytes_equal"] == ["1"]
    assert selftest["field_mismatch_rc"] == selftest["range_mismatch_rc"] == selftest["null_rc"] == [str(SPH_EINVAL)]
