"""Per-body moments without a GPU: hand answers of the restatement
(tests/body_moments_restatement.py) where everything is exact, its first nine sums against the diagnostics'
restatement, sph_body_values through ctypes against the Python floats with ==, the struct layouts, the same function
under the host sanitizers in a stand-alone program (tests/body_moments_selftest.cpp), and the properties of the shared
states that tests/test_gpu_body_moments.py relies on."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import body_moments_restatement as M
import body_states as BS
import diagnostics_restatement as D
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SPH_EINVAL = -1
_cache = {}


def settings():
    return sph.default_settings(1000, True)


def one_body(pos, vel, rho=None):
    pos, vel = np.asarray(pos, F), np.asarray(vel, F)
    rho = np.full(len(pos), 1000, F) if rho is None else rho
    (b,) = M.restate(pos, vel, rho, np.zeros(len(pos), np.int64))
    v = M.values(b)
    assert_values_equal(_lib.body_values(M.to_rows([b]), settings())[0], v, "sph_body_values")  # (the library says the same)
    return b, v


# ---- hand answers: dyadic coordinates and velocities, every term and every sum exact ----

def test_four_particles_translating_together_have_no_internal_energy_and_no_spin():
    pos = np.array([[1, 1, 1], [1.0625, 1, 1], [1, 1.0625, 1], [1, 1, 1.0625]], F)
    assert BR.linked(pos, pos, BR.link_r2(0.1, 0.0)).all(), "all within a link of each other: one body"
    vel = np.tile(np.array([0.5, -0.25, 2.0], F), (4, 1))
    b, v = one_body(pos, vel)
    assert b["count"] == 4 and b["saturated"] == 0
    assert b["sums"]["x"] == int(4.0625 * 2**32) and b["sums"]["vz"] == 8 * 2**32 and b["sums"]["v2"] == int(17.25 * 2**32)
    assert b["sums"]["xx"] == int((3 + 1.0625**2) * 2**32) and b["sums"]["xy"] == int(4.125 * 2**32)
    assert v["velocity"] == (0.5, -0.25, 2.0) and v["com"] == (1.015625, 1.015625, 1.015625)
    assert v["momentum"] == (M.MASS * 2.0, M.MASS * -1.0, M.MASS * 8.0) and v["mass"] == 4 * M.MASS
    assert v["kinetic"] == (0.5 * M.MASS) * 17.25
    assert v["kinetic_internal"] == 0.0 and v["angular"] == (0.0, 0.0, 0.0)
    assert v["covariance"][0] == (3 + 1.0625**2) / 4 - 1.015625**2 == 3 * 0.015625**2
    assert v["covariance"][3] == 4.125 / 4 - 1.015625**2 == -(0.015625**2)


def test_a_square_rotating_about_its_centre():
    r = np.array([[0.5, 0.5, 0], [-0.5, 0.5, 0], [-0.5, -0.5, 0], [0.5, -0.5, 0]], F)
    pos = (r + F(2)).astype(F)
    vel = np.stack([-r[:, 1], r[:, 0], r[:, 2]], axis=1).astype(F)  # omega = (0, 0, 1)
    b, v = one_body(pos, vel)
    assert b["sums"]["vx"] == b["sums"]["vy"] == b["sums"]["vz"] == 0 and b["sums"]["v2"] == 2 * 2**32
    assert b["sums"]["lz"] == 2 * 2**32 and b["sums"]["lx"] == b["sums"]["ly"] == 0
    assert v["momentum"] == (0.0, 0.0, 0.0) and v["velocity"] == (0.0, 0.0, 0.0)
    assert v["angular"] == (0.0, 0.0, M.MASS * 2.0)
    assert v["kinetic"] == (0.5 * M.MASS) * 2.0 and v["kinetic_internal"] == v["kinetic"]
    assert v["covariance"] == (0.25, 0.25, 0.0, 0.0, 0.0, 0.0) and v["gyration"] == math.sqrt(0.5)


def test_a_term_below_one_unit_floors_to_minus_one_through_a_bodys_sum():
    pos = np.array([[1, 1, 1], [1.0625, 1, 1], [3, 3, 3]], F)
    vel = np.array([[-(2.0**-33), 0, 0], [0, 0, 0], [1, 0, 0]], F)
    a, c = M.restate(pos, vel, np.full(3, 1000, F), [0, 0, 2])
    assert a["sums"]["vx"] == -1 and a["count"] == 2 and c["sums"]["vx"] == 2**32 and c["label"] == 2
    assert M.values(a)["momentum"][0] == M.MASS * -(2.0**-32) == _lib.body_values(M.to_rows([a, c]), settings())["momentum"][0, 0]
    q, special = M.q_terms([-(2.0**-33), 2.0**31, np.nan, -(2.0**31), -(2.0**31) - 1.0])
    assert q == [-1, M.INT64_MAX, 0, -(2**63), M.INT64_MIN] and special.tolist() == [False, True, True, False, True]


# ---- the restatement's first nine sums are the diagnostics' ----

def seeded(n=1000, seed=7, nan=False):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.1, 9.9, (n, 3)).astype(F)
    vel = (rng.uniform(-3, 3, (n, 3)) * rng.choice([1.0, 2.0**-30, 1e-3], (n, 1))).astype(F)
    vel[17] = (1e6, -2.5, 0.125)  # v2 = 1e12 + ... >= 2^31: one saturating term, and none among the moments' nine
    if nan:
        vel[n // 3, 1] = np.nan
        vel[n // 4] = (-(2.0**31), np.inf, -np.inf)
    rho = rng.uniform(900, 1100, n).astype(F)
    labels = rng.integers(0, 40, n)
    return pos, vel, rho, labels


def test_the_first_nine_sums_over_all_bodies_are_the_diagnostics():
    pos, vel, rho, labels = seeded()
    bodies = M.restate(pos, vel, rho, labels)
    d = D.restate(pos, vel, rho)
    assert len(bodies) == 40 and sum(b["count"] for b in bodies) == 1000
    for name in D.SUMS:
        assert sum(b["sums"][name] for b in bodies) == d["sums"][name], name
    assert sum(b["saturated"] for b in bodies) == d["saturated"] == 1 == int(_lib.body_values(M.to_rows(bodies), settings())["saturated"].sum())
    # with NaN and infinite velocities the angular terms take the special branches too: the nine sums still agree, and
    # the diagnostics' count is the part of the bodies' that lies in the first nine
    pos, vel, rho, labels = seeded(nan=True)
    bodies = M.restate(pos, vel, rho, labels)
    d = D.restate(pos, vel, rho)
    for name in D.SUMS:
        assert sum(b["sums"][name] for b in bodies) == d["sums"][name], name
    terms = M.row_terms(pos, vel, rho)
    first_nine = sum(int(M.q_terms(terms[name])[1].sum()) for name in M.SUMS[:9])
    assert first_nine == d["saturated"] and sum(b["saturated"] for b in bodies) > d["saturated"] > 1


# ---- sph_body_values through ctypes ----

def assert_values_equal(got, want, what):
    """got: one entry of the structured array of _lib.body_values; want: the dict of M.values"""
    assert set(want) == set(M.VALUE_FIELDS) == set(got.dtype.names)
    for name, w in want.items():
        g = tuple(got[name].tolist()) if isinstance(w, tuple) else got[name].item()
        assert g == w, f"{what}: {name} {g!r} vs {w!r}"


def test_values_equal_the_python_expressions():
    s = settings()
    for nan in (False, True):
        pos, vel, rho, labels = seeded(nan=nan)
        labels[labels == 39] = 1000 + np.arange((labels == 39).sum())  # singletons too
        bodies = M.restate(pos, vel, rho, labels)
        got = _lib.body_values(M.to_rows(bodies), s)
        assert len(got) == len(bodies) > 40
        for g, b in zip(got, bodies):
            assert_values_equal(g, M.values(b), f"body {b['label']}")
    singles = [M.values(b) for b in bodies if b["count"] == 1]
    # a body of one: the second moment is floored to a unit of Q32.32 and the coordinate is exact in it, so the
    # covariance is residue in (-2^-32, 0] plus the roundings of a square below 100 (a few 2^-46)
    assert singles and all(abs(c) <= 2.0**-32 + 1e-12 for v in singles for c in v["covariance"])
    assert any(c < 0 for v in singles for c in v["covariance"])
    L = sph.load_library()
    assert len(_lib.body_values(M.to_rows([]), s)) == 0
    one = M.to_rows(bodies[:1])
    rows, out = one.ctypes.data_as(C.POINTER(_lib.SphBodyMomentsRaw)), _lib.SphBodyValues()
    assert L.sph_body_values(rows, 1, None, C.byref(out)) == SPH_EINVAL
    assert L.sph_body_values(None, 1, C.byref(s), C.byref(out)) == SPH_EINVAL
    assert L.sph_body_values(rows, -1, C.byref(s), C.byref(out)) == SPH_EINVAL
    assert L.sph_body_values(None, 0, C.byref(s), None) == 0


def test_rows_round_trip_and_the_size_histogram():
    pos, vel, rho, labels = seeded()
    bodies = M.restate(pos, vel, rho, labels)
    assert M.from_rows(M.to_rows(bodies)) == bodies and M.to_rows(bodies).dtype == _lib.body_moments_dtype()
    assert min(min(b["sums"].values()) for b in bodies) < 0
    hist = M.size_hist([dict(count=c) for c in (1, 1, 2, 3, 4, 7, 8, 2**31, 2**32 - 1)])
    assert hist.dtype == np.uint32 and hist.nonzero()[0].tolist() == [0, 1, 2, 3, 31] and hist[[0, 1, 2, 3, 31]].tolist() == [2, 2, 2, 1, 2]


# ---- layouts, header, binding, and the stand-alone sanitizer run ----

def test_header_library_and_binding_carry_the_body_moments():
    text = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
    assert re.search(r"#define\s+SPH_HAS_BODY_MOMENTS\s+1", text) and re.search(r"#define\s+SPH_API_VERSION\s+3\b", text)
    assert re.search(r"SPH_BODY_SUMS\s*=\s*18\b", text)
    L = sph.load_library()
    for name in ("sph_measure_bodies", "sph_body_moments_host", "sph_body_values", "sph_get_body_measure_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert _lib.SPH_HAS_BODY_MOMENTS == 1 and len(_lib.BODY_SUMS) == 18 and tuple(_lib.BODY_SUMS) == M.SUMS
    assert _lib.body_moments_dtype() == M.ROW_DTYPE and _lib.body_moments_dtype().itemsize == C.sizeof(_lib.SphBodyMomentsRaw)
    assert _lib.body_values_dtype().itemsize == C.sizeof(_lib.SphBodyValues)
    for name, _ in _lib.SphBodyValues._fields_:
        assert _lib.body_values_dtype().fields[name][1] == getattr(_lib.SphBodyValues, name).offset, name
    for name in ("measure_bodies", "body_values", "body_measure_stats"):
        assert callable(getattr(sph.Simulator, name)), name


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/body_moments_selftest.cpp + csrc/sph_body_values.cpp under ASan + UBSan, run once: {name: [values]}"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("moments") / "body_moments_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "body_moments_selftest.cpp"),
                    os.path.join(ROOT, "cudafluidsimulator_amd", "csrc", "sph_body_values.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and not p.stderr, f"sanitizer report or failure:\n{p.stderr}"
    out = {}
    for line in p.stdout.splitlines():
        name, val = line.split()
        out.setdefault(name, []).append(val)
    return out


def test_struct_sizes_and_offsets_match_the_ctypes_mirrors(selftest):
    one = lambda name: int(selftest[name][0])
    assert one("sizeof_options") == C.sizeof(_lib.SphBodyMeasureOptions) == 16
    assert one("sizeof_raw") == C.sizeof(_lib.SphBodyMomentsRaw) == 304
    assert one("sizeof_values") == C.sizeof(_lib.SphBodyValues) == 200
    assert one("sizeof_stats") == C.sizeof(_lib.SphBodyMeasureStats) == 24
    for tag, struct in (("options", _lib.SphBodyMeasureOptions), ("raw", _lib.SphBodyMomentsRaw), ("values", _lib.SphBodyValues),
                        ("stats", _lib.SphBodyMeasureStats)):
        for f, _ in struct._fields_:
            if f not in ("struct_size",) and not (tag == "stats" and f == "pad_"):
                assert one(f"{tag}_{f}") == getattr(struct, f).offset, (tag, f)


def test_the_host_function_under_the_sanitizers(selftest):
    cases = dict(carry=(M.INT64_MAX, 2**20), small=(3, 3), one=((5 << 32) + 12345, 1), tie=(2**53 + 1, 7), zero=(0, 2),
                 empty=(99, 0), most=(2**40, 2**32 - 1))
    assert selftest["rc"] == ["0"]
    for c, (tag, (base, count)) in enumerate(cases.items()):
        sums = {name: (-1 if k & 1 else 1) * base * (k + 1) for k, name in enumerate(M.SUMS)}
        want = M.values(dict(label=c, count=count, saturated=c * 1000003, sums=sums))
        for name, w in want.items():
            got = selftest[f"{tag}_{name}"]
            if name == "saturated":
                assert got == [str(w)], tag
            else:
                assert tuple(float.fromhex(g) for g in got) == (w if isinstance(w, tuple) else (w,)), (tag, name, got, w)
    assert selftest["none_rc"] == ["0"]
    for name in ("null_rows_rc", "null_out_rc", "null_settings_rc", "negative_rc"):
        assert selftest[name] == [str(SPH_EINVAL)], name


# ---- the shared states hold what the GPU tests rely on ----

def restated_big(name, link):
    """the bodies' restatement of a body_states.big state over the oracle's grid, with the label and the table row of
    every row of the sorted stream"""
    if (name, link) not in _cache:
        pos = BS.big(name)[0]
        s = O.make_settings(len(pos), True)
        cells = int(s.numCellsPerDim)
        keys = O.cell_keys(s, pos)
        ids = np.asarray(O.stable_sort(keys, cells ** 3), dtype=np.int64)
        cs, ce = O.cell_table(keys[ids], cells ** 3)
        out = BR.bodies(pos[ids], ids, np.stack([cs, ce], axis=1), s.h, cells, link)
        out["row_body"] = np.searchsorted(out["table"][:, 0], out["labels"][ids])
        _cache[name, link] = out
    return _cache[name, link]


def wave_groups(row_body):
    """per wave of 64 rows: its bodies, and whether one of them sits on lanes that are not adjacent"""
    out = []
    for w in range(0, len(row_body), 64):
        rows = row_body[w:w + 64]
        split = any(np.diff(np.flatnonzero(rows == b)).max(initial=1) > 1 for b in np.unique(rows))
        out.append((len(np.unique(rows)), split))
    return out


def test_the_inputs_hold_what_the_gpu_tests_need():
    # link h: a giant that is the first row's body of both 2,048-row blocks and nearly fills them (the LDS fold)
    out = restated_big("uniform4096", 0.0)
    rb, counts = out["row_body"], out["table"][:, 1]
    giant = int(np.argmax(counts))
    assert out["num_bodies"] == 89
    for block in (rb[:2048], rb[2048:]):
        assert block[0] == giant and int((block == giant).sum()) > 1900
    assert max(g for g, _ in wave_groups(rb)) == 7
    # link 0.08: many bodies per wave, on lanes that are not adjacent; the folded body is not the block's biggest
    out = restated_big("uniform4096", 0.08)
    rb = out["row_body"]
    assert out["num_bodies"] == 785
    for block in (rb[:2048], rb[2048:]):
        assert int((block == block[0]).sum()) < np.bincount(block).max()
    groups = wave_groups(rb)
    assert max(g for g, _ in groups) == 35 and all(split for _, split in groups)
    hist = M.size_hist([dict(count=int(c)) for c in out["table"][:, 1]])
    assert int((hist > 0).sum()) == 8 and int(hist.sum()) == 785
    # a wave of 64 rows that are 64 bodies of one
    out = restated_big("random4096", 0.0)
    rb, counts = out["row_body"], out["table"][:, 1]
    assert any((counts[rb[w:w + 64]] == 1).all() for w in range(0, 4096, 64))
