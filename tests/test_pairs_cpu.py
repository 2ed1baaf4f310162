"""The pair statistics without a GPU: the two restatements of tests/pair_restatement.py against
each other on the states the GPU tests use, their pair counts against the bodies' links, and the library's pure host
functions sph_pair_edges / sph_pair_values against their restatements, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import pair_restatement as PR
import pair_states as PS

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH_EINVAL = -1
RADII = (0.0, 0.08, 0.025)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else np.uint64)


@pytest.mark.parametrize("name", PS.ALL)
def test_the_two_restatements_agree_and_count_the_bodies_links(name):
    pos, vel, h, cells = PS.state(name)
    for radius, bins in ((0.0, 0), (0.3 * float(h), 5)) if name in PS.SMALL else ((0.08, 16),):
        a = PR.all_pairs(pos, vel, h, radius, bins)
        b = PR.from_lists(pos, vel, h, radius, bins)
        PR.assert_same_table(b, a, f"{name}, radius {radius}, {bins} bins: (b) against (a)")
        links = BR.all_pairs_components(pos, h, radius)[2] if len(pos) > 1 else 0
        assert int(a["pairs"].sum()) == links, (name, radius)
        assert PR.describe_difference(PR.from_rows(PR.to_rows(a), a["edges2"]), a) == []


def test_the_states_hold_what_the_gpu_tests_need():
    # every edge of the 8-bin table has pairs of the origin's on both sides and one within an ulp; the last edge too
    pos, edges = PS.on_the_edges()
    assert len(edges) == PS.EDGE_BINS
    PS.assert_edges_straddled(pos, edges)
    t = PR.all_pairs(*PS.state("edges")[:2], PS.H, 0.0, PS.EDGE_BINS)
    assert (t["pairs"] > 0).all()
    # coincident particles: bin 0, the u_par^2 term 0; particles far apart: an all-zero table
    t = PR.all_pairs(*PS.state("coincident")[:2], PS.H)
    assert t["pairs"].tolist() == [1] + [0] * 31 and t["sums"][0, 0] == 0 and t["sums"][0, 3] == 0 and t["sums"][0, 1] > 0
    t = PR.all_pairs(*PS.state("far_pair")[:2], PS.H)
    assert not t["pairs"].any() and not t["saturated"].any() and not any(int(s) for s in t["sums"].reshape(-1))
    # saturation: clamped and zeroed terms, a negative sum
    t = PR.all_pairs(*PS.state("saturating")[:2], PS.H, 0.0, 4)
    assert t["saturated"].sum() > 40 and max(int(s) for s in t["sums"][:, 1]) >= PR.INT64_MAX
    t = PR.all_pairs(*PS.state("dense4096")[:2], PS.H, 0.08, 16)
    assert min(int(s) for s in t["sums"][:, 2]) < 0


@pytest.mark.parametrize("bins", [0, 1, 2, 8, 32, 127, 128])
def test_pair_edges_is_its_restatement(bins):
    for h in (0.1, 0.25, 0.05):
        for radius in (0.0, 0.08 * h / 0.1, 0.025, 1e-30, float(F(h))):
            if radius > float(F(h)):
                continue
            got = _lib.pair_edges(radius, h, bins)
            want = PR.edges2(radius, h, bins)
            assert got.dtype == F and np.array_equal(bits(got), bits(want)), (bins, h, radius)
            assert (np.diff(got.astype(np.float64)) >= 0).all()
    # a radius so small that the squares underflow: the edges repeat, and the table still does not decrease
    tiny = _lib.pair_edges(1e-30, 0.1, 128)
    assert len(np.unique(tiny)) < 128 and (np.diff(tiny.astype(np.float64)) >= 0).all()


def test_pair_edges_refuses():
    L = sph.load_library()
    out = (C.c_float * 128)()
    for radius, h, bins in ((0.05, 0.1, -1), (0.05, 0.1, 129), (0.2, 0.1, 8), (-0.01, 0.1, 8), (float("nan"), 0.1, 8),
                            (float("inf"), 0.1, 8), (0.05, 0.0, 8), (0.05, float("nan"), 8)):
        assert L.sph_pair_edges(radius, h, bins, out) == SPH_EINVAL, (radius, h, bins)
    assert L.sph_pair_edges(0.05, 0.1, 8, None) == SPH_EINVAL


def made_up_table(bins, seed):
    """rows no state produced: empty bins, sums of either sign and of more than 64 bits, pairs beyond 2^53"""
    rng = np.random.default_rng(seed)
    t = dict(pairs=rng.integers(0, 1 << 20, bins).astype(np.uint64), sums=np.empty((bins, 4), object),
             saturated=rng.integers(0, 9, bins).astype(np.uint64))
    for k in range(bins):
        for s in range(4):
            t["sums"][k, s] = int(rng.integers(-(1 << 62), 1 << 62)) * int(rng.integers(1, 1 << 40)) >> int(rng.integers(0, 60))
    t["pairs"][1::3] = 0
    t["pairs"][bins // 2] = (1 << 60) + 1
    t["sums"][0, 2] = -1
    t["sums"][bins - 1, 0] = -(1 << 100) - 12345
    return t


@pytest.mark.parametrize("bins", [1, 2, 32, 128])
def test_pair_values_equal_the_python_expressions(bins):
    s = sph.default_settings(4096, True)
    tables = [dict(made_up_table(bins, bins), edges2=PR.edges2(0.0, s.h, bins)),
              dict(made_up_table(bins, bins + 1), edges2=PR.edges2(1e-30, s.h, bins))]
    pos, vel, h, _ = PS.state("saturating")
    tables.append(PR.all_pairs(pos, vel, h, 0.0, bins))
    for t in tables:
        for n in (0, 1, 48, 4096, 1 << 24):
            got = _lib.pair_values(PR.to_rows(t), t["edges2"], s, n)
            want = PR.values(t, s.boxDim, n)
            for k in range(bins):
                for name in PR.VALUE_FIELDS:
                    g, w = got[name][k], want[k][name]
                    if name == "saturated":
                        assert int(g) == w, (bins, n, k, name)
                    else:
                        assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64), (bins, n, k, name, g, w)
    assert any(v["approach"] < 0 for v in PR.values(tables[0], s.boxDim, 4096))


def test_pair_values_refuses_a_table_that_decreases():
    s = sph.default_settings(64, True)
    t = dict(made_up_table(8, 3), edges2=PR.edges2(0.0, s.h, 8))
    rows = PR.to_rows(t)
    assert len(_lib.pair_values(rows, t["edges2"], s, 64)) == 8
    for spoil in (lambda e: e.__setitem__(3, e[1]), lambda e: e.__setitem__(0, np.nan), lambda e: e.__setitem__(7, F(0))):
        edges = t["edges2"].copy()
        spoil(edges)
        with pytest.raises(sph.SphError, match=rf"\({SPH_EINVAL}\)"):
            _lib.pair_values(rows, edges, s, 64)
    # equal edges are a table: the bins between them are empty shells
    edges = t["edges2"].copy()
    edges[3] = edges[2]
    got = _lib.pair_values(rows, edges, s, 64)
    assert got["r_lo"][3] == got["r_hi"][3] and got["g"][3] == 0.0
    L = sph.load_library()
    fp = C.POINTER(C.c_float)
    out = (_lib.SphPairValues * 8)()
    args = lambda b, n: (rows.ctypes.data_as(C.POINTER(_lib.SphPairBinRaw)), t["edges2"].ctypes.data_as(fp), b, C.byref(s), n, out)
    assert L.sph_pair_values(*args(8, 64)) == 0
    assert L.sph_pair_values(*args(0, 64)) == SPH_EINVAL and L.sph_pair_values(*args(129, 64)) == SPH_EINVAL
    assert L.sph_pair_values(*args(8, -1)) == SPH_EINVAL


def test_header_library_and_binding_carry_the_pair_statistics():
    text = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
    assert re.search(r"#define\s+SPH_HAS_PAIR_STATS\s+1\b", text) and _lib.SPH_HAS_PAIR_STATS == 1
    assert C.sizeof(_lib.SphPairBinRaw) == 80 == PR.ROW_DTYPE.itemsize == _lib.pair_bin_dtype().itemsize
    assert C.sizeof(_lib.SphPairOptions) == 20 and C.sizeof(_lib.SphPairValues) == 72 == _lib.pair_values_dtype().itemsize
    assert C.sizeof(_lib.SphPairStats) == 48
    assert tuple(name for name, _ in _lib.SphPairValues._fields_) == PR.VALUE_FIELDS
    L = sph.load_library()
    for name in ("sph_pair_edges", "sph_pair_statistics", "sph_pair_statistics_host", "sph_pair_values", "sph_get_pair_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
