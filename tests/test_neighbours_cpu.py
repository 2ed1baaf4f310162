"""The two restatements of the neighbour lists (tests/neighbour_restatement.py) held to each
other and to the restatements the project already trusts, without a GPU: all pairs against the 27-cell walk, the
relation's symmetry, the bodies' links, the derived fields' neighbour counts, and the pairs at the radius itself.
Every comparison is of integers."""
import numpy as np
import pytest

import bodies_restatement as BR
import body_states as BS
import derived_restatement as DR
import grid_states as G
import neighbour_restatement as NR
import neighbour_states as NS

F = np.float32
RADII = (0.0, 0.08, 0.025)
_cache = {}


def state(name):
    """-> pos by id, h, D"""
    if name in ("dense4096", "random4096", "uniform4096"):
        return BS.big(name)[0], 0.1, 100
    if name == "boundary_pairs":
        return BS.boundary_pairs()[0], 0.1, 100
    pos, _, g = NS.on_the_walls(name)
    return pos, g["h"], g["cells"]


def restated(name, radius):
    """both restatements of one state and radius, computed once: (a) all pairs, (b) the walk, and the grid (b) walked"""
    if (name, radius) not in _cache:
        pos, h, D = state(name)
        grid = NR.grid_of(pos, h, D)
        _cache[name, radius] = dict(pos=pos, h=h, D=D, grid=grid, a=NR.all_pairs(pos, h, radius), b=NR.walk_order(*grid, h, D, radius))
    return _cache[name, radius]


STATES = ("dense4096", "random4096", "uniform4096", "D1", "D2", "D3", "boundary_pairs")
CASES = [(s, r) for s in STATES for r in RADII]


@pytest.mark.parametrize("name,radius", CASES)
def test_all_pairs_and_the_walk_give_the_same_lists(name, radius):
    R = restated(name, radius)
    (oa, na), (ob, nb) = R["a"], R["b"]
    assert oa.dtype == ob.dtype == np.uint64 and na.dtype == nb.dtype == np.uint32
    assert np.array_equal(oa, ob), f"{name}, radius {radius}: the lists' lengths differ"
    walked = NR.lists_of(ob, nb)
    assert np.array_equal(np.concatenate([np.sort(l) for l in walked] + [np.zeros(0, np.uint32)]), na)
    if name in ("dense4096", "uniform4096") and radius == 0.0:
        assert any((np.diff(l.astype(np.int64)) < 0).any() for l in walked), "the walk's order is the ascending one: nothing is tested"


@pytest.mark.parametrize("name,radius", CASES)
def test_the_relation_is_symmetric_without_self_or_duplicates(name, radius):
    offsets, nb = restated(name, radius)["a"]
    n = len(offsets) - 1
    owner = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
    assert (owner != nb).all(), "a particle in its own list"
    pairs = owner * n + nb.astype(np.int64)
    assert len(np.unique(pairs)) == len(pairs), "a duplicate"
    assert np.array_equal(np.sort(pairs), np.sort(nb.astype(np.int64) * n + owner)), "not symmetric"


@pytest.mark.parametrize("name,radius", CASES)
def test_entries_are_twice_the_bodies_links(name, radius):
    R = restated(name, radius)
    pos_rows, ids, ranges = R["grid"]
    pairs = BR.links_of(pos_rows, ranges, R["h"], R["D"], BR.link_r2(R["h"], radius))
    unordered = np.unique(np.sort(pairs, axis=1), axis=0) if len(pairs) else pairs
    assert int(R["a"][0][-1]) == 2 * len(unordered)


@pytest.mark.parametrize("name", STATES)
def test_at_radius_h_the_counts_are_the_derived_fields(name):
    R = restated(name, 0.0)
    pos_rows, ids, ranges = R["grid"]
    d = DR.derive(pos_rows, np.zeros_like(pos_rows), ranges, R["h"], G.kernel_coeffs(R["h"])[1], R["D"])
    by_id = np.empty(len(ids), np.int64)
    by_id[ids] = d["neighbours"]
    assert np.array_equal(np.diff(R["a"][0].astype(np.int64)) + 1, by_id)


def test_the_binding_mirrors_the_header():
    import ctypes as C

    import cudafluidsimulator_amd as sph
    from cudafluidsimulator_amd import _lib
    o, s = _lib.SphNeighbourOptions, _lib.SphNeighbourStats
    assert C.sizeof(o) == 24 and (o.radius.offset, o.flags.offset, o.pad_.offset, o.max_entries.offset) == (4, 8, 12, 16)
    assert C.sizeof(s) == 56 and (s.calls.offset, s.entries.offset, s.longest.offset, s.runs_staged.offset, s.seconds.offset) == (8, 16, 24, 32, 48)
    assert (_lib.SPH_HAS_NEIGHBOURS, _lib.SPH_NEIGHBOURS_WALK_ORDER) == (1, 1)
    L = sph.load_library()
    for name in ("sph_neighbour_lists", "sph_neighbours_host", "sph_get_neighbour_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_the_pair_at_the_radius_is_in_and_the_next_float_is_out():
    pos, (near, far), r2 = BS.boundary_pairs()
    assert near == r2 and far > r2
    for which in ("a", "b"):
        offsets, nb = restated("boundary_pairs", 0.0)[which]
        assert offsets.tolist() == [0, 1, 2, 2, 2] and nb.tolist() == [1, 0], which
