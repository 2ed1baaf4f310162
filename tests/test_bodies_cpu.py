"""The bodies' restatement (tests/bodies_restatement.py) against scipy's connected components over an all-pairs link
matrix that knows no cells, against the derived fields' neighbour counts, and against answers worked out by hand; and
the conditions the GPU tests put on their inputs; and the C-ABI's new declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import body_states as BS
import derived_restatement as DR
from oracle import oracle as O

F = np.float32
U = np.uint32
_cache = {}


def grid_of(pos):
    """the oracle's grid of a state for the default settings: (settings, D, ids of the rows, cell ranges)"""
    s = O.make_settings(len(pos), True)
    D = int(s.numCellsPerDim)
    keys = O.cell_keys(s, pos)
    perm = O.stable_sort(keys, D ** 3)
    cs, ce = O.cell_table(keys[perm], D ** 3)
    return s, D, np.asarray(perm, dtype=np.int64), np.stack([cs, ce], axis=1)


def restated(pos, link):
    s, D, ids, cells = grid_of(pos)
    assert F(s.h) == BS.H
    out = BR.bodies(pos[ids], ids, cells, s.h, D, link)
    out["ids"] = ids
    return out


def restated_big(name, link):
    if (name, link) not in _cache:
        _cache[name, link] = restated(BS.big(name)[0], link)
    return _cache[name, link]


def assert_consistent(out, n):
    t = out["table"]
    assert t.dtype == U and t.shape == (out["num_bodies"], 8)
    assert int(t[:, 1].sum()) == n and (np.diff(t[:, 0].astype(np.int64)) > 0).all()
    assert np.array_equal(out["labels"][t[:, 0]], t[:, 0])
    assert (out["labels"] <= np.arange(n)).all()
    most = t[:, 1].max()
    assert out["largest"] == t[t[:, 1] == most, 0].min()


@pytest.mark.parametrize("name,link", BS.BIG)
def test_the_cell_walk_loses_no_link(name, link):
    pos = BS.big(name)[0]
    out = restated_big(name, link)
    k, comp, links = BR.all_pairs_components(pos, BS.H, link)
    assert out["num_bodies"] == k and out["links"] == links
    # the same partition: every scipy component carries one label, and its smallest member is that label
    first = np.full(k, len(pos), np.int64)
    np.minimum.at(first, comp, np.arange(len(pos)))
    assert np.array_equal(out["labels"], first[comp].astype(U))
    assert_consistent(out, len(pos))


@pytest.mark.parametrize("name", ["dense4096", "random4096", "uniform4096"])
def test_links_and_singletons_are_the_derived_fields_neighbour_counts(name):
    pos, vel = BS.big(name)
    s, D, ids, cells = grid_of(pos)
    nb = DR.derive(pos[ids], vel[ids], cells, s.h, s.d_kernel_coeff, D)["neighbours"].astype(np.int64)
    out = restated_big(name, 0.0)
    assert 2 * out["links"] == int(nb.sum()) - len(pos)
    by_id = np.empty_like(nb)
    by_id[ids] = nb
    assert np.array_equal(by_id - 1, out["degree"])
    alone = np.zeros(len(pos), bool)
    t = out["table"]
    alone[t[t[:, 1] == 1, 0]] = True
    assert np.array_equal(alone, by_id == 1)


def rows_spanned(out):
    """per body: the distance between its first and its last row of the sorted stream"""
    row_of = np.empty(len(out["ids"]), np.int64)
    row_of[out["ids"]] = np.arange(len(out["ids"]))
    which, inv = np.unique(out["labels"], return_inverse=True)
    lo, hi = np.full(len(which), 1 << 40), np.zeros(len(which), np.int64)
    np.minimum.at(lo, inv, row_of)
    np.maximum.at(hi, inv, row_of)
    return hi - lo


def test_the_inputs_hold_what_the_gpu_tests_need():
    count = lambda name, link: restated_big(name, link)["num_bodies"]
    size = lambda name, link: int(restated_big(name, link)["table"][:, 1].max())
    assert count("dense4096", 0.0) == 1
    assert 1500 < count("dense4096", 0.025) < 2500 and 1 < size("dense4096", 0.025) <= 8
    assert 3900 < count("random4096", 0.0) < 4096 and size("random4096", 0.0) == 2
    got = [count("uniform4096", l) for l in (0.0, 0.08, 0.06)]
    assert 40 < got[0] < 160 and 500 < got[1] < 1000 and 2000 < got[2] < 2700, got
    t = restated_big("uniform4096", 0.08)["table"]
    assert (t[:, 1] >= 64).sum() >= 2 and (t[:, 1] == 1).sum() > 100 and size("uniform4096", 0.0) > 3000
    # each state: somewhere more than one body, and a body that reaches across more than one wave of sorted rows
    for name, several, link in (("dense4096", 0.025, 0.08), ("random4096", 0.0, 0.0), ("uniform4096", 0.08, 0.08)):
        assert count(name, several) > 1 and rows_spanned(restated_big(name, link)).max() > 64, name


def test_one_particle():
    out = restated(np.array([[5.05, 5.05, 5.05]], F), 0.0)
    assert out["labels"].tolist() == [0] and out["num_bodies"] == 1 and out["largest"] == 0 and out["links"] == 0
    p = np.array([5.05, 5.05, 5.05], F).view(U)
    assert out["table"].tolist() == [[0, 1, *p, *p]]


def test_a_pair_at_exactly_the_link_length_and_one_a_float_further():
    pos, (near, far), r2 = BS.boundary_pairs()
    assert near == r2 and far > r2 and pos[1, 0] == BS.H and pos[3, 0] == np.nextafter(BS.H, F(1))
    out = restated(pos, 0.0)
    assert out["labels"].tolist() == [0, 0, 2, 3] and out["num_bodies"] == 3 and out["links"] == 1 and out["largest"] == 0
    assert out["table"][:, :2].tolist() == [[0, 2], [2, 1], [3, 1]]
    box = out["table"][0, 2:].view(F)
    assert box.tolist() == [0.0, F(5.05), F(5.05), BS.H, F(5.05), F(5.05)]


def test_a_chain_and_the_chain_cut_in_the_middle():
    pos, where = BS.chain()
    out = restated(pos, 0.0)
    assert out["num_bodies"] == 1 and (out["labels"] == 0).all() and out["links"] == 256 and out["largest"] == 0
    assert out["table"][0, :2].tolist() == [0, 257]
    assert np.array_equal(out["table"][0, 2:].view(F), np.concatenate([pos.min(axis=0), pos.max(axis=0)]))
    assert sorted(out["degree"].tolist()) == [1, 1] + [2] * 255
    pos, where = BS.chain(without_middle=True)
    out = restated(pos, 0.0)
    head, tail = where < 128, where > 128
    assert head.sum() == tail.sum() == 128
    want = np.where(head, np.flatnonzero(head).min(), np.flatnonzero(tail).min()).astype(U)
    assert out["num_bodies"] == 2 and out["links"] == 254 and np.array_equal(out["labels"], want)
    assert out["largest"] == 0 and out["table"][:, 1].tolist() == [128, 128]
    for row in out["table"]:
        part = pos[out["labels"] == row[0]]
        assert np.array_equal(row[2:].view(F), np.concatenate([part.min(axis=0), part.max(axis=0)]))


def test_two_blobs_with_and_without_their_bridge():
    pos, order = BS.blobs(bridge=True)
    out = restated(pos, 0.0)
    assert out["num_bodies"] == 1 and out["table"][0, :2].tolist() == [0, 401]
    pos, order = BS.blobs(bridge=False)
    out = restated(pos, 0.0)
    in_a = order < 200
    want = np.where(in_a, np.flatnonzero(in_a).min(), np.flatnonzero(~in_a).min()).astype(U)
    assert out["num_bodies"] == 2 and np.array_equal(out["labels"], want) and out["table"][:, 1].tolist() == [200, 200]


def test_negative_zero_and_negative_coordinates_order_as_floats():
    keys = BR.order_key(np.array([-2.0, -0.0, 0.0, 1e-30, 3.0], F).view(U)).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    labels = np.zeros(3, U)
    table, largest = BR.table_of(np.array([[-1, 0.0, 2], [3, -0.0, -5], [0.5, 1, 1]], F), labels)
    assert table[0, 2:].view(F).tolist() == [-1.0, -0.0, -5.0, 3.0, 1.0, 2.0] and np.signbit(table[0, 3:4].view(F))[0]


def test_header_library_and_binding_carry_the_bodies():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sph_c_api.h")).read()
    assert re.search(r"#define\s+SPH_HAS_BODIES\s+1", text) and re.search(r"#define\s+SPH_API_VERSION\s+3\b", text)
    assert getattr(_lib, "SPH_HAS_BODIES", 0) == 1
    names = ("sph_label_bodies", "sph_bodies_host", "sph_get_body_stats")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.EXPORTED_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    assert set(names) <= set(re.findall(r" T (sph_\w+)", out))
    size = {"int32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8, "float": 4}
    for struct, total in ((_lib.SphBodyStats, 56), (_lib.SphBodyOptions, 8)):
        name = struct.__name__
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S)
        fields = re.findall(r"(int32_t|int64_t|uint64_t|double|float)\s+([^;]+);", m.group(1))
        declared = [(n.strip(), size[t]) for t, decl in fields for n in decl.split(",")]
        assert [n for n, _ in declared] == [n for n, _ in struct._fields_]
        assert [b for _, b in declared] == [C.sizeof(t) for _, t in struct._fields_]
        assert C.sizeof(struct) == sum(b for _, b in declared) == total
    assert _lib.SphBodyStats.seconds.offset == 48
    assert callable(getattr(sph.Simulator, "label_bodies", None)) and callable(getattr(sph.Simulator, "body_stats", None))
