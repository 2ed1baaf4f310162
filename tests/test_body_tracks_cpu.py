"""Body tracks without a GPU: hand answers of the restatement
(tests/body_tracks_restatement.py), the struct layouts through ctypes, the symbols in header, library and binding, and
the properties of the shared states that tests/test_gpu_body_tracks.py relies on, computed through the bodies'
restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import bodies_restatement as BR
import body_states as BS
import body_tracks_restatement as T
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_cache = {}


def labels_of(pos, link):
    """the bodies' restatement over the oracle's grid of a state for the default settings -> labels in id order"""
    s = O.make_settings(len(pos), True)
    D = int(s.numCellsPerDim)
    keys = O.cell_keys(s, pos)
    ids = np.asarray(O.stable_sort(keys, D ** 3), dtype=np.int64)
    cs, ce = O.cell_table(keys[ids], D ** 3)
    return BR.bodies(pos[ids], ids, np.stack([cs, ce], axis=1), s.h, D, link)["labels"]


def jittered(name, sigma):
    """the second state of the GPU tests' pairs: the positions moved by normal(0, sigma), seed 7"""
    pos, _ = BS.big(name)
    return (pos + np.random.default_rng(7).normal(0, sigma, pos.shape)).astype(F)


def shared_labels(name, link, sigma=0.0):
    if (name, link, sigma) not in _cache:
        _cache[name, link, sigma] = labels_of(jittered(name, sigma) if sigma else BS.big(name)[0], link)
    return _cache[name, link, sigma]


def two_calls(first, second):
    t = T.Tracker()
    a = t.call(np.asarray(first))
    return a, t.call(np.asarray(second)), t


# ---- hand answers ----

def test_two_groups_that_merge():
    before = [0] * 100 + [100] * 50
    a, b, t = two_calls(before, [0] * 150)
    assert a["tracks"]["track"].tolist() == [0, 1] and a["summary"]["born"] == 2
    assert b["edges"].tolist() == [(0, 0, 100, T.EDGE_MAIN_PARENT | T.EDGE_MAIN_CHILD), (1, 0, 50, T.EDGE_MAIN_CHILD)]
    assert b["tracks"].tolist() == [(0, 2, 0, 100, T.TRACK_CONTINUES | T.TRACK_MERGED)]  # the larger's track
    assert b["previous"].tolist() == [(0, 0, 100, 1, 0, 100, T.FATE_CONTINUES), (1, 100, 50, 1, 0, 50, T.FATE_ENDED)]
    assert b["summary"] == dict(previous_bodies=2, bodies=1, edges=2, continued=1, born=0, ended=1, merges=1, splits=0, next_track=2, sequence=2)


def test_one_group_that_splits():
    a, b, t = two_calls([0] * 150, [0] * 100 + [100] * 50)
    assert b["edges"].tolist() == [(0, 0, 100, T.EDGE_MAIN_PARENT | T.EDGE_MAIN_CHILD), (0, 1, 50, T.EDGE_MAIN_PARENT)]
    assert b["tracks"].tolist() == [(0, 1, 0, 100, T.TRACK_CONTINUES), (1, 1, 0, 50, T.TRACK_BORN)]  # the larger child continues
    assert b["previous"].tolist() == [(0, 0, 150, 2, 0, 100, T.FATE_CONTINUES | T.FATE_SPLIT)]
    assert b["summary"] == dict(previous_bodies=1, bodies=2, edges=2, continued=1, born=1, ended=0, merges=0, splits=1, next_track=2, sequence=2)


def test_a_tie_goes_to_the_smaller_label():
    pos, where = BS.chain()
    whole = labels_of(pos, 0.0)
    assert len(set(whole.tolist())) == 1
    cut = pos.copy()
    middle = int(np.flatnonzero(where == 128)[0])
    cut[middle] = (8.05, 8.05, 8.05)
    parts = labels_of(cut, 0.0)
    a, b, t = two_calls(whole, parts)
    assert sorted(b["counts"].tolist()) == [1, 128, 128] and b["child_ties"] == 1 and b["parent_ties"] == 0
    halves = [r for r in range(3) if b["counts"][r] == 128]
    assert b["previous"].tolist() == [(0, 0, 257, 3, halves[0], 128, T.FATE_CONTINUES | T.FATE_SPLIT)]
    for r in range(3):
        assert b["tracks"][r]["flags"] == (T.TRACK_CONTINUES if r == halves[0] else T.TRACK_BORN), r
    assert b["tracks"]["track"][halves[0]] == 0 and sorted(b["tracks"]["track"].tolist()) == [0, 1, 2]
    assert b["summary"]["splits"] == 1 and b["summary"]["born"] == 2 and b["summary"]["next_track"] == 3
    # the reverse: the two halves and the particle merge, the tie between the halves goes to the smaller label again
    c = t.call(whole)
    assert c["parent_ties"] == 1 and c["tracks"].tolist() == [(int(b["tracks"]["track"][halves[0]]), 3, halves[0], 128, T.TRACK_CONTINUES | T.TRACK_MERGED)]
    assert c["summary"]["ended"] == 2 and c["summary"]["merges"] == 1 and c["summary"]["next_track"] == 3


def test_a_body_with_two_parents_is_born_where_its_main_parent_goes_elsewhere():
    before = [0] * 10 + [10] * 2           # A = ids 0..9, B = ids 10, 11
    after = [0] * 6 + [6] * 6              # X = ids 0..5 (6 of A), Y = 4 of A and both of B
    a, b, t = two_calls(before, after)
    assert b["edges"].tolist() == [(0, 0, 6, T.EDGE_MAIN_PARENT | T.EDGE_MAIN_CHILD), (0, 1, 4, T.EDGE_MAIN_PARENT), (1, 1, 2, T.EDGE_MAIN_CHILD)]
    assert b["tracks"].tolist() == [(0, 1, 0, 6, T.TRACK_CONTINUES), (2, 2, 0, 4, T.TRACK_BORN | T.TRACK_MERGED)]
    assert b["previous"].tolist() == [(0, 0, 10, 2, 0, 6, T.FATE_CONTINUES | T.FATE_SPLIT), (1, 10, 2, 1, 1, 2, T.FATE_ENDED)]
    assert b["summary"] == dict(previous_bodies=2, bodies=2, edges=3, continued=1, born=1, ended=1, merges=1, splits=1, next_track=3, sequence=2)


def test_the_first_call_the_reset_and_the_refusal():
    t = T.Tracker()
    labels = np.array([0, 0, 2, 3, 2])
    a = t.call(labels)
    assert a["edges"].shape == (0,) and a["previous"].shape == (0,)
    assert a["tracks"].tolist() == [(k, 0, T.NONE, 0, T.TRACK_BORN) for k in range(3)]
    assert a["summary"] == dict(previous_bodies=0, bodies=3, edges=0, continued=0, born=3, ended=0, merges=0, splits=0, next_track=3, sequence=1)
    same = t.call(labels)
    assert same["tracks"]["track"].tolist() == [0, 1, 2] and same["summary"]["continued"] == 3 and same["summary"]["next_track"] == 3
    # a refusal: nothing changes, the next call is as if it had not happened
    assert t.call(np.arange(5), max_edges=4) is None
    assert (t.next_track, t.sequence) == (3, 2) and np.array_equal(t.labels, labels)
    singles = t.call(np.arange(5), max_edges=5)
    assert singles["tracks"]["track"].tolist() == [0, 3, 1, 2, 4] and singles["summary"]["sequence"] == 3
    t.reset()
    again = t.call(labels)
    assert again["tracks"].tobytes() == a["tracks"].tobytes() and again["summary"] == a["summary"]


# ---- the C-ABI ----

def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.SphBodyEdge) == 16 and C.sizeof(_lib.SphBodyTrack) == 24 and C.sizeof(_lib.SphBodyFate) == 32
    assert C.sizeof(_lib.SphBodyTrackOptions) == 16 and C.sizeof(_lib.SphBodyTrackSummary) == 56 and C.sizeof(_lib.SphBodyTrackStats) == 40
    for struct, dtype, mine in ((_lib.SphBodyEdge, _lib.body_edge_dtype(), T.EDGE_DTYPE), (_lib.SphBodyTrack, _lib.body_track_dtype(), T.TRACK_DTYPE),
                                (_lib.SphBodyFate, _lib.body_fate_dtype(), T.FATE_DTYPE)):
        assert dtype == mine and dtype.itemsize == C.sizeof(struct)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], (struct.__name__, name)
    assert [getattr(_lib.SphBodyTrackSummary, k).offset for k in T.SUMMARY] == [8, 12, 16, 20, 24, 28, 32, 36, 40, 48]
    assert _lib.TRACK_SUMMARY == T.SUMMARY
    assert (_lib.SPH_EDGE_MAIN_PARENT, _lib.SPH_EDGE_MAIN_CHILD) == (T.EDGE_MAIN_PARENT, T.EDGE_MAIN_CHILD)
    assert (_lib.SPH_TRACK_CONTINUES, _lib.SPH_TRACK_BORN, _lib.SPH_TRACK_MERGED) == (T.TRACK_CONTINUES, T.TRACK_BORN, T.TRACK_MERGED)
    assert (_lib.SPH_FATE_CONTINUES, _lib.SPH_FATE_ENDED, _lib.SPH_FATE_SPLIT) == (T.FATE_CONTINUES, T.FATE_ENDED, T.FATE_SPLIT)


def test_header_library_and_binding_carry_the_symbols():
    header = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
    assert re.search(r"#define SPH_HAS_BODY_TRACKS 1\b", header) and _lib.SPH_HAS_BODY_TRACKS == 1
    assert _lib.SPH_API_VERSION == 3, "additive: the version stays"
    L = _lib.load_library()
    for name in ("sph_track_bodies", "sph_body_tracks_host", "sph_track_reset", "sph_get_body_track_stats"):
        assert re.search(r"\bint " + name + r"\(sph_handle \*h", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name).argtypes, name
    for struct in ("SphBodyTrackOptions", "SphBodyEdge", "SphBodyTrack", "SphBodyFate", "SphBodyTrackSummary", "SphBodyTrackStats"):
        assert re.search(r"\} " + struct + ";", header), struct
    for word in ("SPH_TRACK_WITH_MOMENTS = 1", "SPH_EDGE_MAIN_PARENT = 1, SPH_EDGE_MAIN_CHILD = 2", "SPH_TRACK_CONTINUES = 1, SPH_TRACK_BORN = 2, SPH_TRACK_MERGED = 4",
                 "SPH_FATE_CONTINUES = 1, SPH_FATE_ENDED = 2, SPH_FATE_SPLIT = 4"):
        assert word in header, word
    for method in ("track_bodies", "track_reset", "body_track_stats"):
        assert callable(getattr(sph.Simulator, method))


# ---- the inputs of the GPU tests ----

def events(first, second):
    _, b, _ = two_calls(first, second)
    born_merged = int(((b["tracks"]["flags"] & T.TRACK_BORN) != 0)[b["tracks"]["parents"] >= 2].sum())
    return b, born_merged


def test_uniform4096_against_its_jitter_has_every_kind_of_event():
    b, born_merged = events(shared_labels("uniform4096", 0.06), shared_labels("uniform4096", 0.06, 0.02))
    s = b["summary"]
    print("uniform4096 at 0.06:", s, "most parents", int(b["tracks"]["parents"].max()), "ties", b["parent_ties"], b["child_ties"], "born with >= 2 parents", born_merged)
    assert s["merges"] >= 100 and s["splits"] >= 100
    assert b["parent_ties"] >= 50 and b["child_ties"] >= 50
    assert born_merged >= 10 and b["tracks"]["parents"].max() >= 5
    wide, _ = events(shared_labels("uniform4096", 0.08), shared_labels("uniform4096", 0.08, 0.02))
    print("uniform4096 at 0.08: most parents", int(wide["tracks"]["parents"].max()))
    assert wide["tracks"]["parents"].max() >= 20


def test_dense4096_against_its_jitter_has_a_body_of_a_thousand_parents():
    b, _ = events(shared_labels("dense4096", 0.025), shared_labels("dense4096", 0.025, 0.01))
    print("dense4096 at 0.025: most parents", int(b["tracks"]["parents"].max()))
    assert b["tracks"]["parents"].max() > 1000


def test_a_coarser_link_only_merges_and_a_finer_one_only_splits():
    fine, coarse = shared_labels("uniform4096", 0.025), shared_labels("uniform4096", 0.05)
    up, _ = events(fine, coarse)
    print("uniform4096, 0.025 -> 0.05:", up["summary"])
    assert up["summary"]["splits"] == 0 and up["summary"]["merges"] >= 100
    down, _ = events(coarse, fine)
    assert down["summary"]["merges"] == 0 and down["summary"]["splits"] == up["summary"]["merges"]
