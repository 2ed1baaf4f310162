"""The body tracks restated in numpy and plain Python, from two label arrays alone: the edges
are np.unique over the (previous row, current row) pairs of the particle ids, everything else follows the definition
word for word.  Imports nothing from the product."""
import numpy as np

U = np.uint32
NONE = 0xFFFFFFFF
EDGE_MAIN_PARENT, EDGE_MAIN_CHILD = 1, 2
TRACK_CONTINUES, TRACK_BORN, TRACK_MERGED = 1, 2, 4
FATE_CONTINUES, FATE_ENDED, FATE_SPLIT = 1, 2, 4
EDGE_DTYPE = np.dtype([("prev", "<u4"), ("cur", "<u4"), ("count", "<u4"), ("flags", "<u4")])
TRACK_DTYPE = np.dtype([("track", "<u8"), ("parents", "<u4"), ("main_parent", "<u4"), ("main_overlap", "<u4"), ("flags", "<u4")])
FATE_DTYPE = np.dtype([("track", "<u8"), ("label", "<u4"), ("count", "<u4"), ("children", "<u4"), ("main_child", "<u4"),
                       ("main_overlap", "<u4"), ("flags", "<u4")])
SUMMARY = ("previous_bodies", "bodies", "edges", "continued", "born", "ended", "merges", "splits", "next_track", "sequence")
assert (EDGE_DTYPE.itemsize, TRACK_DTYPE.itemsize, FATE_DTYPE.itemsize) == (16, 24, 32)


def table_of(labels):
    """-> (the labels of the bodies ascending, the table row of every particle id, the count of every body)"""
    labels = np.asarray(labels, dtype=np.int64)
    uniq, row, count = np.unique(labels, return_inverse=True, return_counts=True)
    return uniq, row.reshape(-1), count


def best(rows, counts):
    """of parallel lists: the row with the greatest count, the smallest such row on a tie -> (row, count, ties)"""
    top = max(counts)
    winners = sorted(r for r, c in zip(rows, counts) if c == top)
    return winners[0], top, len(winners)


def join(prev_labels, cur_labels, prev_tracks, next_track):
    """The overlap of two labellings of the same ids (prev_labels None: the first call) -> dict(edges, tracks, previous,
    summary without `sequence`, and what the tests look at besides: parent_ties, child_ties -- bodies whose main
    parent / child was decided by the tie rule)"""
    clab, crow, ccount = table_of(cur_labels)
    C = len(clab)
    first = prev_labels is None
    if first:
        plab, prow, pcount, P = np.zeros(0, np.int64), None, np.zeros(0, np.int64), 0
        pairs, counts = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    else:
        assert len(prev_labels) == len(cur_labels)
        plab, prow, pcount = table_of(prev_labels)
        P = len(plab)
        assert len(prev_tracks) == P
        # ascending (cur, prev): np.unique sorts the rows of (cur, prev) lexicographically
        both, counts = np.unique(np.stack([crow, prow], axis=1), axis=0, return_counts=True)
        pairs = both[:, ::-1]  # columns (prev, cur)
    E = len(pairs)
    into = [[] for _ in range(C)]    # edges into a current body
    out_of = [[] for _ in range(P)]  # edges out of a previous body
    for e in range(E):
        into[pairs[e, 1]].append(e)
        out_of[pairs[e, 0]].append(e)
    main_parent, main_child = [None] * C, [None] * P
    parent_ties = child_ties = 0
    for c in range(C):
        if into[c]:
            main_parent[c] = best([int(pairs[e, 0]) for e in into[c]], [int(counts[e]) for e in into[c]])
            parent_ties += main_parent[c][2] > 1
    for p in range(P):
        assert out_of[p], "a previous body without a particle"
        main_child[p] = best([int(pairs[e, 1]) for e in out_of[p]], [int(counts[e]) for e in out_of[p]])
        child_ties += main_child[p][2] > 1
    tracks = np.zeros(C, TRACK_DTYPE)
    born = 0
    continued_by = [None] * P
    for c in range(C):
        mp = main_parent[c]
        continues = mp is not None and main_child[mp[0]][0] == c
        if continues:
            assert continued_by[mp[0]] is None, "a track inherited twice"
            continued_by[mp[0]] = c
            track = int(prev_tracks[mp[0]])
        else:
            track = next_track + born
            born += 1
        parents = len(into[c])
        tracks[c] = (track, parents, NONE if mp is None else mp[0], 0 if mp is None else mp[1],
                     (TRACK_CONTINUES if continues else TRACK_BORN) | (TRACK_MERGED if parents >= 2 else 0))
    previous = np.zeros(P, FATE_DTYPE)
    for p in range(P):
        children = len(out_of[p])
        previous[p] = (int(prev_tracks[p]), plab[p], pcount[p], children, main_child[p][0], main_child[p][1],
                       (FATE_CONTINUES if continued_by[p] is not None else FATE_ENDED) | (FATE_SPLIT if children >= 2 else 0))
    edges = np.zeros(E, EDGE_DTYPE)
    for e in range(E):
        p, c = int(pairs[e, 0]), int(pairs[e, 1])
        edges[e] = (p, c, counts[e], (EDGE_MAIN_PARENT if main_parent[c][0] == p else 0) | (EDGE_MAIN_CHILD if main_child[p][0] == c else 0))
    continued = C - born
    summary = dict(previous_bodies=P, bodies=C, edges=E, continued=continued, born=born,
                   ended=sum(1 for p in range(P) if continued_by[p] is None),
                   merges=int((tracks["parents"] >= 2).sum()), splits=int((previous["children"] >= 2).sum()),
                   next_track=next_track + born)
    assert summary["continued"] + summary["born"] == C and summary["continued"] + summary["ended"] == P
    assert first or int(edges["count"].sum()) == len(cur_labels)
    return dict(edges=edges, tracks=tracks, previous=previous, summary=summary, parent_ties=int(parent_ties), child_ties=int(child_ties),
                labels=clab.astype(U), counts=ccount.astype(U))


class Tracker:
    """What a handle carries from call to call: the reference (the labels and tracks of the last successful call),
    next_track and sequence; a refused call changes nothing."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.labels, self.tracks, self.next_track, self.sequence = None, None, 0, 0

    def call(self, labels, max_edges=0):
        """-> join()'s dict with summary["sequence"], or None where the call is refused by max_edges"""
        r = join(self.labels, labels, self.tracks, self.next_track)
        if max_edges and r["summary"]["edges"] > max_edges:
            return None
        self.labels = np.array(labels, copy=True)
        self.tracks = r["tracks"]["track"].copy()
        self.next_track = r["summary"]["next_track"]
        self.sequence += 1
        r["summary"]["sequence"] = self.sequence
        return r


def assert_same(got, want, what):
    """a product result (a dict with tracks, previous, edges, summary) against join()'s / Tracker.call()'s, byte for byte"""
    for k, dt in (("edges", EDGE_DTYPE), ("tracks", TRACK_DTYPE), ("previous", FATE_DTYPE)):
        g = np.ascontiguousarray(got[k])
        assert g.dtype.itemsize == dt.itemsize and g.shape == want[k].shape, f"{what}: {k}: {g.shape} rows of {g.dtype.itemsize} bytes, not {want[k].shape}"
        if not g.tobytes() == want[k].tobytes():
            bad = [i for i in range(len(g)) if g[i].tobytes() != want[k][i].tobytes()]
            raise AssertionError(f"{what}: {k} differs in {len(bad)} rows, first {bad[0]}: {g[bad[0]]} not {want[k][bad[0]]}")
    s = {k: int(got["summary"][k]) for k in SUMMARY if k in want["summary"]}
    assert s == want["summary"], f"{what}: summary {s} not {want['summary']}"
