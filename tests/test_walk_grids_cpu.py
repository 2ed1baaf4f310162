"""The tracers' and the field sample's numpy restatements on the grids of tests/grid_states.py (one per sort plan, grids
too small for a 3 x 3 x 3 neighbourhood, h other than 0.1), without a GPU: that every tracer set of
tests/tracer_sets.py and every lattice of tests/walk_grid_cases.py reaches what tests/test_gpu_walk_grids.py relies
on, and the restatements themselves against a float64 sum over ALL pairs that uses no grid at all."""
import functools

import numpy as np
import pytest

import field_sample_restatement as FS
import grid_states as G
import tracer_restatement as TR
import tracer_sets as TS
import walk_grid_cases as W
from oracle import oracle as O

F = np.float32
U = 2.0 ** -24
MAX_GROUPS = 4      # tracers.hip's kTracerMaxGroups: a wave with more groups walks the direct way
RATIOS = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def oracle_grid(s, pos, vel, rho=None):
    """the oracle's grid of a state in particle-id order: sorted pos, vel, rho and the (D^3, 2) cell ranges"""
    D = int(s.numCellsPerDim)
    keys = O.cell_keys(s, pos)
    assert np.array_equal(keys, G.integer_keys(pos, s.h, D))
    perm = O.stable_sort(keys, D ** 3)
    cs, ce = O.cell_table(keys[perm], D ** 3)
    rho = np.zeros(len(pos), F) if rho is None else rho
    return pos[perm], vel[perm], rho[perm], np.stack([cs, ce], axis=1)


def sample(s, grid, field, lattice):
    return FS.sample(grid[0], grid[1], grid[2], grid[3], s.h, s.d_kernel_coeff, s.numCellsPerDim, field, *lattice)


@functools.lru_cache(maxsize=None)
def case(name):
    """settings, the oracle's grid, the sets and their restated advects (dt = timestep), the lattices and their
    restated density and speed; on crowded grids the same after one step of the oracle, with the pressure.  Computed
    once, shared, never written to."""
    pos, vel, g = G.grid_state(name)
    h, D = g["h"], g["cells"]
    s = G.settings_for(len(pos), h, D)
    grid = oracle_grid(s, pos, vel)
    sets = TS.grid_sets(pos, h, D)
    out = {k: TR.advect(grid[0], grid[1], grid[3], s.h, s.d_kernel_coeff, D, t, s.timestep) for k, t in sets.items()}
    lat = W.lattices(name, pos, h, D)
    fields = {(k, f): sample(s, grid, f, l) for k, l in lat.items() for f in ("density", "speed")}
    c = dict(name=name, g=g, s=s, h=h, D=D, pos=pos, vel=vel, grid=grid, sets=sets, out=out, lat=lat, fields=fields)
    if g["crowded"]:
        ref = G.oracle_sim(s)
        ref.upload(pos, vel)
        ref.step()
        st = ref.download()
        ref.close()
        G.assert_inside(st["pos"], h, D, name + " after a step")
        c["stepped"] = oracle_grid(s, st["pos"], st["vel"], st["rho"])
        c["stepped_lat"] = W.lattices(name, st["pos"], h, D)
        c["pressure"] = {k: sample(s, c["stepped"], "pressure", l) for k, l in c["stepped_lat"].items()}
    return c


def groups_in_caller_order(t, h, D):
    """what k_tracer_walk would count if the sort left the tracers in caller order: a group begins at every inside
    tracer whose group differs from the tracer before it in the wave"""
    c, outside = TR.cells_of(t, h, D)
    inside = ~outside.any(axis=1)
    gkey = np.where(inside, (c[:, 2].astype(np.int64) * D + c[:, 1]) * D + c[:, 0] // 8 * 8, -1)
    out = []
    for w in range(0, len(t), 64):
        k, ins = gkey[w:w + 64], inside[w:w + 64]
        head = ins & np.concatenate([[True], k[1:] != k[:-1]])
        out.append(int(head.sum()))
    return out


@pytest.mark.parametrize("name", W.GRIDS)
def test_the_sets_reach_what_they_are_meant_to_reach(name):
    c = case(name)
    sets, out, h, D, g = c["sets"], c["out"], c["h"], c["D"], c["g"]
    cell = TS.crowded_cell(c["pos"], h, D)
    # A: one occupied cell, four waves of one group
    cc, outside = TR.cells_of(sets["A"], h, D)
    assert len(cc) == 200 and not outside.any() and (cc == cell).all()
    assert TS.wave_groups(sets["A"], h, D) == [1, 1, 1, 1] and (out["A"]["den"] > 0).sum() > 100
    # B: the whole row where D < 8, over the block boundary 7|8 where D >= 8
    cc, outside = TR.cells_of(sets["B"], h, D)
    assert len(cc) == 130 and not outside.any() and (cc[:, 1:] == cell[1:]).all()
    xs = sorted(set(cc[:, 0].tolist()))
    assert xs == list(range(xs[0], xs[-1] + 1))
    if D < 8:
        assert xs == list(range(D))
        assert TS.wave_groups(sets["B"], h, D) == [1, 1, 1]
    else:
        assert 7 in xs and 8 in xs and len(xs) >= 7
        assert TS.wave_groups(sets["B"], h, D) == [1, 2, 1]     # (the boundary falls into the second wave)
    # C and G: particle positions shifted
    assert len(sets["C"]) == 150 and len(sets["G"]) == 4097 > 4 * 1024
    assert (out["C"]["den"] > 0).sum() >= min(100, len(c["pos"])) and (out["G"]["den"] > 0).sum() > 100
    # D: 64 tracers from exactly g rows, for as many rows as the state occupies, up to 25
    rows = len(np.unique(G.cells_of(c["pos"], h)[:, 1:], axis=0))
    names = [k for k in sets if k.startswith("D")]
    assert names == ["D%d" % k for k in range(1, min(rows, 25) + 1)]
    for k, key in enumerate(names, start=1):
        cc, outside = TR.cells_of(sets[key], h, D)
        assert not outside.any() and len(cc) == 64 and len(np.unique(cc[:, 1:], axis=0)) == k
    # E: outside flags, cells 0 and D - 1, words kept, the tracer on particle 7, three identical tracers
    t, e = sets["E"], out["E"]
    cc, outside = TR.cells_of(t, h, D)
    assert np.flatnonzero(outside.any(axis=1)).tolist() == TS.SPECIALS_OUTSIDE
    assert outside[0].tolist() == [True, False, False] and outside[1].tolist() == [False, True, False]
    assert bits(t[1, 1]) == bits(F(h) * F(D)) and t[0, 0] < 0
    assert cc[11].tolist() == [0, 0, 0] and cc[12].tolist() == [D - 1] * 3 and cc[13, :2].tolist() == [D - 1, 0]
    assert cc[[5, 6, 15], 0].tolist() == [0, 0, 0] and bits(t[5, 0]) == 0x80000000
    still = TS.SPECIALS_OUTSIDE
    assert np.array_equal(bits(e["pos"][still]), bits(t[still])) and (bits(e["den"][still]) == 0).all() and (bits(e["vel"][still]) == 0).all()
    assert bits(e["pos"])[14].tolist() == [0x7FC12345, 0xFFC00001, 0x7FC00000]
    assert e["den"][7] > 0 and np.array_equal(bits(t[7]), bits(c["pos"][7]))
    for k in ("pos", "den", "vel"):
        assert np.array_equal(bits(e[k][8]), bits(e[k][9])) and np.array_equal(bits(e[k][8]), bits(e[k][10]))
    assert e["den"][8] > 0
    # F: 88 in cell (0, 0, 0), 40 outside, alternating; sorted [1, 1], in caller order many groups and a direct walk
    t = sets["F"]
    cc, outside = TR.cells_of(t, h, D)
    out_f = outside.any(axis=1)
    assert len(t) == 128 and out_f.sum() == 40 and out_f[:80].tolist() == [False, True] * 40 and not out_f[80:].any()
    assert (cc[~out_f] == 0).all()
    assert TS.wave_groups(t, h, D) == [1, 1]
    assert groups_in_caller_order(t, h, D) == [32, 9] and 32 > MAX_GROUPS
    assert np.array_equal(bits(out["F"]["pos"][out_f]), bits(t[out_f])) and (bits(out["F"]["den"][out_f]) == 0).all()
    # group counts per wave: waves that walk shared and, where the grid has more than four rows, waves that walk direct
    counts = [n for t in sets.values() for n in TS.wave_groups(t, h, D)]
    assert min(counts) <= 1 and any(1 < n <= MAX_GROUPS for n in counts) == (D > 1)
    assert any(n > MAX_GROUPS for n in counts) == (D > 2)
    # what is compared is not zeros: tracers that see fluid, moved tracers, sums of both signs
    hits = sum(int((o["den"] > 0).sum()) for o in out.values())
    moved = sum(int((bits(o["pos"]) != bits(sets[k])).any(axis=1).sum()) for k, o in out.items())
    num = np.concatenate([o["num"].reshape(-1) for o in out.values()])
    assert hits >= 100 and moved >= 100 and (num < 0).sum() > 50 and (num > 0).sum() > 50, (hits, moved)
    for o in out.values():
        for k in ("den", "num"):
            assert not (bits(o[k]) == 0x80000000).any()


@pytest.mark.parametrize("name", W.GRIDS)
def test_the_lattices_reach_what_they_are_meant_to_reach(name):
    c = case(name)
    h, D, lat = c["h"], c["D"], c["lat"]
    assert sorted(lat) == sorted(["row", "fine"] + (["wide", "span"] if name in W.WIDE else []))
    for field in ("density", "speed"):
        nonzero = sum(int((c["fields"][k, field] != 0).sum()) for k in lat)
        assert nonzero >= 200, (name, field, nonzero)
    for k, (origin, spacing, shape) in lat.items():
        assert shape == ((3, 3, 65) if k == "span" else (3, 3, 130))      # two bricks and a two-lane tail
        cx, ox = FS.cells_of(FS.lattice_axis(origin[0], spacing[0], shape[2]), h, D)
        cy, oy = FS.cells_of(FS.lattice_axis(origin[1], spacing[1], shape[1]), h, D)
        cz, oz = FS.cells_of(FS.lattice_axis(origin[2], spacing[2], shape[0]), h, D)
        den = c["fields"][k, "density"]
        assert (bits(den[:, oy, :]) == 0).all() and (bits(den[:, :, ox]) == 0).all() and (bits(den[oz]) == 0).all()
        if k == "row":
            # a y row outside the grid, the anchor's row inside; 43 cells in x, or the whole row and both ends outside
            assert oy.tolist()[:2] == [True, False] and not ox[1] and ox[0] == (origin[0] < 0)
            assert ox[-1] == (D < 43) and 43 <= len(set(cx[~ox].tolist())) + max(43 - D, 0) <= 44
            assert D >= 43 or (ox[0] and cx[1] == 0)
            assert (den[:, 1, :] > 0).any()
        if k == "fine":
            assert len(set(cx[~ox].tolist())) <= 3 and not oy.any() or D == 1
            assert (den > 0).sum() >= 200
        if k in ("wide", "span"):
            far = 2 if k == "wide" else 4
            assert ox[0] and ox[-1] and not ox[1:-1].any() and (np.diff(cx[1:-1]) >= far).all()
            first = cx[1:64]                                             # the first brick: lanes 1 .. 63 are inside
            assert first[0] <= 1 and first[-1] >= (D // 2 - 4 if k == "wide" else D - 5)
            assert (den > 0).any(), "no point of the lattice sees the anchor"
    if c["g"]["crowded"]:
        nonzero = sum(int((p > 0).sum()) for p in c["pressure"].values())
        assert nonzero >= 200, (name, "pressure", nonzero)
    else:
        assert (c["grid"][2] == 0).all()      # (no step taken: the pressure of rho = 0 is 0 everywhere)


def test_the_long_run_is_several_chunks_with_a_partial_last_one():
    """from the cell table alone: the row of three x-cells around LONG_CELL holds more than 1,100 stream rows in one
    contiguous run, at least three chunks of either kernel (kTracerChunk 256, kSampleChunk 512), the last one partial"""
    pos, vel, g = W.long_run_state()
    h, D = g["h"], g["cells"]
    s = G.settings_for(len(pos), h, D)
    cells = oracle_grid(s, pos, vel)[3]
    cx, cy, cz = W.LONG_CELL
    runs = [cells[(cz * D + cy) * D + x] for x in (cx - 1, cx, cx + 1)]
    assert all(r[1] > r[0] for r in runs) and runs[0][1] == runs[1][0] and runs[1][1] == runs[2][0]
    count = int(runs[2][1] - runs[0][0])
    assert runs[1][1] - runs[1][0] >= W.LONG_ROWS and count > 1100
    for chunk in (256, 512):
        assert count > 2 * chunk and count % chunk != 0, (count, chunk)
    # the sets and the lattice lie where they should: three cells of the row, every wave one group; the lattice runs
    # the whole row with a point outside at either end
    sets = W.long_run_sets(h)
    for dx in (-1, 0, 1):
        c, outside = TR.cells_of(sets["L%d" % dx], h, D)
        assert not outside.any() and (c == (cx + dx, cy, cz)).all()
    assert TS.wave_groups(sets["Lall"], h, D) == [1] * 10
    origin, spacing, shape = W.long_run_lattice(h, D)
    c, outside = FS.cells_of(FS.lattice_axis(origin[0], spacing[0], shape[2]), h, D)
    assert outside[0] and outside[-1] and not outside[1:-1].any() and sorted(set(c[1:-1].tolist())) == list(range(D))
    for a in (1, 2):
        c, outside = FS.cells_of(FS.lattice_axis(origin[a], spacing[a], 3), h, D)
        assert not outside.any() and c.tolist() == [W.LONG_CELL[a]] * 3


# ---- the restatements against float64 over all pairs ----
#
# u = 2^-24, H2 = h^2 and W0 = MASS dcoef H2^3 (the weight at distance 0) in float64, from the fp32 inputs.  For one
# candidate at squared distance d2 <= H2 (1 + 8 u), to first order in u:
#   dx = p - x is rounded once, dx^2 carries 3 u; the two adds of d2 make it 5 u d2 <= 5 u H2 absolute;
#   h2 = fl(h h) carries u H2; diff = fl(h2 - d2) is off by u H2 + 5 u H2 + u |diff| <= 7 u H2 ABSOLUTE -- relative to
#   diff itself it is unbounded, diff cancels at the rim of the support;
#   diff^3 is off by 3 H2^2 (7 u H2) = 21 u H2^3, and the four multiplies of MASS (((dcoef diff) diff) diff) add 4 u:
#   |m - m64| <= 25 u W0.  TERM = 26 covers the terms of second order.
#   A numerator term m v_a rounds once more: |fl(m v_a) - m64 v_a| <= 27 u W0 |v_a|.
# The take test compares d2 and h2 with errors 5 u H2 and u H2: a candidate with |d2 - H2| <= 8 u H2 may be taken by one
# side only.  What it then adds or lacks is at most MASS dcoef (8 u H2)^3 on the float64 side and, with diff off by
# 7 u H2, no more on the fp32 side: far below its own allowance TERM u W0, so counting it among the K candidates
# covers it.  The same holds for a candidate within H2 that the grid walk does not visit because fl(p / h) put the
# point or the row into the next cell: its distance is h (1 - 2 u D) at least, its term below (4 u D)^3 W0.
# The left-to-right sum of K terms makes K - 1 adds, each off by u times a partial sum, which the sum of the
# magnitudes bounds: (K - 1) u (S + E) with S = sum |m64 v| (sum m64 for the density) and E the terms' own error.
# So  |den - den64| <= E + (K - 1) u (S + E),  E = K TERM u W0, and per axis
#     |num - num64| <= E + (K - 1) u (S + E),  E = (TERM + 1) u W0 sum |v_a|.
TERM = 26.0
MASS64 = float(F(0.02))


def all_pairs(points, pos, vel, h, dcoef):
    """float64 sums over ALL rows of the state for every point: den, num (m, 3), K (candidates within H2 (1 + 8 u)),
    marginal (|d2 - H2| <= 8 u H2), taken (d2 <= H2), S (m, 3) = sum |m64 v_a|, V (m, 3) = sum |v_a| over the K"""
    H2 = float(F(h)) ** 2
    W = MASS64 * float(F(dcoef))
    P, X, V = points.astype(np.float64), pos.astype(np.float64), np.abs(vel.astype(np.float64))
    out = dict(den=[], num=[], K=[], marginal=[], taken=[], S=[], V=[])
    for at in range(0, len(P), 1024):
        p = P[at:at + 1024]
        d2 = (p[:, None, 0] - X[None, :, 0]) ** 2
        d2 += (p[:, None, 1] - X[None, :, 1]) ** 2
        d2 += (p[:, None, 2] - X[None, :, 2]) ** 2
        take = d2 <= H2
        diff = H2 - d2
        m = np.where(take, W * (diff * diff * diff), 0.0)
        near = d2 <= H2 * (1 + 8 * U)
        out["den"].append(m.sum(axis=1))
        out["num"].append(m @ vel.astype(np.float64))
        out["S"].append(m @ V)
        out["V"].append(near.astype(np.float64) @ V)
        out["K"].append(near.sum(axis=1))
        out["taken"].append(take.sum(axis=1))
        out["marginal"].append((np.abs(d2 - H2) <= 8 * U * H2).sum(axis=1))
    return {k: np.concatenate(v) for k, v in out.items()}


def hold_to_float64(what, ref, den, num, h, dcoef):
    """-> the largest error / bound ratio of den (and of num, where given) against all_pairs' sums"""
    W0 = MASS64 * float(F(dcoef)) * (float(F(h)) ** 2) ** 3
    K = ref["K"].astype(np.float64)
    adds = np.maximum(K - 1, 0)
    assert ref["marginal"].sum() <= 0.01 * ref["taken"].sum(), (what, int(ref["marginal"].sum()), int(ref["taken"].sum()))
    E = K * TERM * U * W0
    bound = E + adds * U * (ref["den"] + E)
    err = np.abs(den.astype(np.float64) - ref["den"])
    assert (err <= bound).all(), f"{what}: den off by {err.max():.3e}"
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert (err[bound == 0] == 0).all()
    if num is not None:
        E = (TERM + 1) * U * W0 * ref["V"]
        bound = E + adds[:, None] * U * (ref["S"] + E)
        err = np.abs(num.astype(np.float64) - ref["num"])
        assert (err <= bound).all(), f"{what}: a numerator off by {err.max():.3e}"
        assert (err[bound == 0] == 0).all()
        if (bound > 0).any():
            ratio = max(ratio, float((err[bound > 0] / bound[bound > 0]).max()))
    return ratio


@pytest.mark.parametrize("name", W.GRIDS)
def test_restatements_against_float64_all_pairs(name):
    c = case(name)
    s, h, D = c["s"], c["h"], c["D"]
    pos, vel = c["pos"], c["vel"]
    # the tracers of every set that lie inside the grid (the others get +0 by definition, whatever lies near them)
    t = np.concatenate(list(c["sets"].values()))
    den = np.concatenate([o["den"] for o in c["out"].values()])
    num = np.concatenate([o["num"] for o in c["out"].values()])
    inside = ~TR.cells_of(t, h, D)[1].any(axis=1)
    ref = all_pairs(t[inside], pos, vel, s.h, s.d_kernel_coeff)
    assert (ref["taken"] > 0).sum() >= 100
    worst = hold_to_float64(f"{name}: tracers", ref, den[inside], num[inside], s.h, s.d_kernel_coeff)
    pairs = int(ref["taken"].sum())
    for k, lattice in c["lat"].items():
        pts = FS.lattice_points(*lattice).reshape(-1, 3)
        inside = ~FS.cells_of(pts, h, D)[1].any(axis=1)
        ref = all_pairs(pts[inside], pos, vel, s.h, s.d_kernel_coeff)
        got = c["fields"][k, "density"].reshape(-1)[inside]
        worst = max(worst, hold_to_float64(f"{name}: lattice {k}", ref, got, None, s.h, s.d_kernel_coeff))
        pairs += int(ref["taken"].sum())
    RATIOS[name] = worst
    print(f"{name}: largest error / bound over {pairs} taken pairs: {worst:.4f}; so far, over all grids: {max(RATIOS.values()):.4f}")
    assert pairs > 1000 and 0 < worst <= 1
