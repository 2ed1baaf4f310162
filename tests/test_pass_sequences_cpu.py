"""The plans of tests/pass_sequences.py without a GPU: every seed tests/test_gpu_pass_sequences.py runs, walked with the
oracle and the restatements alone.  What the seed list covers as a whole, the floors every pass call must find in the
state it reads, and what the restatements cost (which is what a seed costs on the GPU machine: the kernels take
milliseconds).

Measured with the committed seed list (0 .. 23, six seeds per grid; test_what_the_seed_list_covers prints the tables
under pytest -s).  Seconds on one CPU core, floors included, summed over a grid's seeds / its costliest seed / the
restatements that cost most:
    D7        7.9 /  1.5 (seed 16)   liquid 1.1, measure 0.6, derive 0.5, pairs 0.5, track 0.4
    D10h025  12.3 /  2.5 (seed 13)   measure 1.7, track 0.8, derive 0.8, lists 0.8, label 0.6, pairs 0.6
    D41      22.9 /  4.3 (seed 10)   measure 3.0, derive 2.4, track 1.6, label 0.9, pairs 0.7
    D102     40.1 /  8.6 (seed 23)   measure 5.1, track 4.3, label 2.2, derive 1.1, pairs 1.1
The restatements alone are a third of that: the floors' all-pairs lists and bodies are the rest, and the GPU test does
not compute them.  D102 is thinned first: three of four of its list, label, measure, track and pairs calls take 0.5 h
or 0.3 h, not h (its cluster of a thousand rows within h of each other makes a million entries at radius h); the count
of calls and the kinds of pass are the other grids'.
Pass calls that do work, over the seed list (at least 20 each, asserted): flat 24, field 22, column 23, liquid 25,
sample 24, surface 23, diagnose 23, tracers 20, derive 23, lists 28, label 25, measure 41, track 28, pairs 25 (an advect
of no tracers is not counted).
Re-reads of a reader that holds a result, at once / after a step or an upload since: frame 4 / 10, sample 2 / 2,
surface 2 / 6, diagnose 2 / 9, tracers 0 / 5, derive 0 / 2, lists 1 / 5, bodies 0 / 7, moments 2 / 5, tracks 1 / 5,
pairs 2 / 9.
Pairs calls refused for their options (SPH_EINVAL): 129 bins with and without a table to leave alone (seeds 2, 17), a
radius one ulp above h with and without one (seeds 8 and 11, seed 5); each of the four is asserted to occur.
The draws are seeded with pass_sequences.PLAN_SEED + seed.  PLAN_SEED is the first of 7000, 7001, ... under which
everything this file asserts holds: a fourteenth pass changed every seed's draws, and under 7000 three seeds' plans
took the state below the floors.
"""
import functools
import time

import numpy as np
import pytest

import pass_sequences as PS


class Recorder(PS.Model):
    """the model, noting what every pass call returned: the sizes that grow and shrink on the device"""

    def __init__(self, p):
        super().__init__(p)
        self.sizes = {k: [] for k in ("pixels", "sample", "surface", "tracers", "bodies", "edges", "entries", "moments", "bins")}
        self.floors = []
        self.reached = None

    def apply(self, op):
        super().apply(op)
        self.reached = None

    def floor(self, k, op):
        if self.reached is None:
            self.reached = self.reach()
        self.floors.append((k, op["kind"], self.reached))

    def want(self, op, i, helpers=None, iso=None):
        out = super().want(op, i, helpers, iso)
        kind, s = op["kind"], self.sizes
        if kind in PS.FRAMES:
            s["pixels"].append(op["size"][0] * op["size"][1])
        elif kind == "sample":
            s["sample"].append(out["field"].size)
        elif kind == "surface":
            s["surface"].append(len(out["triangles"]))
        elif kind == "tracers":
            s["tracers"].append(len(out["pos"]))
        elif kind == "lists":
            s["entries"].append(len(out["neighbours"]))
        elif kind == "pairs":
            s["bins"].append(len(out["pairs"]))
        else:
            if "num_bodies" in out:
                s["bodies"].append(out["num_bodies"])
            if "moments" in out:
                s["moments"].append(len(out["moments"]))
            if "join" in out:
                s["edges"].append(out["join"]["summary"]["edges"])
        return out


@functools.lru_cache(maxsize=None)
def walked(seed):
    p = PS.plan(seed)
    model = Recorder(p)
    t0 = time.perf_counter()
    PS.drive(p, model, on_pass=model.floor)
    model.seconds = time.perf_counter() - t0
    model.close()
    return p, model


def test_the_plan_is_a_pure_function_of_the_seed():
    for seed in PS.SEEDS[:4]:
        assert repr(PS.plan(seed)) == repr(PS.plan(seed))
    assert len(PS.SEEDS) == len(set(PS.SEEDS))


@pytest.mark.parametrize("seed", PS.SEEDS)
def test_every_pass_call_finds_the_floors(seed):
    """Conditions on the plans: at every pass call the oracle's state holds at least 20,000 list entries at radius h,
    50 bodies of two or more rows at link 0.3 h and a body of 24 rows.  The clicks and uploads are the plans' own."""
    p, model = walked(seed)
    assert 24 <= len(p["ops"]) <= 30
    assert sum(op["kind"] in PS.STEPPING for op in p["ops"]) <= PS.MAX_STEPS
    assert model.floors
    for k, kind, got in model.floors:
        assert got["entries"] >= PS.MIN_ENTRIES and got["bodies"] >= PS.MIN_BODIES and got["biggest"] >= PS.MIN_BIG_BODY, \
            f"seed {seed} ({p['grid']}), op {k} {kind}: {got}"


def ups_and_downs(values):
    d = np.diff(np.asarray(values, dtype=np.int64))
    return bool((d > 0).any()), bool((d < 0).any())


def test_what_the_seed_list_covers():
    plans = [walked(seed) for seed in PS.SEEDS]
    after, order, inside, frames, sizes, refusals, combos = set(), set(), set(), set(), set(), set(), set()
    options = set()
    fresh, stale = {}, {}       # re-reads of a reader that holds a result: before / after the state has moved on
    calls = {}
    for p, model in plans:
        combos.add((p["grid"], p["env"]["SPH_PIPELINE"]))
        last = None
        for call in PS.passes_of(p):
            op, follows, first, within = call["op"], call["after"], call["first"], call["inside"]
            kind = op["kind"]
            if not call["works"]:
                continue        # (an advect of no tracers returns before it looks at the grid)
            calls[kind] = calls.get(kind, 0) + 1
            if follows:
                after.add((follows, kind))
            order.add((kind, first))
            if within:
                inside.add(kind)
            if kind in PS.FRAMES:
                if last:
                    frames.add((last[0], kind))
                    if last[1] != op["size"]:
                        sizes.add(op["size"])
                last = (kind, op["size"])
        held = {}
        for k, op in enumerate(p["ops"]):
            if op["kind"] == "refuse":
                refusals.add(op["what"])
                if op["what"] == "pair_options":    # (what is wrong with them, does the pairs' reader hold a result)
                    options.add(("bins" if op["bins"] > 128 else "radius", "pairs" in held))
            if op["kind"] == "phases" and op["probe"]:
                refusals.add(f"phase{op['probe'][0]}")
            if op["kind"] == "reread":
                assert op["reader"] in held, f"seed {p['seed']}, op {k}: a re-read of {op['reader']}, which holds nothing"
                count = stale if held[op["reader"]] else fresh
                count[op["reader"]] = count.get(op["reader"], 0) + 1
            PS.follow(held, op)
    missing = [(a, q) for a in PS.AFTER for q in PS.PASSES if (a, q) not in after]
    assert not missing, f"no pass of this kind directly after: {missing}"
    assert inside == set(PS.PASSES)
    assert order == {(q, f) for q in PS.PASSES for f in (True, False)}, "a pass is never the first, or never a later one, of a gap"
    assert frames >= {(a, b) for a in PS.FRAMES for b in PS.FRAMES if a != b}, "a frame kind never follows another"
    assert sizes == set(PS.SIZES), "a frame size never follows a different one"
    assert refusals == set(PS.REFUSALS)
    assert options == {(w, r) for w in ("bins", "radius") for r in (True, False)}, "a refused pairs call: never this option with / without a result to leave alone"
    # every host reader is read again while it holds a result, and at least once after a step or an upload since
    assert set(fresh) | set(stale) == set(PS.READERS), f"never re-read: {sorted(set(PS.READERS) - set(fresh) - set(stale))}"
    assert set(stale) == set(PS.READERS), f"never re-read after the state moved on: {sorted(set(PS.READERS) - set(stale))}"
    assert combos == {(g, v) for g in PS.GRIDS for v in ("0", "1")}
    for what in plans[0][1].sizes:
        up = down = False
        for _, model in plans:
            u, d = ups_and_downs(model.sizes[what])
            up, down = up or u, down or d
        assert up and down, f"{what}: never {'down' if up else 'up'} within a sequence"
    # the coverage and cost tables (pytest -s shows them)
    print("\npass calls over the seed list:", {q: calls[q] for q in PS.PASSES})
    assert min(calls[q] for q in PS.PASSES) >= 20, "a pass makes fewer than 20 working calls over the seed list"
    print("re-reads (at once / after the state moved on):", {r: (fresh.get(r, 0), stale.get(r, 0)) for r in PS.READERS})
    for grid in PS.GRIDS:
        mine = [(p["seed"], m.seconds) for p, m in plans if p["grid"] == grid]
        cost = {}
        for p, m in plans:
            if p["grid"] == grid:
                for k, v in m.cost.items():
                    cost[k] = cost.get(k, 0.0) + v
        print(f"{grid}: {sum(s for _, s in mine):.1f} s over seeds {[s for s, _ in mine]}, costliest seed {max(mine, key=lambda x: x[1])}; "
              + ", ".join(f"{k} {v:.1f}" for k, v in sorted(cost.items(), key=lambda x: -x[1])))
