"""Random call sequences over the fourteen analysis passes: the plan of a seed, the model that says what every call
must return, and the driver that walks a plan.  tests/test_pass_sequences_cpu.py runs the plans with the oracle alone
(what they cover, what they reach, what the restatements cost); tests/test_gpu_pass_sequences.py runs them on a
Simulator.  Imports nothing from the product.

A plan is a list of operations.  State operations move the state (step, timed, phases, open_grid, click, upload,
snapshot); pass operations read it (PASSES; "tracers" is an optional set followed by an advect), "track_reset" forgets
the tracks' reference, "refuse" is a call that must fail and change nothing, "reread" reads a pass's last result again
through its host reader.  The model: the oracle for the state, the passes' restatements for the results, the tracers
and a body_tracks_restatement.Tracker carried across the whole sequence."""
import hashlib
import time

import numpy as np

import bodies_restatement as BR
import body_moments_restatement as M
import body_tracks_restatement as T
import column_frame_restatement as CF
import derived_restatement as DR
import diagnostics_restatement as DG
import field_frame_restatement as FF
import field_sample_restatement as FS
import grid_states as G
import liquid_frame_restatement as LF
import neighbour_restatement as NR
import pair_restatement as PR
import render_restatement as R
import row_walk_cases as RW
import surface_restatement as SR
import tracer_restatement as TR

F = np.float32
SEEDS = list(range(24))
# what a seed's draws are seeded with, less the seed: the first of 7000, 7001, ... with which the seed list covers what
# tests/test_pass_sequences_cpu.py asserts, every pass call finds the floors, and every pass makes 20 working calls
PLAN_SEED = 7160
GRIDS = ("D7", "D10h025", "D41", "D102")
SWEEPS = ("list", "lds", "direct")
# tests/test_gpu_api_fuzz.py's KNOBS (tests/test_gpu_pass_sequences.py asserts that they are)
KNOBS = {"SPH_PIPELINE": ("0", "1"), "SPH_READBACK_SDMA": ("0", "1"),
         "SPH_ZERO_PAIR_FILTER": ("0", "1"), "SPH_SLIM_DIV": ("0", "1"), "SPH_XCD_ROTATE": ("0", "1", "5")}
FRAMES = ("flat", "field", "column", "liquid")
PASSES = FRAMES + ("sample", "surface", "diagnose", "tracers", "derive", "lists", "label", "measure", "track", "pairs")
PLAIN = {"flat": "SPH_RENDER_PLAIN", "field": "SPH_RENDER_PLAIN", "column": "SPH_RENDER_PLAIN", "liquid": "SPH_RENDER_PLAIN",
         "sample": "SPH_SAMPLE_PLAIN", "surface": "SPH_SURFACE_PLAIN", "diagnose": "SPH_DIAG_PLAIN", "tracers": "SPH_TRACER_PLAIN",
         "derive": "SPH_DERIVE_PLAIN", "lists": "SPH_NEIGHBOURS_PLAIN", "label": "SPH_BODIES_PLAIN", "measure": "SPH_BODIES_PLAIN",
         "track": "SPH_BODIES_PLAIN", "pairs": "SPH_PAIRS_PLAIN"}
# the passes under the state rules of analysis_begin: SPH_ESTATE in phases 2 and 3 (the frames and the diagnostics
# read pos4[cur] / vel4[cur] in any phase; what these hold inside a step is not defined, and no plan calls them there)
WALKERS = ("sample", "surface", "tracers", "derive", "lists", "label", "measure", "track", "pairs")
AFTER = ("step", "timed", "click", "upload", "snapshot", "open_grid")   # what every pass must directly follow
STEPPING = ("step", "timed", "click", "snapshot", "open_grid", "phases")
SIZES = ((800, 600), (160, 120), (97, 61))
LATTICES = ((8, 8, 8), (5, 9, 17), (20, 20, 20))       # (nz, ny, nx)
TRACER_COUNTS = (0, 1, 130, 2000)
FIELD_RANGES = {"speed": (0.25, 3.0), "density": (100.0, 1500.0), "pressure": (0.0, 40.0)}
DIAGNOSE = (dict(hist=None, value_range=None), dict(hist="speed", value_range=(0.0, 4.0)), dict(hist="density", value_range=None))
# the pair statistics' table sizes (0 means 32) and, per call, SPH_PAIRS_WORKGROUPS ("0": the default launch; 1 and 3
# workgroups carry their tables across tiles, with other passes' launches between the calls)
PAIR_BINS = (0, 1, 7, 128)
PAIR_WORKGROUPS = ("0", "1", "3")
# "pair_options": a pairs call with 129 bins or a radius just above h, SPH_EINVAL; it leaves the previous result readable
REFUSALS = ("max_edges", "max_bodies", "max_entries", "phase2", "phase3", "pair_options")
# the result a host reader serves again, by pass: sph_frame_host, sph_sample_host, ... ("bodies": sph_bodies_host)
READERS = ("frame", "sample", "surface", "diagnose", "tracers", "derive", "lists", "bodies", "moments", "tracks", "pairs")
GAPS = 8                    # state operations of a seed that the schedule below pairs with the pass that follows them
MAX_STEPS = 16
# the floors of every pass call (conditions on the plans, asserted by tests/test_pass_sequences_cpu.py)
MIN_ENTRIES, MIN_BODIES, MIN_BIG_BODY = 20000, 50, 24
# every (state operation, pass that directly follows it), in a fixed shuffled order: the gaps of consecutive seeds
# take consecutive entries, so the seed list as a whole covers the table whatever the seeds' own draws give
SCHEDULE = [(a, p) for a in AFTER for p in PASSES]
SCHEDULE = [SCHEDULE[i] for i in np.random.default_rng(0).permutation(len(SCHEDULE))]


def radii(h):
    return RW.radii(h)


def above(h):
    """the float32 next above h, as a Python float: the smallest radius the pair statistics refuse"""
    return float(np.nextafter(F(h), F(np.inf)))


def centre(g):
    """the cell corner the cube of row_walk_cases.row_state() is built about, in cells"""
    return min(8, g["cells"] // 2)


def lattice(g, shape):
    """(origin, spacing, shape): the lattice over five cells a side about the cube"""
    h = float(F(g["h"]))
    lo = (centre(g) - 2.5) * h
    nz, ny, nx = shape
    return (lo, lo, lo), tuple(5.0 * h / (k - 1) for k in (nx, ny, nz)), shape


def click_pixel(g, dx, dy):
    """a window pixel whose click (grid_states.click_cell) lands on cell (c + dx, c + dy), c the cube's centre"""
    D, c = g["cells"], centre(g)
    px = G.BOX_MIN_X + int((G.BOX_MAX_X - G.BOX_MIN_X) * (c + dx + 0.5) / D)
    py = G.BOX_MIN_Y + int((G.BOX_MAX_Y - G.BOX_MIN_Y) * (D - c - dy + 0.5) / D)
    return px, py


def draw_pass(rng, name, g, scheduled=False, tracers_set=True, cheap=False):
    """one pass operation with its arguments; scheduled: the call must do work (tracers: some are set)"""
    h = float(g["h"])
    op = dict(kind=name, plain=str(rng.integers(2)))
    size = SIZES[rng.integers(3)]
    if name == "flat":
        op.update(size=size, point_size=int(rng.choice([1, 3, 9])), shade=str(rng.choice(["flat", "count"])))
    elif name == "field":
        field = str(rng.choice(FS.FIELDS))
        op.update(size=size, point_size=int(rng.choice([1, 3, 9])), field=field, range=FIELD_RANGES[field] if rng.integers(2) else (0.0, 0.0))
    elif name == "column":
        op.update(size=size, range=(0.25, 2.0) if rng.integers(2) else (0.0, 0.0))
    elif name == "liquid":
        op.update(size=size, smooth=int(rng.choice([0, 2])))
    elif name == "sample":
        op.update(field=str(rng.choice(FS.FIELDS)), shape=LATTICES[rng.integers(3)])
    elif name == "surface":
        op.update(shape=LATTICES[rng.integers(3)])
    elif name == "diagnose":
        op.update(DIAGNOSE[rng.integers(3)])
    elif name == "tracers":
        counts = TRACER_COUNTS[1:] if scheduled else TRACER_COUNTS
        setting = (not tracers_set) or rng.integers(3) == 0
        op.update(set=(int(rng.choice(counts)), int(rng.integers(1 << 30))) if setting else None, dt=None if rng.integers(2) else 0.0)
    elif name == "lists":
        op.update(radius=radii(h)[rng.integers(3)], walk_order=bool(rng.integers(2)))
    elif name in ("label", "measure"):
        op.update(link=radii(h)[rng.integers(3)])
    elif name == "track":
        op.update(link=radii(h)[rng.integers(3)], moments=bool(rng.integers(2)))
    elif name == "pairs":
        op.update(bins=int(PAIR_BINS[rng.integers(4)]), radius=radii(h)[rng.integers(3)], workgroups=PAIR_WORKGROUPS[rng.integers(3)])
    if cheap and name in ("lists", "label", "measure", "track", "pairs"):
        # D102's cluster: a thousand rows within h of each other, a million entries at radius h
        op["radius" if name in ("lists", "pairs") else "link"] = radii(h)[1 + rng.integers(2)]
    return op


def readers_of(op):
    """the host readers a successful pass call fills"""
    kind = op["kind"]
    if kind in FRAMES:
        return ("frame",)
    if kind == "label":
        return ("bodies",)
    if kind == "measure":
        return ("bodies", "moments")
    if kind == "track":
        return ("bodies", "tracks", "moments") if op["moments"] else ("bodies", "tracks")
    return (kind,)


def follow(held, op):
    """held: reader -> has the state moved since the result it holds was made; updated for one operation of a plan, as
    tests/test_gpu_pass_sequences.py's Device keeps `last`.  A call refused by a cap empties its own reader (and has
    labelled); a pairs call refused for its options leaves the pairs' reader as it was."""
    kind = op["kind"]

    def called(q):
        for r in readers_of(q):
            held[r] = False

    if kind in PASSES:
        called(op)
    elif kind == "track_reset":
        held.pop("tracks", None)
    elif kind == "refuse":
        if op["what"] == "pair_options":
            pass
        elif op["what"] == "max_entries":
            held.pop("lists", None)
        else:
            held["bodies"] = False
            held.pop("tracks" if op["what"] == "max_edges" else "moments", None)
            if op["what"] == "max_edges" and op["moments"]:
                held.pop("moments", None)
        called(op["then"])
    elif kind in STEPPING or kind == "upload":
        for q in op.get("passes", ()):
            called(q)
        for r in held:
            held[r] = True


def plan(seed):
    """-> dict(seed, grid, sweep, env, ops): a pure function of the seed"""
    rng = np.random.default_rng(PLAN_SEED + seed)
    grid = GRIDS[seed % 4]
    g = G.GRIDS[grid]
    sweep = SWEEPS[rng.integers(3)]
    env = {k: str(rng.choice(v)) for k, v in KNOBS.items()}
    env["SPH_PIPELINE"] = str((seed // 4) % 2)         # every grid with both values over the seeds 0 .. 7, 8 .. 15, ...
    heavy = grid == "D102"
    n_ops = int(rng.integers(24, 31))
    # how many extra operations follow each gap's first pass
    extras = np.zeros(GAPS, np.int64)
    ops, steps = [], 0
    state = dict(tracers=False, reference=False)
    held = {}

    def a_pass(name, scheduled=False):
        op = draw_pass(rng, name, g, scheduled, state["tracers"], cheap=heavy and rng.integers(4) != 0)
        if name == "tracers" and op["set"] is not None:
            state["tracers"] = True
        if name == "track":
            state["reference"] = True
        return op

    def a_state(kind):
        nonlocal steps
        op = dict(kind=kind)
        if kind == "click":
            op["pixel"] = click_pixel(g, int(rng.integers(-1, 2)), int(rng.integers(-1, 2)))
        elif kind == "upload":
            op.update(what=str(rng.choice(["walls", "jitter"])), seed=int(rng.integers(1 << 30)))
        elif kind == "open_grid":
            op["passes"] = []
        elif kind == "phases":
            op["probe"] = None
        steps += kind in STEPPING
        return op

    def an_extra():
        kind = str(rng.choice(["pass"] * 8 + ["reread"] * 6 + ["refuse"] * 3 + ["track_reset", "phases", "step"]))
        if kind == "pass":
            return a_pass(PASSES[rng.integers(len(PASSES))])
        if kind == "reread":
            # among the readers that hold a result; three times in four among those whose result the state has left behind
            stale = sorted(r for r, moved in held.items() if moved)
            pool = stale if stale and rng.integers(4) else sorted(held)
            if not pool:
                return a_pass(PASSES[rng.integers(len(PASSES))])
            return dict(kind="reread", reader=pool[rng.integers(len(pool))])
        if kind == "track_reset":
            state["reference"] = False
            return dict(kind="track_reset")
        if kind == "refuse":
            what = REFUSALS[rng.integers(len(REFUSALS))]
            if what == "max_edges" and not state["reference"]:
                what = "max_bodies"
            if what in ("phase2", "phase3"):          # a step by hand with a pass where none is legal
                op = a_state("phases")
                probe = draw_pass(rng, WALKERS[rng.integers(len(WALKERS))], g, tracers_set=True, cheap=True)
                if probe["kind"] == "tracers":
                    probe["set"] = None               # (sph_tracers_set has no state rule: the advect alone is refused)
                op["probe"] = (int(what[-1]), probe)
                return op
            if what == "pair_options":         # SPH_EINVAL: too many bins, or a radius one ulp above h
                bad = dict(bins=129, radius=0.0) if rng.integers(2) else dict(bins=int(PAIR_BINS[rng.integers(4)]), radius=above(g["h"]))
                op = dict(kind="refuse", what=what, plain=str(rng.integers(2)), **bad)
                op["then"] = a_pass("pairs")
                return op
            link = radii(g["h"])[2]
            op = dict(kind="refuse", what=what, link=link, moments=bool(rng.integers(2)), plain=str(rng.integers(2)))
            # ... and the next successful call of that pass straight after it: it must equal the model, which the
            # refusal left alone
            op["then"] = a_pass({"max_edges": "track", "max_bodies": "measure", "max_entries": "lists"}[what])
            return op
        return a_state(kind)

    scheduled = [SCHEDULE[(seed * GAPS + k) % len(SCHEDULE)] for k in range(GAPS)]
    total = 2 * GAPS - sum(1 for a, _ in scheduled if a == "open_grid")
    for _ in range(n_ops - total):
        extras[rng.integers(GAPS)] += 1
    for k, (after, first) in enumerate(scheduled):
        op = a_state(after)
        ops.append(op)
        if after == "open_grid":
            op["passes"].append(a_pass(first, scheduled=True))
            for _ in range(int(rng.integers(3))):
                op["passes"].append(a_pass(PASSES[rng.integers(len(PASSES))]))
            follow(held, op)
        else:
            follow(held, op)
            ops.append(a_pass(first, scheduled=True))
            follow(held, ops[-1])
        for _ in range(int(extras[k])):
            ops.append(an_extra() if steps < MAX_STEPS else a_pass(PASSES[rng.integers(len(PASSES))]))
            follow(held, ops[-1])
    assert 24 <= len(ops) <= 30 and steps <= MAX_STEPS, (seed, len(ops), steps)
    return dict(seed=seed, grid=grid, sweep=sweep, env=env, ops=ops)


def describe(op):
    return op["kind"] + " " + ", ".join(f"{k}={v}" for k, v in op.items() if k not in ("kind", "passes", "probe", "then"))


# ---- the model ----

def words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def assert_same(got, want, what):
    """two results, name -> array / number, byte for byte"""
    assert set(want) <= set(got), f"{what}: {sorted(set(want) - set(got))} missing"
    for k, b in want.items():
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            bad = (words(a) != words(b)).reshape(-1, a.dtype.itemsize).any(axis=1)
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries of {k} differ, first at {int(np.flatnonzero(bad)[0])}")


class Inputs:
    """what a restatement is fed with: the state in id order and the grid that was walked"""

    def __init__(self, st, ids, cells):
        self.pos, self.vel, self.rho = st["pos"], st["vel"], st["rho"]
        self.ids = np.asarray(ids).astype(np.int64)
        self.cells = cells
        self.rows, self.vrows, self.rrows = self.pos[self.ids], self.vel[self.ids], self.rho[self.ids]

    def key(self):
        d = hashlib.sha1()
        for a in (self.pos, self.vel, self.rho, self.ids, self.cells):
            d.update(np.ascontiguousarray(a).tobytes())
        return d.digest()


class Model:
    def __init__(self, p):
        self.plan = p
        self.name = p["grid"]
        pos, vel, self.g = RW.row_state(self.name)
        self.start = (pos, vel)
        self.s = G.settings_for(len(pos), self.g["h"], self.g["cells"])
        self.h, self.D, self.coeff = self.s.h, int(self.s.numCellsPerDim), self.s.d_kernel_coeff
        self.ref = G.oracle_sim(self.s)
        self.ref.upload(pos, vel)
        self.tracers = np.zeros((0, 3), F)
        self.tracker = T.Tracker()
        self.fields = {}
        self.prepared = {}
        self.cost = {}

    def close(self):
        self.ref.close()

    # -- the state --
    def upload_of(self, op):
        """the state an upload operation uploads"""
        if op["what"] == "walls":
            pos, vel, _ = RW.walls(self.name)
            return pos, vel
        pos, vel = self.start[0].copy(), self.start[1].copy()
        rng = np.random.default_rng(op["seed"])
        top = np.nextafter(G.box_of(self.h, self.D), F(0))
        pos = np.clip((pos + rng.uniform(-0.02, 0.02, pos.shape) * float(self.h)).astype(F), F(0), top)
        G.assert_inside(pos, self.h, self.D, "a jittered upload")
        return np.ascontiguousarray(pos), vel

    def apply(self, op):
        """a state operation on the oracle (phases and open_grid: the step they make; snapshot: nothing, the handle
        comes back to where it was)"""
        kind = op["kind"]
        if kind in ("step", "timed", "phases", "open_grid"):
            self.ref.step()
        elif kind == "click":
            self.ref.step()
            self.ref.click(*op["pixel"])
        elif kind == "upload":
            self.ref.upload(*self.upload_of(op))
        else:
            assert kind == "snapshot", kind

    def inputs(self):
        """the oracle's state over a grid built on the CPU (the product's grid is the same stable sort)"""
        st = self.ref.download()
        _, ids, cells = NR.grid_of(st["pos"], self.h, self.D)
        return Inputs(st, ids, cells)

    def assert_sorted(self, i, tag):
        """the grid a walker left behind sph_download_grid is a stable sort of the downloaded state by cell: every id
        once, the rows' cells in ascending order -- the CPU sort's sequence of cells; the product sorts the previous
        step's order, not the id order, so the rows of one cell may stand in another order than the CPU's --, the CPU's
        run for every occupied cell and no rows in any other"""
        _, ids, cells = NR.grid_of(i.pos, self.h, self.D)
        c = BR.row_cells(i.pos, self.h, self.D).astype(np.int64)
        key = (c[:, 2] * self.D + c[:, 1]) * self.D + c[:, 0]
        assert np.array_equal(np.sort(i.ids), np.arange(len(i.pos))), f"{tag}: sph_download_grid's ids are not a permutation of the ids"
        assert np.array_equal(key[i.ids], key[ids]), f"{tag}: sph_download_grid's ids are not sorted by the cells of the state"
        got = np.asarray(i.cells).reshape(-1, 2)
        assert got.shape == cells.shape, f"{tag}: {got.shape} cell ranges"
        full = cells[:, 1] > cells[:, 0]
        assert np.array_equal(got[full], cells[full]) and (got[~full, 1] <= got[~full, 0]).all(), f"{tag}: sph_download_grid's cell ranges are not the state's"

    def pairs(self, i, radius):
        key = (i.key(), radius)
        if key not in self.prepared:
            self.prepared.clear()           # (the calls on one state follow each other)
            self.prepared[key] = PR.prepared(i.pos, i.vel, self.h, radius)
        return self.prepared[key]

    def walks(self, op):
        """does this pass call find or build the grid of the state (sph_download_grid then returns the one it walked)?
        The frames and the diagnostics read the state alone; an advect of no tracers returns before it looks."""
        if op["kind"] == "tracers":
            return (op["set"][0] if op["set"] is not None else len(self.tracers)) > 0
        return op["kind"] in WALKERS

    def reach(self):
        """what the floors are about, of the oracle's state"""
        i = self.inputs()
        offsets, _ = NR.all_pairs(i.pos, self.h, 0.0)
        count = BR.bodies(i.rows, i.ids, i.cells, self.h, self.D, 0.3 * float(self.h))["table"][:, 1]
        return dict(entries=int(offsets[-1]), bodies=int((count >= 2).sum()), biggest=int(count.max()))

    # -- the passes --
    def tracers_of(self, op):
        m, seed = op["set"]
        lo, _, _ = lattice(self.g, LATTICES[0])
        rng = np.random.default_rng(seed)
        return np.ascontiguousarray((lo[0] + 5.0 * float(F(self.h)) * rng.random((m, 3))).astype(F))

    def field(self, i, name, lat):
        key = (i.key(), name, lat)
        if key not in self.fields:
            if len(self.fields) > 8:
                self.fields.clear()
            self.fields[key] = FS.sample(i.rows, i.vrows, i.rrows, i.cells, self.h, self.coeff, self.D, name, *lat)
        return self.fields[key]

    def iso(self, op):
        """the level of a surface operation: half the maximum of the density sampled on its lattice (of the state
        before the call, which the call does not change)"""
        return float(F(0.5) * self.field(self.inputs(), "density", lattice(self.g, op["shape"])).max())

    def bodies(self, i, link, helpers):
        if helpers and "bodies" in helpers:
            return helpers["bodies"](link)
        return BR.bodies(i.rows, i.ids, i.cells, self.h, self.D, link)

    def want(self, op, i, helpers=None, iso=None):
        """the result of a pass operation over the inputs i -> name -> array; the tracers and the tracker move on.
        helpers: name -> function of the passes' own test files that restates from the handle ("derive", "bodies",
        "walk")"""
        t0 = time.perf_counter()
        out = self._want(op, i, helpers or {}, iso)
        self.cost[op["kind"]] = self.cost.get(op["kind"], 0.0) + time.perf_counter() - t0
        return out

    def _want(self, op, i, helpers, iso):
        kind = op["kind"]
        h, D, coeff = self.h, self.D, self.coeff
        if kind in FRAMES:
            w, ht = op["size"]
        if kind == "flat":
            return R.render(i.pos, width=w, height=ht, point_size=op["point_size"], shade=op["shade"])
        if kind == "field":
            r = FF.render_field(i.pos, i.vel, i.rho, field=op["field"], lo=op["range"][0], hi=op["range"][1], width=w, height=ht,
                                point_size=op["point_size"])
            r["range"] = np.array(r["range"], F)
            return r
        if kind == "column":
            r = CF.render_column(i.pos, h, coeff, lo=op["range"][0], hi=op["range"][1], width=w, height=ht)
            assert r.pop("border") == 0, "a contribution on the border of the restatement's box"
            del r["edge"]
            r["range"] = np.array(r["range"], F)
            return r
        if kind == "liquid":
            r = LF.render_liquid(i.pos, h, coeff, smooth_iterations=op["smooth"], width=w, height=ht)
            assert r["border"] == 0, "a contribution on the border of the restatement's box"
            return {k: r[k] for k in ("front", "column", "smooth", "normals", "rgb")}
        if kind == "sample":
            return dict(field=self.field(i, op["field"], lattice(self.g, op["shape"])), dims=np.array(op["shape"]))
        if kind == "surface":
            lat = lattice(self.g, op["shape"])
            v, t, _ = SR.extract(self.field(i, "density", lat), lat[0], lat[1], iso)
            return dict(vertices=v, triangles=t)
        if kind == "diagnose":
            return dict(raw=DG.restate(i.pos, i.vel, i.rho, hist=op["hist"], value_range=op["value_range"]))
        if kind == "tracers":
            if op["set"] is not None:
                self.tracers = self.tracers_of(op)
            dt = self.s.timestep if op["dt"] is None else op["dt"]
            r = TR.advect(i.rows, i.vrows, i.cells, h, coeff, D, self.tracers, dt)
            self.tracers = r["pos"]
            return {k: r[k] for k in ("pos", "den", "vel")}
        if kind == "derive":
            if "derive" in helpers:
                return helpers["derive"]()
            rows = DR.derive(i.rows, i.vrows, i.cells, h, coeff, D)
            out = {}
            for k in ("vorticity", "divergence", "grad_rho", "rho", "neighbours"):
                out[k] = np.empty_like(rows[k])
                out[k][i.ids] = rows[k]
            return out
        if kind == "lists":
            if op["walk_order"]:
                r = helpers["walk"](op["radius"]) if "walk" in helpers else NR.walk_order(i.rows, i.ids, i.cells, h, D, op["radius"])
            else:
                r = NR.all_pairs(i.pos, h, op["radius"])
            return dict(offsets=r[0], neighbours=r[1])
        if kind == "pairs":
            return self.pairs(i, op["radius"]).table(PR.edges2(op["radius"], h, op["bins"]))
        b = self.bodies(i, op["link"], helpers)
        out = {k: b[k] for k in ("labels", "table", "num_bodies", "largest")}
        if kind == "measure" or (kind == "track" and op["moments"]):
            bodies = M.restate(i.pos, i.vel, i.rho, b["labels"])
            out.update(moments=M.to_rows(bodies), size_hist=M.size_hist(bodies))
        if kind == "track":
            out["join"] = self.tracker.call(b["labels"])
        else:
            assert kind in ("label", "measure"), kind
        return out

    def refused(self, op, i, helpers=None):
        """what a call refused by a cap leaves: the labelling it made (max_bodies, max_edges), nothing else; a pairs call
        refused for its options (which i may be None for: it walks no grid) leaves nothing and takes nothing"""
        if op["what"] in ("max_entries", "pair_options"):
            return None
        b = self.bodies(i, op["link"], helpers or {})
        if op["what"] == "max_edges":
            before = (self.tracker.next_track, self.tracker.sequence)
            assert self.tracker.labels is not None and self.tracker.call(b["labels"], max_edges=1) is None, "premise: the call is refused"
            assert before == (self.tracker.next_track, self.tracker.sequence)
        else:
            assert b["num_bodies"] > 1, "premise: the call is refused"
        return {k: b[k] for k in ("labels", "table", "num_bodies", "largest")}


# ---- the driver ----

def passes_of(p):
    """every pass call of a plan in order, as dicts: k (operation number), op, after (the kind of the state operation it
    directly follows, else None), first (no pass that walks the grid came before it in its gap: a walker then builds the
    grid ahead, or finds the open phase's; a later one finds what that one built), inside (within an open grid phase),
    works (False for an advect of no tracers, which returns before it looks at the grid)"""
    out, after, first, m = [], None, True, 0

    def note(k, q, after, inside):
        nonlocal first, m
        if q["kind"] == "tracers" and q["set"] is not None:
            m = q["set"][0]
        works = not (q["kind"] == "tracers" and m == 0)
        out.append(dict(k=k, op=q, after=after, first=first, inside=inside, works=works))
        if works and q["kind"] in WALKERS:
            first = False

    for k, op in enumerate(p["ops"]):
        kind = op["kind"]
        if kind == "open_grid":
            first = True
            for j, q in enumerate(op["passes"]):
                note(k, q, "open_grid" if j == 0 else None, True)
            after, first = "open_grid", True
        elif kind in PASSES:
            note(k, op, after, False)
            after = None
        elif kind in STEPPING or kind == "upload":
            after, first = kind, True
        else:
            if kind == "refuse":
                if op["what"] != "pair_options":
                    first = False       # (the call walked the grid before a cap refused it; bad options are refused before)
                note(k, op["then"], None, False)
            after = None            # a refusal, a reread or a reset stands between
    return out


def drive(p, model, device=None, bare=None, on_pass=None):
    """Walk a plan: the model always; device: the handle under test, an object with apply(op), phase(name), call(op, iso)
    -> result, refuse(op), probe(op), reread(reader, tag), inputs(walked) -> Inputs, helpers(), check(model, tag),
    compare(op, got, want, tag), reset(); bare: the handle that makes the state operations only (apply, phase);
    on_pass(k, op): called before every pass call (the oracle holds the state the pass reads)."""
    what = f"seed {p['seed']} ({p['grid']}, {p['sweep']}, {p['env']})"

    def a_pass(k, op, tag):
        if on_pass:
            on_pass(k, op)
        iso = model.iso(op) if op["kind"] == "surface" else None
        if device is None:
            model.want(op, model.inputs(), iso=iso)
            return
        got = device.call(op, iso)
        i = device.inputs(model.walks(op))
        if op["kind"] == "pairs":
            model.assert_sorted(i, tag)
        try:
            want = model.want(op, i, device.helpers(), iso)
        except AssertionError as e:     # (a restatement that cannot make sense of the grid and the state it was given)
            raise AssertionError(f"{tag}: the restatement over sph_download_grid + sph_download_state after the call: {e}") from e
        device.compare(op, got, want, tag)

    for k, op in enumerate(p["ops"]):
        kind = op["kind"]
        tag = f"{what}, op {k} {describe(op)}"
        if kind in PASSES:
            a_pass(k, op, tag)
        elif kind == "track_reset":
            model.tracker.reset()
            if device:
                device.reset(tag)
        elif kind == "reread":
            if device:
                device.reread(op["reader"], tag)
        elif kind == "refuse":
            if device is None:
                model.refused(op, model.inputs())
            else:
                device.refuse(op, tag)
                i = None if op["what"] == "pair_options" else device.inputs(True)
                device.refused(op, model.refused(op, i, device.helpers()), tag)
            a_pass(k, op["then"], f"{tag}: the next call, {describe(op['then'])}")
        elif kind in ("open_grid", "phases"):
            for d in (device, bare):
                if d:
                    d.phase("grid")
            for j, q in enumerate(op.get("passes", ())):
                a_pass(k, q, f"{tag}, inside the open grid phase: pass {j} {describe(q)}")
            for number, name in ((2, "density"), (3, "force")):
                for d in (device, bare):
                    if d:
                        d.phase(name)
                if device and op.get("probe") and op["probe"][0] == number:
                    device.probe(op["probe"][1], f"{tag}: in phase {number}, {describe(op['probe'][1])}")
            for d in (device, bare):
                if d:
                    d.phase("readback")
            model.apply(op)
        else:
            model.apply(op)
            for d in (device, bare):
                if d:
                    d.apply(op, model, k)
        if device and (kind in STEPPING or kind == "upload"):
            device.check(model, tag)
