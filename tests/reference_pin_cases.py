"""The cases that pin the oracle -- and through tests/golden/reference_pin.json the strict GPU sweeps -- to the
reference's own kernels executed on the host (oracle/reference.py).  Shared by
tests/test_reference_pin_cpu.py (reference against oracle, needs the reference build), tests/golden/make_golden.py
--reference (writes the digests the reference build produces) and tests/test_gpu_reference_pin.py (the sweeps against
the digests; reads the JSON only).  Every state is seeded numpy; the JSON carries the digest of each input so that a
generator that drew other numbers is reported as such.

Run as a program it is the child process of the comparisons that use the reference's own random setup(): that one
consumes the process's rand() and equals the unseeded sequence only as the first consumer in a fresh process."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import grid_states as G  # noqa: E402
from helpers import bits, dense_block, nasty_state  # noqa: E402
from oracle import oracle as O  # noqa: E402

F = np.float32
PIN_JSON = os.path.join(HERE, "golden", "reference_pin.json")
ARRAYS = ("pos", "vel", "rho", "prs", "force")
DIGESTED = ("pos", "vel", "rho", "prs")          # what sph_download_state returns: the GPU test compares these
H, CELLS = 0.1, 100                              # the reference's own grid
CLICKS = {1: G.CLICK, 2: G.EDGE_CLICKS[0], 3: G.EDGE_CLICKS[1]}


def sha(a):
    """sha256 over the bytes of the C-contiguous float32 array"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


# ---- states ----

def cutoff_state(seed=11):
    """n = 1000 on the reference's grid.  400 base points in eight cells (rho > REST_DENSITY: pressure on); 100 exact
    duplicates (dist = 0) and 100 duplicates 5e-5 away (dist < EPS_F = 1e-4: the pressure and viscosity terms are
    gated out, the density term is not); 100 + 100 partners whose coordinate is the fp32 sum base + 0.1f / base +
    0.0999999f along one axis (the rounded difference falls on either side of h); and 2 x 50 pairs whose difference
    along x is EXACTLY 0.1f and exactly 0.0999999f, the other coordinates equal: dist2 = fl(h * h) exactly, the `>`
    of all three kernels decides.  An exact difference of 0.1f needs both ends on the 2^-27 lattice, so those bases
    sit at x < 0.025 (cell 0, beyond the wall plane like grid_states.state()'s rows, inside the grid) and their
    partners in cell 1; y and z within h / 2, so that pressure is on there too."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(4.0, 4.2, (400, 3)).astype(F)
    dup = base[rng.choice(400, 100, replace=False)].copy()
    near = base[rng.choice(400, 100, replace=False)].copy()
    near[np.arange(100), rng.integers(0, 3, 100)] += F(5e-5)
    parts = [base, dup, near]
    for off in (F(0.1), F(0.0999999)):
        p = base[rng.choice(400, 100, replace=False)].copy()
        p[np.arange(100), rng.integers(0, 3, 100)] += off
        parts.append(p)
    q = F(2.0 ** -27)
    for off in (F(0.1), F(0.0999999)):
        a = np.empty((50, 3), F)
        a[:, 0] = rng.integers(int(0.004 / q), int(0.02 / q), 50).astype(F) * q
        a[:, 1:] = rng.uniform(4.0, 4.05, (50, 2)).astype(F)
        b = a.copy()
        b[:, 0] = a[:, 0] + off
        d = b[:, 0] - a[:, 0]
        assert d.dtype == F and (d == off).all(), "the partners' difference must be exact"
        if off == F(0.1):
            assert (d * d == F(0.1) * F(0.1)).all()
        parts += [a, b]
    pos = np.ascontiguousarray(np.concatenate(parts), dtype=F)
    vel = rng.uniform(-1.0, 1.0, pos.shape).astype(F)
    assert len(pos) == 1000
    G.assert_inside(pos, H, CELLS, "cut-offs")
    return pos, vel


def h_state(h, cells, n=3000, seed=21):
    """grid_states.state() with 1000 rows moved into the 3 x 3 x 3 cells about the middle, so that sums are long"""
    pos, vel = G.state(n, h, cells, seed)
    rng = np.random.default_rng(seed + 100)
    mid = (cells // 2 + 0.5) * h
    pos[:1000] = (mid + rng.uniform(-1.45 * h, 1.45 * h, (1000, 3))).astype(F)
    G.assert_inside(pos, h, cells, f"h = {h}")
    return np.ascontiguousarray(pos), vel


class Case:
    def __init__(self, name, pos, vel, h, cells, steps, clicks=None, dt=None):
        self.name, self.pos, self.vel, self.h, self.cells, self.steps = name, pos, vel, h, cells, steps
        self.clicks = dict(clicks or {})
        self.dt = dt

    def settings(self, factory=None):
        if (self.h, self.cells, self.dt) == (H, CELLS, None):
            return (factory or O.make_settings)(len(self.pos), False)      # the reference's own, main.cpp:57-63
        return G.settings_for(len(self.pos), self.h, self.cells, factory=factory)


def _grid(name):
    pos, vel, g = G.grid_state(name)
    return Case(name, pos, vel, g["h"], g["cells"], 1 if name == "D1" else 4)


def _click(name):
    pos, vel, info = G.click_state(name)
    return Case("click " + name, pos, vel, info["h"], info["cells"], 4, clicks=CLICKS)


def _h(h, cells):
    pos, vel = h_state(h, cells)
    return Case(f"h{h}", pos, vel, h, cells, 4)


def _nasty(which):
    pos, vel = nasty_state(3000, 0) if which == 0 else nasty_state(3000, 50, fast_factor=15.0)
    return Case(f"nasty {which}", pos, vel, H, CELLS, 4)


def _cutoffs():
    pos, vel = cutoff_state()
    return Case("cut-offs", pos, vel, H, CELLS, 4)


BUILDERS = {"cut-offs": _cutoffs}
BUILDERS.update({name: (lambda name=name: _grid(name)) for name in G.GRIDS})
BUILDERS.update({"click " + name: (lambda name=name: _click(name)) for name in G.CLICK_GRIDS})
BUILDERS.update({f"h{h}": (lambda h=h, d=d: _h(h, d)) for h, d in ((0.01, 50), (1.0, 10), (0.2, 32), (0.25, 32))})
BUILDERS.update({f"nasty {w}": (lambda w=w: _nasty(w)) for w in (0, 1)})
JSON_CASES = ["cut-offs", "D2", "D7", "D102", "D257", "click h0.3", "h0.01", "h1.0"]


def case(name):
    return BUILDERS[name]()


# ---- runs ----

def oracle_run(c):
    """-> per step (1-based list index k - 1) the oracle's download and its sorted ids; `before`: the positions each
    step started from"""
    ora = G.oracle_sim(c.settings())
    ora.upload(c.pos, c.vel)
    out = []
    for k in range(1, c.steps + 1):
        before = ora.download()["pos"]
        ora.step()
        ids = ora.sorted_state()["ids"].copy()
        if k in c.clicks:
            ora.click(*c.clicks[k])
        d = ora.download(want_force=True)
        d["ids"], d["before"] = ids, before
        out.append(d)
    ora.close()
    return out


def reference_run(c, oracle_steps, schedule=True):
    """The reference's kernels on the host over the same case, each step in the oracle's order of that step.  Every
    step starts from positions asserted inside the grid (the reference has no bounds check)."""
    from oracle import reference as R
    ref = R.ReferenceSim(len(c.pos), False, settings=c.settings())
    ref.upload(c.pos, c.vel)
    out = []
    for k in range(1, c.steps + 1):
        G.assert_inside(oracle_steps[k - 1]["before"], c.h, c.cells, f"{c.name}: before step {k}")
        if k > 1:
            if differing(out[-1]["pos"], oracle_steps[k - 1]["before"]):
                break                    # the runs parted: the oracle's order no longer applies, the caller reports it
            G.assert_inside(out[-1]["pos"], c.h, c.cells, f"{c.name}: the reference's positions before step {k}")
        ref.step(order=oracle_steps[k - 1]["ids"] if schedule else None, click=c.clicks.get(k))
        out.append(ref.download(want_force=True))
    ref.close()
    return out


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def assert_same_steps(got, want, what, arrays=ARRAYS):
    for k, (g, w) in enumerate(zip(got, want), 1):
        for key in arrays:
            bad = differing(g[key], w[key])
            assert bad == 0, f"{what}, step {k}: {bad} of {w[key].size} words of {key} differ"
    assert len(got) == len(want)


def digests(c, steps):
    """the JSON entry of a case from a run of it"""
    return dict(n=len(c.pos), h=c.h, cells=c.cells, clicks={str(k): list(v) for k, v in sorted(c.clicks.items())},
                input=dict(pos=sha(c.pos), vel=sha(c.vel)),
                steps={str(k): {key: sha(d[key]) for key in DIGESTED} for k, d in enumerate(steps, 1)})


def reference_digests():
    """What make_golden.py --reference writes: every JSON case as the reference build runs it now."""
    out = dict(what="sha256 of the C-contiguous float32 arrays, particle-id order, after each step, as the reference's "
                    "own kernels produce them on the host under the canonical build schedule "
                    "(tests/reference_pin_cases.py; regenerate: python tests/golden/make_golden.py --reference)",
               cases={})
    for name in JSON_CASES:
        c = case(name)
        out["cases"][name] = digests(c, reference_run(c, oracle_run(c)))
    return out


def dump(obj):
    return json.dumps(obj, indent=1, sort_keys=True) + "\n"


def load_pins():
    with open(PIN_JSON) as f:
        return json.load(f)["cases"]


# ---- the child process: the reference's own random setup() ----

def _child(what):
    import ctypes as C
    from oracle import reference as R
    if what == "random-setup":
        n = 1000
        ref = R.ReferenceSim(n, True)
        ref.setup()                                   # the first consumer of rand() in this process
        got = ref.download()
        s = O.make_settings(n, True)
        assert differing(got["pos"], O.init_positions(s)) == 0, "setup() -i random: oracle.init_positions"
        import cudafluidsimulator_amd as sph
        lib_pos = np.zeros((n, 3), F)
        ls = sph.default_settings(n, True)
        assert sph.load_library().sph_initial_positions(C.byref(ls), lib_pos.ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert differing(got["pos"], lib_pos) == 0, "setup() -i random: sph_initial_positions"
        assert not got["vel"].any() and not got["rho"].any() and not got["prs"].any() and not got["force"].any()
    elif what == "random4096":
        gold = np.load(os.path.join(HERE, "golden", "random4096.npz"))
        ref = R.ReferenceSim(4096, True)
        ref.setup()                                   # the first consumer of rand() in this process
        ora = O.OracleSim(4096, True)
        ora.setup()
        run_golden(ref, ora, gold, 100, "random4096")
    else:
        raise SystemExit(f"unknown child {what}")
    print("child ok:", what)


def run_golden(ref, ora, gold, steps, what):
    """Reference and oracle from their initialisers (already run), exact after every step over the five arrays, and
    every array the .npz stores re-derived from the reference's code."""
    assert differing(ref.download()["pos"], ora.download()["pos"]) == 0, f"{what}: initial positions"
    stored = set(gold.files)
    for k in range(1, steps + 1):
        G.assert_inside(ora.download()["pos"], H, CELLS, f"{what}: before step {k}")
        ora.step()
        ref.step(order=ora.sorted_state()["ids"])
        r, o = ref.download(), ora.download(want_force=True)
        for key in ARRAYS:
            bad = differing(r[key], o[key])
            assert bad == 0, f"{what}, step {k}: {bad} of {o[key].size} words of {key} differ"
        for key in ("pos", "vel", "rho"):
            if f"{key}_{k}" in stored:
                assert differing(r[key], gold[f"{key}_{k}"]) == 0, f"{what}: the stored {key}_{k}"
                stored.discard(f"{key}_{k}")
        if f"pos_{k}" in gold.files:
            assert differing(ref.get_position(), gold[f"pos_{k}"]) == 0, f"{what}: getPosition() at step {k}"
    assert not stored, f"{what}: stored arrays never reached: {sorted(stored)}"


if __name__ == "__main__":
    _child(sys.argv[1])
