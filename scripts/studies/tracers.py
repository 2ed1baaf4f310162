#!/usr/bin/env python3
"""GPU time of a tracer advect (sph_tracers_advect) on one state: n particles after `steps` steps, m tracers, two
seedings -- a blob of 0.5^3 inside the floor pile, and one tracer per particle id k n / m -- on the default path
(key + sort + shared / direct walk) and on the check path (SPH_TRACER_PLAIN=1).  Every leg is
SphTracerStats.seconds (HIP events around key + sort + walk) over `calls` advects with dt = 0, so the tracers stay
where they are; the legs alternate over `rounds` rounds and the median round is reported, with its minimum and
maximum as the run-to-run spread.  Beside it the yardstick field_sample.py names: the density sweep two steps on,
in ns per candidate test.  A tracer's candidate tests are the rows of the 27 cells around its own, counted on the
host from the cell table.
  python scripts/studies/tracers.py [--n N] [--steps K] [--m M] [--out FILE.json]
SPH_LIB_PATH selects another build of the library (make variant EXTRA=-DTRACER_MAX_GROUPS=G moves the threshold)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--m", type=int, default=65536)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

F = np.float32
D = 100


def box3(a, axis):
    """a[i - 1] + a[i] + a[i + 1] along `axis`, zero beyond the ends"""
    pad = [(1, 1) if k == axis else (0, 0) for k in range(a.ndim)]
    b = np.pad(a, pad)
    sl = lambda lo, hi: tuple(slice(lo, hi) if k == axis else slice(None) for k in range(a.ndim))
    n = a.shape[axis]
    return b[sl(0, n)] + b[sl(1, n + 1)] + b[sl(2, n + 2)]


def seedings(pos):
    """name -> (m, 3) float32"""
    n = len(pos)
    y0 = float(np.percentile(pos[:, 1], 1.0))                        # the floor pile (early on: the lowest fluid there is)
    pile = pos[(pos[:, 1] >= y0) & (pos[:, 1] < y0 + 0.5)]
    cx, cz = (float(np.median(pile[:, a])) for a in (0, 2))
    lo = np.array([min(max(cx - 0.25, 0.0), 9.5), min(y0, 9.5), min(max(cz - 0.25, 0.0), 9.5)])
    blob = np.ascontiguousarray(lo + 0.5 * np.random.default_rng(1).random((args.m, 3)), dtype=F)
    ids = (np.arange(args.m, dtype=np.int64) * n) // args.m
    return {"blob_0.5^3": blob, "one_per_particle_id": np.ascontiguousarray(pos[ids])}


def measure(sim):
    seeds = seedings(sim.download_state()["pos"])
    legs = [(w, plain) for w in seeds for plain in (False, True)]
    per_leg = {leg: [] for leg in legs}
    counted = {}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up
        for leg in legs:
            w, plain = leg
            os.environ["SPH_TRACER_PLAIN"] = "1" if plain else "0"
            sim.set_tracers(seeds[w])
            sim.sync()
            sim.tracer_stats(reset=True)
            for _ in range(args.calls):
                sim.advect_tracers(0.0)
            st = sim.tracer_stats(reset=True)
            assert st["calls"] == args.calls
            if rnd:
                per_leg[leg].append(1e3 * st["seconds"] / args.calls)
                counted[leg] = {k: st[k] // args.calls for k in ("waves_shared", "waves_direct", "groups")}
    cells = sim.download_grid()["cells"].astype(np.int64)
    around = box3(box3(box3((cells[:, 1] - cells[:, 0]).reshape(D, D, D), 0), 1), 2)
    row = {}
    for (w, plain), v in per_leg.items():
        t = seeds[w]
        c = (t / F(sim.settings.h)).astype(np.int64)
        inside = ((t >= 0) & (c < D)).all(axis=1)
        tests = int(around[c[inside, 2], c[inside, 1], c[inside, 0]].sum())
        ms = statistics.median(v)
        r = {"ms_per_advect_median": ms, "min": min(v), "max": max(v), "candidate_tests": tests,
             "ns_per_candidate_test": 1e6 * ms / tests if tests else None}
        if not plain:
            r.update(counted[(w, plain)])
        row[w + ("_plain" if plain else "_default")] = r
    # the yardstick, as in field_sample.py: the step right after consumes the grid built ahead, whose event span holds
    # the advects; the step after that is a step of its own
    sim.set_tracers(np.zeros((0, 3), F))
    sim.simulate()
    sim.kernel_times(reset=True)
    sim.simulate()
    kt = sim.kernel_times(reset=True)
    assert kt.steps == 1
    cells = sim.download_grid()["cells"].astype(np.int64)
    count = (cells[:, 1] - cells[:, 0]).reshape(D, D, D)
    sweep_tests = int((count * box3(box3(box3(count, 0), 1), 2)).sum())
    row["density_sweep_two_steps_on"] = {"ms": 1e3 * kt.density, "candidate_tests": sweep_tests,
                                         "ns_per_candidate_test": 1e9 * kt.density / sweep_tests}
    return row


sim = sph.Simulator(sph.default_settings(args.n, True), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "m": args.m, "calls_per_round": args.calls, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    out["after_step_%d" % steps] = measure(sim)
    done += 2  # (the yardstick's steps)
    print(json.dumps({("after_step_%d" % steps): out["after_step_%d" % steps]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
