#!/usr/bin/env python3
"""GPU time of the run diagnostics (sph_diagnose) on one state: n particles after setup and after `steps` steps,
with and without a histogram, production path and plain path (SPH_DIAG_PLAIN=1).  Every leg is the diagnostics
launches alone, from sph_get_diagnostics_time; the legs alternate over `rounds` rounds of `calls` calls and the
median round is reported.  Beside it two yardsticks: 32 bytes x n over the HBM peak, and the wall time of what the
same numbers cost without the feature -- sph_download_state plus a numpy pass over the arrays (float64 sums, minima
and maxima, a histogram; NOT the exact Python-int restatement of the tests, which is far slower).
  python scripts/studies/diagnostics.py [--n N] [--steps K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--hbm-peak-tbs", type=float, default=8.0, help="HBM3E peak of the MI355X, TB/s")
ap.add_argument("--out", default=None)
args = ap.parse_args()

LEGS = [(hist, plain) for hist in (None, "speed") for plain in (False, True)]


def host_pass(sim):
    """what a user does without sph_diagnose: download 32 bytes per particle, reduce with numpy"""
    t0 = time.perf_counter()
    st = sim.download_state()
    t1 = time.perf_counter()
    pos, vel, rho = (st[k].astype(np.float64) for k in ("pos", "vel", "rho"))
    v2 = (vel * vel).sum(axis=1)
    out = [pos.sum(axis=0), vel.sum(axis=0), rho.sum(), st["prs"].astype(np.float64).sum(), v2.sum(),
           pos.min(axis=0), pos.max(axis=0), rho.min(), rho.max()]
    speed = np.sqrt(v2)
    out += [speed.max(), np.histogram(speed, 256)[0]]
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def measure(sim):
    per_leg = {leg: [] for leg in LEGS}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up
        for leg in LEGS:
            hist, plain = leg
            os.environ["SPH_DIAG_PLAIN"] = "1" if plain else "0"
            sim.sync()
            sim.diagnostics_time(reset=True)
            for _ in range(args.calls):
                sim.diagnose(hist)
            sim.diagnostics_raw()
            sec, calls = sim.diagnostics_time(reset=True)
            assert calls == args.calls
            if rnd:
                per_leg[leg].append(1e6 * sec / calls)
    row = {}
    for (hist, plain), v in per_leg.items():
        name = ("plain" if plain else "production") + ("_with_histogram" if hist else "")
        row[name] = {"us_per_call_median": statistics.median(v), "min": min(v), "max": max(v)}
    host = [host_pass(sim) for _ in range(4)][1:]
    row["host_download_state_ms_median"] = 1e3 * statistics.median(h[0] for h in host)
    row["host_numpy_pass_ms_median"] = 1e3 * statistics.median(h[1] for h in host)
    os.environ["SPH_DIAG_PLAIN"] = "0"
    walls = []
    for _ in range(5):  # queue, wait, derive: what the caller of Simulator.diagnostics() waits for
        sim.sync()
        t0 = time.perf_counter()
        sim.diagnostics("speed")
        walls.append(1e3 * (time.perf_counter() - t0))
    row["diagnostics_call_wall_ms_median"] = statistics.median(walls[1:])
    return row


sim = sph.Simulator(sph.default_settings(args.n, True))
sim.setup()
out = {"n": args.n, "calls_per_round": args.calls, "rounds": args.rounds, "library": os.path.basename(sph.library_path()),
       "bytes_read": 32 * args.n, "hbm_peak_tbs": args.hbm_peak_tbs,
       "us_at_hbm_peak": 32 * args.n / (args.hbm_peak_tbs * 1e12) * 1e6}
done = 0
for steps in sorted({0, args.steps}):
    while done < steps:
        sim.simulate()
        done += 1
    key = "after_setup" if steps == 0 else "after_step_%d" % steps
    out[key] = measure(sim)
    print(json.dumps({key: out[key]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
