#!/usr/bin/env python3
"""GPU time of the derived-field sweep (sph_derive) on one state: n particles after `early` and after `steps` steps,
on the default path (one wave per 64 sorted rows, runs staged in LDS) and on the check path (SPH_DERIVE_PLAIN=1).
Every leg is SphDeriveStats.seconds (HIP events around the sweep) over `calls` derives; the legs alternate over
`rounds` rounds and the median round is reported, with its minimum and maximum as the run-to-run spread.  Beside
both the yardstick: the density sweep of the step that consumes a grid of the same state (SphKernelTimes.density).
The derives' own kernels land in the event span of the step that consumes their grid, so the state is downloaded,
uploaded again -- which drops that grid -- and stepped once with nothing in between.
  python scripts/studies/derived.py [--n N] [--steps K] [--early K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library (-DDERIVE_SLICE=... moves the LDS slice)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--out", default=None)
args = ap.parse_args()


def measure(sim):
    per_leg = {False: [], True: []}
    runs = {}
    for rnd in range(args.rounds + 1):  # round 0 warms both legs up (and builds the grid ahead)
        for plain in (False, True):
            os.environ["SPH_DERIVE_PLAIN"] = "1" if plain else "0"
            sim.sync()
            sim.derive_stats(reset=True)
            for _ in range(args.calls):
                sim._check(sim._L.sph_derive(sim._h), "sph_derive")
            st = sim.derive_stats(reset=True)
            assert st["calls"] == args.calls
            if rnd:
                per_leg[plain].append(1e3 * st["seconds"] / args.calls)
            if not plain:
                runs = {k: st[k] // args.calls for k in ("runs_staged", "runs_direct")}
    os.environ["SPH_DERIVE_PLAIN"] = "0"
    fields = sim.derive()
    row = {}
    for plain, v in per_leg.items():
        row["plain" if plain else "default"] = {"ms_per_derive_median": statistics.median(v), "min": min(v), "max": max(v)}
    row["default"].update(runs)
    row["taken_candidates"] = int(fields["neighbours"].sum(dtype="int64"))
    # the yardstick: the same particles, no grid built ahead, one step
    st = sim.download_state()
    sim.upload_state(st["pos"], st["vel"])
    sim.kernel_times(reset=True)
    sim.simulate()
    kt = sim.kernel_times(reset=True)
    assert kt.steps == 1
    row["density_sweep_same_state"] = {"ms": 1e3 * kt.density}
    d, p, y = row["default"], row["plain"], 1e3 * kt.density
    row["default_over_plain"] = d["ms_per_derive_median"] / p["ms_per_derive_median"]
    row["default_over_density_sweep"] = d["ms_per_derive_median"] / y
    # the issue's condition: not slower than the check path by more than the spread (the wider of the two legs')
    spread = max(d["max"] - d["min"], p["max"] - p["min"])
    row["default_not_slower_than_plain_beyond_spread"] = bool(d["ms_per_derive_median"] <= p["ms_per_derive_median"] + spread)
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "init": args.init, "calls_per_round": args.calls, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    out["after_step_%d" % steps] = measure(sim)
    done += 1  # (the yardstick's step)
    print(json.dumps({("after_step_%d" % steps): out["after_step_%d" % steps]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
