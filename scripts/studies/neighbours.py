#!/usr/bin/env python3
"""GPU time of the neighbour lists (sph_neighbour_lists) on one run: n particles after `early` and after `steps` steps,
count, scan, emit and sort each on its own, on the default path and on the check path (SPH_NEIGHBOURS_PLAIN=1).
Every leg is SphNeighbourStats.seconds over `calls` calls with SPH_NEIGHBOURS_TIME_PHASE naming the one phase whose
HIP events are summed (the other phases run untimed); the legs alternate over `rounds` rounds and the median round is
reported, with its minimum and maximum as the run-to-run spread.  Beside them, in the same rounds, the yardstick: the
derived fields' sweep of the same state (SphDeriveStats.seconds, default path: k_derive_wave), which tests the same
candidates as the count.
  python scripts/studies/neighbours.py [--n N] [--steps K] [--early K] [--paths default,plain] [--out FILE.json]
SPH_LIB_PATH selects another build of the library (-DNBR_SLICE=..., -DNBR_SORT_SLICE=..., -DNBR_SORT_LISTS=...)."""
import argparse
import ctypes as C
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
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--paths", default="default,plain")
ap.add_argument("--radius", type=float, default=0.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
PHASES = ("count", "scan", "emit", "sort")
paths = [p == "plain" for p in args.paths.split(",")]


def lists(sim):
    opt = _lib.SphNeighbourOptions(C.sizeof(_lib.SphNeighbourOptions), args.radius, 0, 0, 1 << 40)
    sim._check(sim._L.sph_neighbour_lists(sim._h, C.byref(opt)), "sph_neighbour_lists")


def summary(v):
    return {"ms_median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(sim):
    legs = {(plain, k): [] for plain in paths for k in range(1, 5)}
    derive, runs, st = [], {}, {}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up (builds the grid ahead, sizes the buffers)
        for (plain, k), v in legs.items():
            os.environ["SPH_NEIGHBOURS_PLAIN"] = "1" if plain else "0"
            os.environ["SPH_NEIGHBOURS_TIME_PHASE"] = str(k)
            sim.sync()
            sim.neighbour_stats(reset=True)
            for _ in range(args.calls):
                lists(sim)
            sim.sync()
            st = sim.neighbour_stats(reset=True)
            assert st["calls"] == args.calls
            if rnd:
                v.append(1e3 * st["seconds"] / args.calls)
            if not plain:
                runs = {r: st[r] // args.calls for r in ("runs_staged", "runs_direct")}
        os.environ["SPH_DERIVE_PLAIN"] = "0"
        sim.sync()
        sim.derive_stats(reset=True)
        for _ in range(args.calls):
            sim._check(sim._L.sph_derive(sim._h), "sph_derive")
        d = sim.derive_stats(reset=True)
        if rnd:
            derive.append(1e3 * d["seconds"] / args.calls)
    os.environ["SPH_NEIGHBOURS_TIME_PHASE"] = "0"
    os.environ["SPH_NEIGHBOURS_PLAIN"] = "0"
    entries = st["entries"] // args.calls
    n = sim.settings.numParticles
    row = {"entries": entries, "longest": st["longest"], "mean_list": entries / n,
           "bytes_written": {"counts": 4 * n, "offsets": 8 * (n + 1), "neighbours_emit": 4 * entries, "neighbours_sort": 4 * entries},
           "derive_wave_same_state": summary(derive)}
    for plain in paths:
        name = "plain" if plain else "default"
        row[name] = {PHASES[k - 1]: summary(legs[plain, k]) for k in range(1, 5)}
        row[name]["total_ms"] = sum(row[name][p]["ms_median"] for p in PHASES)
    if False in paths:
        row["default"].update(runs)
        c, y = row["default"]["count"], row["derive_wave_same_state"]
        spread = max(c["max"] - c["min"], y["max"] - y["min"])
        row["count_over_derive_wave"] = c["ms_median"] / y["ms_median"]
        row["count_not_slower_than_derive_wave_beyond_spread"] = bool(c["ms_median"] <= y["ms_median"] + spread)
        if True in paths:
            row["default_sort_over_plain_sort"] = row["default"]["sort"]["ms_median"] / row["plain"]["sort"]["ms_median"]
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "init": args.init, "radius": args.radius, "calls_per_round": args.calls, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    out["after_step_%d" % steps] = measure(sim)
    print(json.dumps({"library": out["library"], ("after_step_%d" % steps): out["after_step_%d" % steps]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
