#!/usr/bin/env python3
"""GPU time of the pair statistics (sph_pair_statistics) on one run: n particles after `early` and after `steps` steps,
on the default path and on the check path (SPH_PAIRS_PLAIN=1), SphPairStats.seconds over `calls` calls.  In the same
rounds, on the same states:
  derive   the derived fields' sweep (SphDeriveStats.seconds, default path: k_derive_wave), which stages the same
           32-byte records over the same runs: pairs / derive is what the binning and the LDS scatter cost on top of
           the walk;
  route    what the pass replaces: sph_neighbour_lists in walk order with max_entries raised plus sph_neighbours_host,
           wall-clock from the call until the lists have landed in pinned memory (and its GPU seconds beside it); the
           pair statistics' own wall-clock, call until sph_pair_statistics_host returns, stands beside it.
The legs alternate over `rounds` rounds (round 0 warms every leg up) and the median round is reported with its minimum
and maximum as the run-to-run spread.
  python scripts/studies/pairs.py [--n N] [--steps K] [--early K] [--bins B] [--legs default,plain,derive,route] [--out FILE.json]
SPH_LIB_PATH selects another build of the library (-DPAIR_SLICE=..., -DPAIR_WGS_PER_CU=..., -DPAIR_DEFER=0,
-DPAIR_BIN_MAJOR=0); SPH_PAIRS_WORKGROUPS in the environment another number of workgroups."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--plain-rounds", type=int, default=2, help="rounds that also run the check path (it is slow)")
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--legs", default="default,plain,derive,route")
ap.add_argument("--bins", type=int, default=0)
ap.add_argument("--radius", type=float, default=0.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
legs = args.legs.split(",")


def pairs_call(sim):
    opt = _lib.SphPairOptions(C.sizeof(_lib.SphPairOptions), 0, args.radius, args.bins, 0)
    sim._check(sim._L.sph_pair_statistics(sim._h, C.byref(opt)), "sph_pair_statistics")


def pairs_leg(sim, plain, calls):
    """-> (GPU ms per call, wall ms of one call until its table is on the host, the stats)"""
    os.environ["SPH_PAIRS_PLAIN"] = "1" if plain else "0"
    sim.sync()
    sim.pair_stats(reset=True)
    for _ in range(calls):
        pairs_call(sim)
    sim.sync()
    st = sim.pair_stats(reset=True)
    assert st["calls"] == calls
    t0 = time.perf_counter()
    pairs_call(sim)
    sim._check(sim._L.sph_pair_statistics_host(sim._h, None, None, None), "sph_pair_statistics_host")
    wall = 1e3 * (time.perf_counter() - t0)
    os.environ["SPH_PAIRS_PLAIN"] = "0"
    return 1e3 * st["seconds"] / calls, wall, st


def route_leg(sim):
    """-> (wall ms until the lists are on the host, GPU ms of the four launches, entries)"""
    opt = _lib.SphNeighbourOptions(C.sizeof(_lib.SphNeighbourOptions), args.radius, _lib.SPH_NEIGHBOURS_WALK_ORDER, 0, 1 << 40)
    os.environ["SPH_NEIGHBOURS_PLAIN"] = "0"
    sim.sync()
    sim.neighbour_stats(reset=True)
    t0 = time.perf_counter()
    sim._check(sim._L.sph_neighbour_lists(sim._h, C.byref(opt)), "sph_neighbour_lists")
    entries = C.c_uint64(0)
    sim._check(sim._L.sph_neighbours_host(sim._h, None, None, None, C.byref(entries)), "sph_neighbours_host")
    wall = 1e3 * (time.perf_counter() - t0)
    return wall, 1e3 * sim.neighbour_stats(reset=True)["seconds"], entries.value


def summary(v):
    return {"ms_median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(sim):
    t = {k: [] for k in ("default", "default_wall", "plain", "plain_wall", "derive", "route_wall", "route_gpu")}
    row = {}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up (builds the grid ahead, sizes the buffers)
        if "default" in legs:
            ms, wall, st = pairs_leg(sim, False, args.calls)
            row.update(pairs=st["pairs"] // args.calls, runs_staged=st["runs_staged"] // args.calls, runs_direct=st["runs_direct"] // args.calls)
            if rnd:
                t["default"].append(ms), t["default_wall"].append(wall)
        if "plain" in legs and rnd <= args.plain_rounds:
            ms, wall, st = pairs_leg(sim, True, 1)
            row["pairs_plain"] = st["pairs"]
            if rnd:
                t["plain"].append(ms), t["plain_wall"].append(wall)
        if "derive" in legs:
            os.environ["SPH_DERIVE_PLAIN"] = "0"
            sim.sync()
            sim.derive_stats(reset=True)
            for _ in range(args.calls):
                sim._check(sim._L.sph_derive(sim._h), "sph_derive")
            d = sim.derive_stats(reset=True)
            if rnd:
                t["derive"].append(1e3 * d["seconds"] / args.calls)
        if "route" in legs:
            wall, gpu, entries = route_leg(sim)
            row["route_entries"] = entries
            if rnd:
                t["route_wall"].append(wall), t["route_gpu"].append(gpu)
        print(json.dumps({"round": rnd, **{k: v[-1] for k, v in t.items() if v}}), flush=True)
    row.update({k: summary(v) for k, v in t.items() if v})
    if t["default"]:
        # what the walk sends to the LDS table: a count and at most eight sum words per pair (zero words are skipped)
        row["lds_atomics_upper_bound"] = 9 * row["pairs"]
        if t["derive"]:
            row["default_over_derive_wave"] = row["default"]["ms_median"] / row["derive"]["ms_median"]
        if t["plain"]:
            row["plain_over_default"] = row["plain"]["ms_median"] / row["default"]["ms_median"]
        if t["route_wall"]:
            row["route_wall_over_default_wall"] = row["route_wall"]["ms_median"] / row["default_wall"]["ms_median"]
            row["route_gpu_over_default"] = row["route_gpu"]["ms_median"] / row["default"]["ms_median"]
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "init": args.init, "radius": args.radius, "bins": args.bins or 32, "calls_per_round": args.calls,
       "rounds": args.rounds, "legs": legs, "library": os.path.basename(sph.library_path())}
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
