#!/usr/bin/env python3
"""GPU time of the body labelling (sph_label_bodies) on one state: n particles after `early` and after `steps` steps,
at link = h and link = h / 2, on the default path (one link sweep over half of each neighbourhood into a concurrent
union-find, then flatten and the reductions) and on the check path (SPH_BODIES_PLAIN=1: min-label propagation, one
27-cell sweep per round).  Every leg is SphBodyStats.seconds (HIP events around the call's kernels; the check path's
span includes the host's wait between rounds) over `calls` labellings; the legs alternate over `rounds` rounds and the
median round is reported, with its minimum and maximum as the run-to-run spread.  Beside them the scale of one 27-cell
walk on the same state: the derived fields' sweep (SphDeriveStats.seconds).  The two paths' labels, tables and link
counts are compared word for word at the size that is timed.
  python scripts/studies/bodies.py [--n N] [--steps K] [--early K] [--out FILE.json]"""
import argparse
import ctypes
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
ap.add_argument("--calls", type=int, default=3, help="labellings per round on the default path")
ap.add_argument("--plain-calls", type=int, default=1, help="labellings per round on the check path")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--out", default=None)
args = ap.parse_args()


def leg(sim, link, plain):
    os.environ["SPH_BODIES_PLAIN"] = "1" if plain else "0"
    calls = args.plain_calls if plain else args.calls
    opt = _lib.SphBodyOptions(8, link)
    sim.sync()
    sim.body_stats(reset=True)
    for _ in range(calls):
        sim._check(sim._L.sph_label_bodies(sim._h, ctypes.byref(opt)), "sph_label_bodies")
    st = sim.body_stats(reset=True)
    assert st["calls"] == calls and st["gave_up"] == 0
    return 1e3 * st["seconds"] / calls, st["rounds"] // calls, st["links"] // calls, st["unions"] // calls


def measure(sim, link):
    per_leg = {False: [], True: []}
    seen = {}
    for rnd in range(args.rounds + 1):  # round 0 warms both legs up (and builds the grid ahead)
        for plain in (False, True):
            ms, rounds, links, unions = leg(sim, link, plain)
            if rnd:
                per_leg[plain].append(ms)
            seen[plain] = dict(rounds=rounds, links=links, unions=unions)
    row = {"link": link}
    for plain, v in per_leg.items():
        row["plain" if plain else "default"] = {"ms_per_call_median": statistics.median(v), "min": min(v), "max": max(v), **seen[plain]}
    # same words from both paths at this size
    results = {}
    for plain in (False, True):
        os.environ["SPH_BODIES_PLAIN"] = "1" if plain else "0"
        results[plain] = sim.label_bodies(link)
    os.environ["SPH_BODIES_PLAIN"] = "0"
    a, b = results[False], results[True]
    row["paths_agree"] = bool(np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["table"], b["table"])
                              and a["largest"] == b["largest"] and seen[False]["links"] == seen[True]["links"]
                              and seen[False]["unions"] == seen[True]["unions"])
    t = a["table"]
    row["num_bodies"] = a["num_bodies"]
    row["largest_count"] = int(t[:, 1].max())
    row["singletons"] = int((t[:, 1] == 1).sum())
    d, p = row["default"], row["plain"]
    row["default_over_plain"] = d["ms_per_call_median"] / p["ms_per_call_median"]
    row["default_below_plain_on_every_round"] = bool(d["max"] < p["min"])
    return row


def derive_sweep(sim):
    v = []
    for rnd in range(args.rounds + 1):
        sim.sync()
        sim.derive_stats(reset=True)
        for _ in range(args.calls):
            sim._check(sim._L.sph_derive(sim._h), "sph_derive")
        st = sim.derive_stats(reset=True)
        if rnd:
            v.append(1e3 * st["seconds"] / args.calls)
    return {"ms_per_derive_median": statistics.median(v), "min": min(v), "max": max(v)}


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
h = float(np.float32(sim.settings.h))
out = {"n": args.n, "init": args.init, "calls_per_round": args.calls, "plain_calls_per_round": args.plain_calls,
       "rounds": args.rounds, "library": os.path.basename(sph.library_path()), "candidates": "global memory (no LDS staging tried)"}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    row = {"derive_sweep_same_state": derive_sweep(sim), "link_h": measure(sim, h), "link_half_h": measure(sim, float(np.float32(0.5) * np.float32(h)))}
    for k in ("link_h", "link_half_h"):
        row[k]["default_over_derive_sweep"] = row[k]["default"]["ms_per_call_median"] / row["derive_sweep_same_state"]["ms_per_derive_median"]
    out["after_step_%d" % steps] = row
    print(json.dumps({("after_step_%d" % steps): row}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
