#!/usr/bin/env python3
"""GPU time of the per-body moments (sph_measure_bodies) on one state: n particles after `early`
and after `steps` steps, at link = h and link = h / 2, on the default path (wave groups, the LDS fold of a block's
first body, one set of global atomics per 2,048 rows) and on the check path (SPH_BODIES_PLAIN=1: every word of every
row a global atomic).  Every leg is SphBodyMeasureStats.seconds -- the moment launches alone, HIP events around them --
over `calls` calls; the legs alternate over `rounds` rounds and the median round is reported, with its minimum and
maximum as the run-to-run spread.  Beside them, from the same calls, the labelling's time (SphBodyStats.seconds) and
the yardstick of one pass over the sorted stream (40 B x n over the HBM peak).  The two paths' raw rows and size
histograms are compared byte for byte at the size that is timed.
  python scripts/studies/body_moments.py [--n N] [--steps K] [--early K] [--out FILE.json]"""
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

HBM_PEAK = 8.0e12  # bytes / s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--calls", type=int, default=3, help="calls per round on the default path")
ap.add_argument("--plain-calls", type=int, default=1, help="calls per round on the check path")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--out", default=None)
args = ap.parse_args()


def leg(sim, link, plain):
    """-> (ms of the moment launches per call, ms of the labelling per call)"""
    os.environ["SPH_BODIES_PLAIN"] = "1" if plain else "0"
    calls = args.plain_calls if plain else args.calls
    opt = _lib.SphBodyMeasureOptions(ctypes.sizeof(_lib.SphBodyMeasureOptions), link, 0, 0)
    sim.sync()
    sim.body_stats(reset=True)
    sim.body_measure_stats(reset=True)
    for _ in range(calls):
        sim._check(sim._L.sph_measure_bodies(sim._h, ctypes.byref(opt)), "sph_measure_bodies")
    ms, ls = sim.body_measure_stats(reset=True), sim.body_stats(reset=True)
    assert ms["calls"] == ls["calls"] == calls and ls["gave_up"] == 0
    return 1e3 * ms["seconds"] / calls, 1e3 * ls["seconds"] / calls


def measure(sim, link):
    per_leg = {False: [], True: []}
    labelling = {False: [], True: []}
    for rnd in range(args.rounds + 1):  # round 0 warms both legs up (and builds the grid ahead)
        for plain in (False, True):
            ms, label_ms = leg(sim, link, plain)
            if rnd:
                per_leg[plain].append(ms)
                labelling[plain].append(label_ms)
    row = {"link": link}
    for plain, v in per_leg.items():
        row["plain" if plain else "default"] = {"ms_per_call_median": statistics.median(v), "min": min(v), "max": max(v),
                                                "labelling_ms_per_call_median": statistics.median(labelling[plain])}
    # same bytes from both paths at this size
    results = {}
    for plain in (False, True):
        os.environ["SPH_BODIES_PLAIN"] = "1" if plain else "0"
        results[plain] = sim.measure_bodies(link)
    os.environ["SPH_BODIES_PLAIN"] = "0"
    a, b = results[False], results[True]
    row["paths_agree"] = bool(a["moments"].tobytes() == b["moments"].tobytes() and np.array_equal(a["size_hist"], b["size_hist"])
                              and np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["table"], b["table"]))
    counts = a["moments"]["count"]
    row["num_bodies"] = a["num_bodies"]
    row["largest_count"] = int(counts.max())
    row["singletons"] = int((counts == 1).sum())
    row["saturated"] = int(a["moments"]["saturated"].sum())
    row["size_hist"] = a["size_hist"].tolist()
    d, p = row["default"], row["plain"]
    row["default_over_plain"] = d["ms_per_call_median"] / p["ms_per_call_median"]
    row["default_below_plain_on_every_round"] = bool(d["max"] < p["min"])
    row["moments_over_labelling"] = d["ms_per_call_median"] / d["labelling_ms_per_call_median"]
    row["yardstick_ms_40B_per_row"] = 1e3 * 40.0 * args.n / HBM_PEAK
    row["default_over_yardstick"] = d["ms_per_call_median"] / row["yardstick_ms_40B_per_row"]
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
h = float(np.float32(sim.settings.h))
out = {"n": args.n, "init": args.init, "calls_per_round": args.calls, "plain_calls_per_round": args.plain_calls,
       "rounds": args.rounds, "library": os.path.basename(sph.library_path()), "hbm_peak_bytes_per_s": HBM_PEAK}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    row = {"link_h": measure(sim, h), "link_half_h": measure(sim, float(np.float32(0.5) * np.float32(h)))}
    out["after_step_%d" % steps] = row
    print(json.dumps({("after_step_%d" % steps): row}), flush=True)
    if args.out:  # (what is measured so far survives a run that is cut short)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
sim.close()
out["condition_met"] = all(out[k][l]["default_below_plain_on_every_round"] and out[k][l]["paths_agree"]
                           for k in out if k.startswith("after_step_") for l in ("link_h", "link_half_h"))
print(json.dumps({"condition_met": out["condition_met"]}), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
