#!/usr/bin/env python3
"""GPU time of the body tracks (sph_track_bodies): n particles, the labelling of step `a` as the
reference and the state of step `a + 1` tracked against it, for a + 1 = `early` and a + 1 = `steps`, at link = h and
link = h / 2, on the default path (the fold, the sort of the partial edges, integer atomics) and on the check path
(SPH_BODIES_PLAIN=1: every particle id a partial, the sorts over all n).  The two states of a pair are downloaded once
and uploaded again for every call, the reference always made on the default path (its words are the same); every leg
is SphBodyTrackStats.seconds of the one tracked call -- the track launches alone, HIP events around them; the legs
alternate over `rounds` rounds and the median round is reported, with its minimum and maximum as the run-to-run spread;
the condition is the default path below the check path in every round.
Beside them, from the same calls: the partial edges M, the edges, the labelling's time (SphBodyStats.seconds) and the
yardstick of one pass over what the fold reads (28 B x n -- position and id 16, the row's label 4, its rank 4, prow 4
-- over the HBM peak).  The two paths' results are compared byte for byte at the size that is timed.
  python scripts/studies/body_tracks.py [--n N] [--steps K] [--early K] [--out FILE.json]"""
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
ap.add_argument("--early", type=int, default=20, help="also measure the pair that ends after this many steps (0: skip)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--init", default="random", choices=("random", "grid"))
ap.add_argument("--out", default=None)
args = ap.parse_args()


def snapshot(sim):
    st = sim.download_state()
    return np.array(st["pos"], copy=True), np.array(st["vel"], copy=True)


def tracked(sim, before, after, link, plain, results=False):
    """the reference from `before` (default path), then `after` tracked on the path asked for
    -> (ms of the track launches, ms of the labelling, partials, edges), or the call's results"""
    os.environ["SPH_BODIES_PLAIN"] = "0"
    opt = _lib.SphBodyTrackOptions(ctypes.sizeof(_lib.SphBodyTrackOptions), link, 0, 0)
    sim.track_reset()
    sim.upload_state(*before)
    sim._check(sim._L.sph_track_bodies(sim._h, ctypes.byref(opt)), "sph_track_bodies")
    sim.upload_state(*after)
    sim.sync()
    sim.body_stats(reset=True)
    sim.body_track_stats(reset=True)
    os.environ["SPH_BODIES_PLAIN"] = "1" if plain else "0"
    try:
        if results:
            return sim.track_bodies(link)
        sim._check(sim._L.sph_track_bodies(sim._h, ctypes.byref(opt)), "sph_track_bodies")
    finally:
        os.environ["SPH_BODIES_PLAIN"] = "0"
    ts, ls = sim.body_track_stats(reset=True), sim.body_stats(reset=True)
    assert ts["calls"] == ls["calls"] == 1 and ls["gave_up"] == 0
    return 1e3 * ts["seconds"], 1e3 * ls["seconds"], ts["partials"], ts["edges"]


def measure(sim, before, after, link):
    legs = {False: [], True: []}
    for rnd in range(args.rounds + 1):  # round 0 warms both legs up
        for plain in (False, True):
            got = tracked(sim, before, after, link, plain)
            if rnd:
                legs[plain].append(got)
    row = {"link": link}
    for plain, v in legs.items():
        ms = [g[0] for g in v]
        row["plain" if plain else "default"] = {"ms_per_call_median": statistics.median(ms), "min": min(ms), "max": max(ms), "rounds_ms": ms,
                                                "labelling_ms_per_call_median": statistics.median(g[1] for g in v),
                                                "partials": v[0][2], "edges": v[0][3]}
    a, b = (tracked(sim, before, after, link, plain, results=True) for plain in (False, True))
    row["paths_agree"] = bool(all(a[k].tobytes() == b[k].tobytes() for k in ("labels", "table", "tracks", "previous", "edges"))
                              and a["summary"] == b["summary"])
    row["summary"] = a["summary"]
    row["most_parents"] = int(a["tracks"]["parents"].max())
    row["most_children"] = int(a["previous"]["children"].max())
    d, p = row["default"], row["plain"]
    row["partials_over_n"] = d["partials"] / args.n
    row["default_over_plain"] = d["ms_per_call_median"] / p["ms_per_call_median"]
    row["default_below_plain_on_every_round"] = bool(all(a < b for a, b in zip(d["rounds_ms"], p["rounds_ms"])))
    row["default_max_below_plain_min"] = bool(d["max"] < p["min"])
    row["tracks_over_labelling"] = d["ms_per_call_median"] / d["labelling_ms_per_call_median"]
    row["yardstick_ms_28B_per_row"] = 1e3 * 28.0 * args.n / HBM_PEAK
    row["default_over_yardstick"] = d["ms_per_call_median"] / row["yardstick_ms_28B_per_row"]
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
h = float(np.float32(sim.settings.h))
out = {"n": args.n, "init": args.init, "rounds": args.rounds, "library": os.path.basename(sph.library_path()), "hbm_peak_bytes_per_s": HBM_PEAK}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps - 1:
        sim.simulate()
        done += 1
    before = snapshot(sim)
    sim.simulate()
    done += 1
    after = snapshot(sim)
    row = {"link_h": measure(sim, before, after, h), "link_half_h": measure(sim, before, after, float(np.float32(0.5) * np.float32(h)))}
    key = "step_%d_to_%d" % (steps - 1, steps)
    out[key] = row
    print(json.dumps({key: row}), flush=True)
    if args.out:  # (what is measured so far survives a run that is cut short)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    sim.upload_state(*after)  # (the run goes on from the state it had reached)
sim.close()
out["condition_met"] = all(out[k][l]["default_below_plain_on_every_round"] and out[k][l]["paths_agree"]
                           for k in out if k.startswith("step_") for l in ("link_h", "link_half_h"))
print(json.dumps({"condition_met": out["condition_met"]}), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
