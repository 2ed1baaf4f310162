#!/usr/bin/env python3
"""GPU time of the view frame (sph_render_view) on one run: n particles after `early` and after `steps` steps, radius
0.5 h, 800 x 600, from the reference camera (the eye of the other four frames) and from an oblique one; with it the
grid layers and candidate tests per ray (SphCastStats).  In the same rounds, on the same states:
  liquid   sph_render_liquid at the same size, for scale (sph_get_render_time);
  check    the check path (SPH_CAST_PLAIN=1) against the default path on the largest square view the check path admits
           (rays x particles <= 2^32), from the oblique camera.
The legs alternate over `rounds` rounds (round 0 warms every leg up) and the median round is reported with its minimum
and maximum as the run-to-run spread.
  python scripts/studies/ray_cast.py [--n N] [--steps K] [--early K] [--legs view,liquid,check] [--out FILE.json]
SPH_LIB_PATH selects another build of the library."""
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
ap.add_argument("--legs", default="view,liquid,check")
ap.add_argument("--width", type=int, default=800)
ap.add_argument("--height", type=int, default=600)
ap.add_argument("--out", default=None)
args = ap.parse_args()
legs = args.legs.split(",")
CAMERAS = {"reference": dict(eye=(5, 5, 15), target=(5, 5, 0), tan_half=(2.0, 2.0)),
           "oblique": dict(eye=(-4, 13, 9), target=(5, 5, 5), tan_half=(0.0, 0.0))}


def view_leg(sim, cam, width, height, plain, calls):
    """-> (GPU ms per frame, layers per ray, tests per ray, pixels with a hit)"""
    os.environ["SPH_CAST_PLAIN"] = "1" if plain else "0"
    sim.sync()
    sim.render_time(reset=True)
    sim.cast_stats(reset=True)
    for _ in range(calls):
        sim.render_view(cam["eye"], cam["target"], width=width, height=height, tan_half=cam["tan_half"], radius=0.5 * sim.settings.h)
    sec, frames = sim.render_time(reset=True)
    st = sim.cast_stats(reset=True)
    assert frames == calls == st["calls"]
    hits = int((sim.view_buffer() != _lib.CAST_MISS).sum())
    os.environ["SPH_CAST_PLAIN"] = "0"
    return 1e3 * sec / calls, st["layers"] / st["rays"], st["tests"] / st["rays"], hits


def liquid_leg(sim, calls):
    sim.sync()
    sim.render_time(reset=True)
    for _ in range(calls):
        sim.render_liquid(radius=0.5 * sim.settings.h, width=args.width, height=args.height)
    sec, frames = sim.render_time(reset=True)
    assert frames == calls
    return 1e3 * sec / calls


def summary(v):
    return {"ms_median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(sim):
    side = 1
    while (side + 1) ** 2 * sim.n <= 1 << 32:
        side += 1
    t = {}
    row = {"check_view": [side, side]}
    for rnd in range(args.rounds + 1):   # round 0 warms every leg up (builds the grid ahead, sizes the buffers)
        for name, cam in CAMERAS.items():
            if "view" in legs:
                ms, layers, tests, hits = view_leg(sim, cam, args.width, args.height, False, args.calls)
                row[name] = dict(layers_per_ray=layers, tests_per_ray=tests, pixels_hit=hits)
                if rnd:
                    t.setdefault(name, []).append(ms)
        if "liquid" in legs:
            ms = liquid_leg(sim, args.calls)
            if rnd:
                t.setdefault("liquid", []).append(ms)
        if "check" in legs:
            for plain in (False, True):
                ms, layers, tests, hits = view_leg(sim, CAMERAS["oblique"], side, side, plain, 1)
                row["check_plain" if plain else "check_default"] = dict(tests_per_ray=tests, pixels_hit=hits)
                if rnd:
                    t.setdefault("check_plain" if plain else "check_default", []).append(ms)
        print(json.dumps({"round": rnd, **{k: v[-1] for k, v in t.items() if v}}), flush=True)
    for k, v in t.items():
        row.setdefault(k, {}).update(summary(v))
    if "check_plain" in t:
        row["plain_over_default"] = row["check_plain"]["ms_median"] / row["check_default"]["ms_median"]
    return row


sim = sph.Simulator(sph.default_settings(args.n, args.init == "random"), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "init": args.init, "size": [args.width, args.height], "calls_per_round": args.calls, "rounds": args.rounds,
       "legs": legs, "library": os.path.basename(sph.library_path())}
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
