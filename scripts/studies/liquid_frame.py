#!/usr/bin/env python3
"""GPU time of the liquid frame (sph_render_liquid), tiled and plain, beside the tiled column frame
(sph_render_column) on one state: n particles after `steps` steps, 800 x 600, every option at its default.  Every
leg is the whole frame from sph_get_render_time (liquid: two clears + sphere splat + column splat + maximum + three
smoothing iterations + compose); the legs alternate over `rounds` rounds of `frames` renders and the median round is
reported with its spread.  Also measured: free fall (step 20).
  python scripts/studies/liquid_frame.py [--n N] [--steps K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/studies/liquid_frame.py --rounds 1 --early 0
--legs liquid_tiled,liquid_plain` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--legs", default="liquid_tiled,liquid_plain,column_tiled")
ap.add_argument("--out", default=None)
args = ap.parse_args()

LEGS = [  # name, plain splat, call
    ("liquid_tiled", False, lambda s: s.render_liquid()),
    ("liquid_plain", True, lambda s: s.render_liquid()),
    ("column_tiled", False, lambda s: s.render_column()),
]
LEGS = [leg for leg in LEGS if leg[0] in args.legs.split(",")]


def measure(sim):
    per_leg = {name: [] for name, _, _ in LEGS}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up
        for name, plain, call in LEGS:
            os.environ["SPH_RENDER_PLAIN"] = "1" if plain else "0"
            sim.sync()
            sim.render_time(reset=True)
            for _ in range(args.frames):
                call(sim)
            sec, frames = sim.render_time(reset=True)
            assert frames == args.frames
            if rnd:
                per_leg[name].append(1e3 * sec / frames)
    return {name: {"ms_per_frame_median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in per_leg.items()}


sim = sph.Simulator(sph.default_settings(args.n, True))
sim.setup()
out = {"n": args.n, "image": "800 x 600, defaults", "frames_per_round": args.frames, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    row = measure(sim)
    os.environ["SPH_RENDER_PLAIN"] = "0"
    sim.render_liquid()
    tiled = sim.liquid_buffers()
    row["pixels_with_a_surface"] = int((tiled["front"] != 0xFFFFFFFF).sum())
    row["pixels_with_a_column"] = int((tiled["column"] != 0).sum())
    os.environ["SPH_RENDER_PLAIN"] = "1"
    sim.render_liquid()
    plain = sim.liquid_buffers()
    row["plain_equals_tiled"] = bool(all(np.array_equal(tiled[k].view(np.uint8), plain[k].view(np.uint8)) for k in tiled))
    out["after_step_%d" % steps] = row
    print(json.dumps({("after_step_%d" % steps): row}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
