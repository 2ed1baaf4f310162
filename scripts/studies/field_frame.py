#!/usr/bin/env python3
"""GPU time of the field frame (sph_render_field) beside the flat frame (sph_render_frame) on one state:
n particles after `steps` steps, 800 x 600, point size 3, speed.  Every leg is clear + splat + compose from
sph_get_render_time; the legs alternate over `rounds` rounds of `frames` renders and the median round is
reported.  Also measured: free fall (step 20), where the rectangles of the workgroups are widest.
The time of ONE kernel (the range kernel, the splat) comes from a kernel trace, not from here: the
automatic-range leg minus the fixed-range leg is printed as a cross-check only, it is a difference of two
medians that lies within their spread.
  python scripts/studies/field_frame.py [--n N] [--steps K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/studies/field_frame.py --rounds 1 --early 0`
(a run of its own; profiles/field_frame_kernel_stats.csv)."""
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
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

LEGS = [  # name, plain splat, call
    ("flat_tiled", False, lambda s: s.render_frame()),
    ("field_speed_tiled_auto_range", False, lambda s: s.render_field("speed")),
    ("field_speed_tiled_fixed_range", False, lambda s: s.render_field("speed", 0.0, 5.0)),
    ("flat_plain", True, lambda s: s.render_frame()),
    ("field_speed_plain_auto_range", True, lambda s: s.render_field("speed")),
]


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
    row = {name: {"ms_per_frame_median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in per_leg.items()}
    row["auto_minus_fixed_range_ms (difference of medians: cross-check, not the kernel time)"] = (row["field_speed_tiled_auto_range"]["ms_per_frame_median"]
                                             - row["field_speed_tiled_fixed_range"]["ms_per_frame_median"])
    return row


sim = sph.Simulator(sph.default_settings(args.n, True), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "image": "800 x 600, point size 3", "frames_per_round": args.frames, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    out["after_step_%d" % steps] = measure(sim)
    sim.render_field("speed")
    out["after_step_%d" % steps]["speed_range"] = [float(x) for x in sim.field_range()]
    print(json.dumps({("after_step_%d" % steps): out["after_step_%d" % steps]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
