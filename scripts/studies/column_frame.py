#!/usr/bin/env python3
"""GPU time of the column frame (sph_render_column), tiled and plain, beside the tiled field frame
(sph_render_field, speed) on one state: n particles after `steps` steps, 800 x 600, automatic range.  Every leg
is clear + splat + [range] + compose from sph_get_render_time; the legs alternate over `rounds` rounds of
`frames` renders and the median round is reported.  Also measured: free fall (step 20).
Beside the times: the share of the tiled splat's 1024-row workgroups whose hull of footprints does not fit
the 8192-pixel tile, worked out on the host from the sorted order of the last grid build (sph_download_grid)
with the footprint bound of DESIGN.md section 10h in float64, and the pixel tests per particle.
  python scripts/studies/column_frame.py [--n N] [--steps K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/studies/column_frame.py --rounds 1 --early 0`
(a run of its own)."""
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
ap.add_argument("--out", default=None)
args = ap.parse_args()
W, H, TILE, BLOCK = 800, 600, 8192, 1024

LEGS = [  # name, plain splat, call
    ("column_tiled", False, lambda s: s.render_column()),
    ("column_plain", True, lambda s: s.render_column()),
    ("field_speed_tiled", False, lambda s: s.render_field("speed")),
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
    return {name: {"ms_per_frame_median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in per_leg.items()}


def footprints(sim):
    """the footprint boxes of the rows in the order the splat reads them, and what follows from them"""
    st, ids = sim.download_state(), sim.download_grid()["ids"]
    p = st["pos"][ids].astype(np.float64)
    h = float(np.float32(sim.settings.h))
    X, Y, w = p[:, 0] - 5.0, p[:, 1] - 5.0, 15.0 - p[:, 2]
    k = h * np.sqrt(1.0 + (X / w) ** 2 + (Y / w) ** 2) / (w - h)
    px = np.floor((0.5 * X / w + 1.0) * 0.5 * W)
    py = (H - 1) - np.floor((0.5 * Y / w + 1.0) * 0.5 * H)
    hx, hy = np.ceil(0.25 * W * k) + 1, np.ceil(0.25 * H * k) + 1
    c0, c1 = np.maximum(px - hx, 0), np.minimum(px + hx, W - 1)
    r0, r1 = np.maximum(py - hy, 0), np.minimum(py + hy, H - 1)
    tests = np.maximum(c1 - c0 + 1, 0) * np.maximum(r1 - r0 + 1, 0)
    pad = (-len(p)) % BLOCK
    lo = lambda a: np.pad(a, (0, pad), constant_values=np.inf).reshape(-1, BLOCK).min(1)
    hi = lambda a: np.pad(a, (0, pad), constant_values=-np.inf).reshape(-1, BLOCK).max(1)
    area = (hi(c1) - lo(c0) + 1) * (hi(r1) - lo(r0) + 1)
    return {"workgroups": int(len(area)), "workgroups_fell_back": int((area > TILE).sum()),
            "share_fell_back": float((area > TILE).mean()), "median_hull_pixels": float(np.median(area)),
            "pixel_tests_per_particle_mean": float(tests.mean()), "pixel_tests_per_particle_min": float(tests.min()),
            "pixel_tests_per_particle_max": float(tests.max())}


sim = sph.Simulator(sph.default_settings(args.n, True))
sim.setup()
out = {"n": args.n, "image": "800 x 600, automatic range", "frames_per_round": args.frames, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    row = measure(sim)
    row["footprints"] = footprints(sim)
    os.environ["SPH_RENDER_PLAIN"] = "0"
    sim.render_column()
    tiled = sim.column_buffer()
    row["column_range"] = [float(x) for x in sim.column_range()]
    row["pixels_with_fluid"] = int((tiled != 0).sum())
    os.environ["SPH_RENDER_PLAIN"] = "1"
    sim.render_column()
    row["plain_equals_tiled"] = bool(np.array_equal(tiled, sim.column_buffer()))
    out["after_step_%d" % steps] = row
    print(json.dumps({("after_step_%d" % steps): row}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
