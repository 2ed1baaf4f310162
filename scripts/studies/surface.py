#!/usr/bin/env python3
"""GPU time of the surface mesh (sph_extract_surface) on one state: n particles after `steps` steps, the lattices
101^3 and 201^3 over the box, iso = half the rest density, production path and plain path (SPH_SURFACE_PLAIN=1).  Every leg
reports the two figures of sph_get_surface_time -- the sampling kernel, and count + scan + emit -- and the mesh's
size; the legs alternate over `rounds` rounds of `calls` extractions and the median round is reported.  The
yardstick for the extraction is the sampling kernel over the same lattice.
  python scripts/studies/surface.py [--n N] [--steps K] [--out FILE.json]
SPH_LIB_PATH selects another build of the library."""
import argparse
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
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iso", type=float, default=500.0, help="half of SPH_REST_DENSITY")
ap.add_argument("--out", default=None)
args = ap.parse_args()

F = np.float32
LATTICES = {"101^3": 101, "201^3": 201}
LEGS = [(w, plain) for w in LATTICES for plain in (False, True)]

sim = sph.Simulator(sph.default_settings(args.n, True), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
for _ in range(args.steps):
    sim.simulate()
box = float(sim.settings.boxDim)
per_leg = {leg: [] for leg in LEGS}
size = {}
for rnd in range(args.rounds + 1):  # round 0 warms every leg up
    for leg in LEGS:
        w, plain = leg
        N = LATTICES[w]
        os.environ["SPH_SURFACE_PLAIN"] = "1" if plain else "0"
        sim.sync()
        sim.surface_time(reset=True)
        for _ in range(args.calls):
            mesh = sim.extract_surface(args.iso, (0.0, 0.0, 0.0), float(F(box) / F(N - 1)), (N, N, N))
        sample, extract, calls = sim.surface_time(reset=True)
        assert calls == args.calls
        size[leg] = (len(mesh["vertices"]), len(mesh["triangles"]))
        if rnd:
            per_leg[leg].append((1e3 * sample / calls, 1e3 * extract / calls))
out = {"n": args.n, "steps": args.steps, "iso": args.iso, "calls_per_round": args.calls, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
for (w, plain), v in per_leg.items():
    s, e = [a for a, _ in v], [b for _, b in v]
    out[w + ("_plain" if plain else "_production")] = {
        "vertices": size[(w, plain)][0], "triangles": size[(w, plain)][1],
        "sample_ms_median": statistics.median(s), "sample_ms_min": min(s), "sample_ms_max": max(s),
        "extract_ms_median": statistics.median(e), "extract_ms_min": min(e), "extract_ms_max": max(e)}
sim.close()
print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
