#!/usr/bin/env python3
"""The display loop with the frame rendered on the GPU: `simulate(); render(); frame_host()` against the
loop that fetches positions, `simulate(); getPosition()` (what display.cpp does, bench.py --mode display).
Per-frame wall time and the renderer's GPU time (sph_get_render_time) for frames 1-20 (free fall) and
81-100 (floor pile), plain and aggregated splat, with and without the position read-back.
usage: python scripts/studies/render_loop.py [--n N] [--frames K] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4194304)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()
s = sph.default_settings(args.n, True)
WINDOWS = {"frames_1_20": (0, 20), "frames_81_100": (80, 100)}


def loop(label, render, readback, plain=False):
    os.environ["SPH_RENDER_PLAIN"] = "1" if plain else "0"
    sim = sph.Simulator(s, flags=0 if readback else _lib.SPH_FLAG_NO_READBACK)
    sim.setup()
    for _ in range(5):  # warm-up, as bench.py does, then back to the initial condition
        sim.simulate()
        if render:
            sim.render_frame()
            sim.frame_host()
        elif readback:
            sim.getPosition()
    sim.sync()
    sim.setup()
    wall, gpu = [], []
    if render:
        sim.render_time(reset=True)
    t_all = time.perf_counter()
    for _ in range(args.frames):
        t0 = time.perf_counter()
        sim.simulate()
        if render:
            sim.render_frame()
            sim.frame_host()
        elif readback:
            sim.getPosition()
        else:
            sim.sync()
        wall.append(time.perf_counter() - t0)
        if render:
            gpu.append(sim.render_time(reset=True)[0])
    total = time.perf_counter() - t_all
    sim.close()
    row = {"loop": label, "render": render, "readback": readback, "splat": ("plain" if plain else "aggregated") if render else None,
           "ms_per_frame": 1e3 * total / args.frames}
    for name, (a, b) in WINDOWS.items():
        if b <= args.frames:
            row[name] = {"wall_ms": 1e3 * sum(wall[a:b]) / (b - a)}
            if render:
                row[name]["render_gpu_ms"] = 1e3 * sum(gpu[a:b]) / (b - a)
    print(json.dumps(row), flush=True)
    return row


rows = [loop("simulate(); getPosition()", False, True),
        loop("simulate(); sync()  [no read-back, nothing drawn]", False, False)]
for readback in (False, True):
    for plain in (True, False):
        rows.append(loop("simulate(); render(); frame_host()", True, readback, plain))
out = {"n": args.n, "frames": args.frames, "image": "800 x 600, point size 3, flat", "rows": rows}
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
