#!/usr/bin/env python3
"""GPU time of the field sample (sph_sample_field) on one state: n particles after `steps` steps, a 400 x 400
slice at z = 5 and a 128^3 volume over the box, tile path and plain path (SPH_SAMPLE_PLAIN=1).  Every leg is
the sampling kernel alone, from sph_get_sample_time; the legs alternate over `rounds` rounds of `calls` samples
and the median round is reported.  Beside it the yardstick: the density sweep two steps on (the first step after
the samples consumes the sampler's grid, and its event span holds the samples) -- SphKernelTimes.density over that
sweep's candidate tests.  Candidate tests are
counted on the host from the cell table: per lattice point (and per particle) the rows of the 27 cells around its
own; for the tile path also the candidates a wave READS, 64 lanes times the stretch it stages.
  python scripts/studies/field_sample.py [--n N] [--steps K] [--out FILE.json]
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
ap.add_argument("--early", type=int, default=20, help="also measure after this many steps (0: skip)")
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--field", default="density")
ap.add_argument("--out", default=None)
args = ap.parse_args()

F = np.float32
D = 100
WORKLOADS = {  # origin, spacing, (nz, ny, nx)
    "slice_400x400_z5": ((0.0, 0.0, 5.0), (float(F(10) / F(400)),) * 2 + (1.0,), (1, 400, 400)),
    "volume_128^3": ((0.0, 0.0, 0.0), (float(F(10) / F(128)),) * 3, (128, 128, 128)),
}
LEGS = [(w, plain) for w in WORKLOADS for plain in (False, True)]


def axis_cells(origin, spacing, count, h):
    p = F(origin) + np.arange(count).astype(F) * F(spacing)
    q = p / F(h)
    inside = (p >= 0) & (q < F(D))
    return np.where(inside, q, 0).astype(np.int64), inside


def box3(a, axis):
    """a[i - 1] + a[i] + a[i + 1] along `axis`, zero beyond the ends"""
    pad = [(1, 1) if k == axis else (0, 0) for k in range(a.ndim)]
    b = np.pad(a, pad)
    sl = lambda lo, hi: tuple(slice(lo, hi) if k == axis else slice(None) for k in range(a.ndim))
    n = a.shape[axis]
    return b[sl(0, n)] + b[sl(1, n + 1)] + b[sl(2, n + 2)]


def candidate_counts(count, h, origin, spacing, shape):
    """count[z, y, x]: rows per cell.  Returns (tests of the plain walk, candidates read by the tile path's waves)."""
    nz, ny, nx = shape
    cx, okx = axis_cells(origin[0], spacing[0], nx, h)
    cy, oky = axis_cells(origin[1], spacing[1], ny, h)
    cz, okz = axis_cells(origin[2], spacing[2], nz, h)
    yz = box3(box3(count, 0), 1)                       # the nine (y, z) rows of cells folded, per x
    rows = yz[cz[:, None], cy[None, :], :] * (okz[:, None] & oky[None, :])[:, :, None]   # (nz, ny, D)
    plain = int((box3(rows, 2)[:, :, cx] * okx[None, None, :]).sum())
    csum = np.concatenate([np.zeros(rows.shape[:2] + (1,), np.int64), np.cumsum(rows, axis=2)], axis=2)
    tile = 0
    for b in range(0, nx, 64):
        lanes = np.flatnonzero(okx[b:b + 64]) + b
        if len(lanes) == 0:
            continue
        lo, hi = max(int(cx[lanes].min()) - 1, 0), min(int(cx[lanes].max()) + 1, D - 1)
        # (an upper bound by the empty cells at the ends of the stretch, which hold no rows anyway)
        tile += 64 * int((csum[:, :, hi + 1] - csum[:, :, lo]).sum())
    return plain, tile


def measure(sim):
    per_leg = {leg: [] for leg in LEGS}
    for rnd in range(args.rounds + 1):  # round 0 warms every leg up
        for leg in LEGS:
            w, plain = leg
            os.environ["SPH_SAMPLE_PLAIN"] = "1" if plain else "0"
            sim.sync()
            sim.sample_time(reset=True)
            for _ in range(args.calls):
                sim.sample_field(args.field, *WORKLOADS[w])
            sec, calls = sim.sample_time(reset=True)
            assert calls == args.calls
            if rnd:
                per_leg[leg].append(1e3 * sec / calls)
    cells = sim.download_grid()["cells"].astype(np.int64)
    count = (cells[:, 1] - cells[:, 0]).reshape(D, D, D)
    row = {}
    for (w, plain), v in per_leg.items():
        tests, read = candidate_counts(count, sim.settings.h, *WORKLOADS[w])
        ms = statistics.median(v)
        r = {"ms_per_sample_median": ms, "min": min(v), "max": max(v), "candidate_tests": tests,
             "ns_per_candidate_test": 1e6 * ms / tests if tests else None}
        if not plain:
            r["candidates_read_by_all_lanes"] = read
            r["ns_per_candidate_read"] = 1e6 * ms / read if read else None
        row[w + ("_plain" if plain else "_tile")] = r
    # The yardstick: the density sweep of a step of its own.  The step right after the samples consumes the grid the
    # sampler built, whose events were recorded before the samples ran: its "density" span holds them.  The step
    # after that builds its own grid; its table (still valid after the step) gives that sweep's candidate tests.
    sim.simulate()
    sim.kernel_times(reset=True)
    sim.simulate()
    kt = sim.kernel_times(reset=True)
    assert kt.steps == 1
    cells = sim.download_grid()["cells"].astype(np.int64)
    count = (cells[:, 1] - cells[:, 0]).reshape(D, D, D)
    sweep_tests = int((count * box3(box3(box3(count, 0), 1), 2)).sum())
    row["density_sweep_two_steps_on"] = {"ms": 1e3 * kt.density, "candidate_tests": sweep_tests,
                                         "ns_per_candidate_test": 1e9 * kt.density / sweep_tests}
    return row


sim = sph.Simulator(sph.default_settings(args.n, True), flags=_lib.SPH_FLAG_NO_READBACK)
sim.setup()
out = {"n": args.n, "field": args.field, "calls_per_round": args.calls, "rounds": args.rounds,
       "library": os.path.basename(sph.library_path())}
done = 0
for steps in sorted({args.early, args.steps} - {0}):
    while done < steps:
        sim.simulate()
        done += 1
    out["after_step_%d" % steps] = measure(sim)
    done += 2  # (the yardstick's steps)
    print(json.dumps({("after_step_%d" % steps): out["after_step_%d" % steps]}), flush=True)
sim.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
