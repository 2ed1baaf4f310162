"""What the three frames share on the device ("The tile scheme"): one tile kernel whose
workgroups decide, each for itself, between the LDS tile and the per-hit global atomics, one check-path kernel and
one clear.  The frames' own tests make every workgroup of a launch take the same branch; here a launch mixes them.
The state is uploaded and not stepped, so the splat reads it in particle-id order and the test lays out each
1024-row workgroup: rows 0-1023 a tight cluster (fits the tile), rows 1024-2047 spread over the box (falls back
at 800 x 600), rows 2048-2099 the cluster again, a partly filled last workgroup (fits).  Every comparison is exact:
buffer words, RGB bytes and the bits of the range against the three numpy restatements, and the check path
against the tiled one."""
import functools

import numpy as np
import pytest

import cudafluidsimulator_amd as sph

import column_frame_restatement as CF
import field_frame_restatement as FF
import render_restatement as R

pytestmark = pytest.mark.gpu

F = np.float32
N, BLOCK, TILE = 2100, 1024, 8192      # rows, rows per workgroup and pixels per tile of the splat
W, H = 800, 600
EXPECTED_FIT = [True, False, True]


@functools.lru_cache(maxsize=None)
def settings():
    """(not at import: the library is loaded by the first test, after every test module has been imported)"""
    return sph.default_settings(N, True)


@functools.lru_cache(maxsize=None)
def state():
    """(pos, vel) in id order: the clusters inside [4.9, 5.1]^3, a few pixels in the middle of the image"""
    rng = np.random.default_rng(20)
    pos = np.empty((N, 3), F)
    cluster = np.r_[0:BLOCK, 2 * BLOCK:N]
    pos[cluster] = rng.uniform(4.9, 5.1, (len(cluster), 3))
    pos[BLOCK:2 * BLOCK] = rng.uniform(1.0, 9.0, (BLOCK, 3))
    vel = rng.normal(0.0, 1.0, (N, 3)).astype(F)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def hull_fits(c0, r0, c1, r1):
    """per workgroup: does the hull of its rows' pixel boxes (inclusive, clipped; empty: c1 < c0) fit the tile"""
    fits = []
    for b in range(0, N, BLOCK):
        on = c1[b:b + BLOCK] >= c0[b:b + BLOCK]
        assert on.any()
        x0, x1 = c0[b:b + BLOCK][on].min(), c1[b:b + BLOCK][on].max()
        y0, y1 = r0[b:b + BLOCK][on].min(), r1[b:b + BLOCK][on].max()
        fits.append(bool((x1 - x0 + 1) * (y1 - y0 + 1) <= TILE))
    return fits


def splat_fits(pos, point_size):
    """flat and field frames: the box of the visible centres, widened by the radius and clipped"""
    px, py, _ = R.project(pos, W, H)
    r = (point_size - 1) // 2
    seen = (px + r >= 0) & (px - r < W) & (py + r >= 0) & (py - r < H)
    c0, c1 = np.maximum(px - r, 0), np.where(seen, np.minimum(px + r, W - 1), -1)
    return hull_fits(c0, np.maximum(py - r, 0), c1, np.minimum(py + r, H - 1))


def column_fits(pos):
    """column frame: the hull of the footprint bounds of section 10h (in float64, as scripts/studies/column_frame.py)"""
    p = pos.astype(np.float64)
    h = float(F(settings().h))
    X, Y, w = p[:, 0] - 5.0, p[:, 1] - 5.0, 15.0 - p[:, 2]
    k = h * np.sqrt(1.0 + (X / w) ** 2 + (Y / w) ** 2) / (w - h)
    px = np.floor((0.5 * X / w + 1.0) * 0.5 * W)
    py = (H - 1) - np.floor((0.5 * Y / w + 1.0) * 0.5 * H)
    hx, hy = np.ceil(0.25 * W * k) + 1, np.ceil(0.25 * H * k) + 1
    c0, c1 = np.maximum(px - hx, 0), np.minimum(px + hx, W - 1)
    r0, r1 = np.maximum(py - hy, 0), np.minimum(py + hy, H - 1)
    return hull_fits(c0, r0, np.where(r1 >= r0, c1, c0 - 1), r1)


def test_both_kinds_of_workgroup_occur_in_every_launch():
    for ps in (1, 3, 9):
        assert splat_fits(state()[0], ps) == EXPECTED_FIT, f"point_size {ps}"
    assert column_fits(state()[0]) == EXPECTED_FIT


def speed_quartiles():
    v = np.sort(FF.scalar(state()[1], np.zeros(N, F), "speed"))
    lo, hi = float(v[N // 4]), float(v[3 * N // 4])
    assert v[0] < lo < hi < v[-1]
    return lo, hi


# (kind, options) of every frame rendered at 800 x 600; an uploaded state has no densities yet (rho = 0 on every
# row: density and pressure are constant fields, every pixel a tie that the depth alone decides)
FLAT = [("flat", dict(shade=s)) for s in ("flat", "count")]
FIELD = ([("field", dict(field=f)) for f in FF.FIELDS]
         + [("field", dict(field="speed", lo=speed_quartiles()[0], hi=speed_quartiles()[1])),
            ("field", dict(field="density", lo=-1.0, hi=1.0)), ("field", dict(field="pressure", lo=-0.5, hi=3.0))])
COLUMN = [("column", dict()), ("column", dict(lo=0.25, hi=2.0))]
POINTS = [(k, dict(o, point_size=ps)) for ps in (1, 9) for k, o in (FLAT[1], FIELD[0])]


def gpu_frame(sim, kind, opt):
    if kind == "flat":
        out = dict(rgb=sim.render(**opt))
        out.update(sim.frame_buffers())
    elif kind == "field":
        sim.render_field(**opt)
        out = dict(rgb=np.array(sim.frame_host(), copy=True), value=sim.field_buffer(), range=sim.field_range())
        out.update(sim.frame_buffers())
    else:
        sim.render_column(**opt)
        out = dict(rgb=np.array(sim.frame_host(), copy=True), column=sim.column_buffer(), range=sim.column_range())
    return out


@functools.lru_cache(maxsize=None)
def restated(kind, items):
    """the restatement of a frame of the uploaded state (rho = 0), computed once per frame"""
    pos, vel = state()
    opt = dict(items)
    if kind == "flat":
        return R.render(pos, width=W, height=H, point_size=opt.get("point_size", 3), shade=opt["shade"])
    if kind == "field":
        return FF.render_field(pos, vel, np.zeros(N, F), width=W, height=H, **opt)
    want = CF.render_column(pos, settings().h, settings().d_kernel_coeff, width=W, height=H, **opt)
    assert want.pop("border") == 0, "a contribution on the border of the restatement's box"
    del want["edge"]   # (no call serves the edge layer behind a column frame; it is in the RGB)
    return want


def assert_frames_equal(got, want, what):
    assert got.keys() == want.keys(), what
    for k in got:
        if k == "range":
            ga, wa = (np.array(x[k], F).view(np.uint32).tolist() for x in (got, want))
            assert ga == wa, f"{what}: range {got[k]} vs {want[k]}"
            continue
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = a != b
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {a.size} entries differ, first at {np.argwhere(bad)[0]}"


def uploaded():
    sim = sph.Simulator(settings())
    sim.upload_state(*state())
    st = sim.download_state()
    assert np.array_equal(st["pos"], state()[0]) and not st["rho"].any()
    return sim


def check_both_paths(frames, monkeypatch):
    """every frame tiled and on the check path, each path on a handle of its own, against the restatement and each other"""
    got = {}
    for plain in ("0", "1"):
        monkeypatch.setenv("SPH_RENDER_PLAIN", plain)
        sim = uploaded()
        got[plain] = [gpu_frame(sim, kind, opt) for kind, opt in frames]
        sim.close()
    for i, (kind, opt) in enumerate(frames):
        want = restated(kind, tuple(sorted(opt.items())))
        assert_frames_equal(got["0"][i], want, f"tiled, {kind} {opt}")
        assert_frames_equal(got["1"][i], got["0"][i], f"plain vs tiled, {kind} {opt}")
        filled = got["0"][i]["column" if kind == "column" else "count"]
        assert (filled[290:310, 390:410] != 0).any()                          # the clusters
        assert (filled[:, :300] != 0).any() and (filled[:, 500:] != 0).any()  # the spread rows, either side of them


# point sizes 1 and 9: the smallest and the largest widening of the box of the centres
@pytest.mark.parametrize("frames", [FLAT, FIELD, COLUMN, POINTS], ids=["flat", "field", "column", "point_sizes"])
def test_tile_and_fallback_in_one_launch(frames, monkeypatch):
    check_both_paths(frames, monkeypatch)


def test_one_handle_flat_field_column_flat(monkeypatch):
    # the shared clear leaves nothing of the previous kind behind: same image size, every frame its restatement
    monkeypatch.setenv("SPH_RENDER_PLAIN", "0")
    sim = uploaded()
    for kind, opt in (FLAT[1], FIELD[0], COLUMN[0], FLAT[0], COLUMN[1], FIELD[3]):
        want = restated(kind, tuple(sorted(opt.items())))
        assert_frames_equal(gpu_frame(sim, kind, opt), want, f"in sequence: {kind} {opt}")
    sim.close()
