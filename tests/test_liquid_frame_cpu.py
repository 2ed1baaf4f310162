"""The liquid frame's surface and definition, checked without a GPU: the library exports the two entry points,
header and binding agree, the API version stays 3, and the numpy restatement of the definition
(tests/liquid_frame_restatement.py) gives the answers worked by hand, agrees with its own
brute-force form and stays close to float64 evaluations of the exact geometry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import column_frame_restatement as CF
import liquid_frame_restatement as LF
import render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
NEW_SYMBOLS = ["sph_render_liquid", "sph_download_liquid_buffers"]
F = np.float32
U32 = np.uint32
EMPTY = LF.EMPTY
# h and the poly6 coefficient of every default run, as tests/test_column_frame_cpu.py forms them
H = F(0.1)
COEFF = F(315.0) / (F(64.0) * F(3.14159265) * F(float(H) ** 9))


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))["pos_1"]


def plane_of(values):
    """a plane of depth bits from floats, NaN = empty"""
    v = np.asarray(values, dtype=F)
    return np.where(np.isnan(v), EMPTY, LF.bits(v))


# ---- the surface ----

def test_library_exports_the_liquid_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    exported = set(re.findall(r" T (sph_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER), name
        assert hasattr(sph.load_library(), name)
    for name in ("render_liquid", "liquid_buffers"):
        assert callable(getattr(sph.Simulator, name)), name


def test_version_stays_3_and_the_feature_macro_is_there():
    assert re.search(r"#define\s+SPH_API_VERSION\s+3\b", HEADER)
    assert _lib.SPH_API_VERSION == 3
    assert sph.load_library().sph_api_version() == 3  # needs no device
    assert re.search(r"#define\s+SPH_HAS_LIQUID_FRAME\s+1\b", HEADER)
    assert _lib.SPH_HAS_LIQUID_FRAME == 1


def test_header_and_binding_agree_on_the_struct():
    body = re.search(r"typedef struct SphLiquidFrameOptions \{(.*?)\} SphLiquidFrameOptions;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([\w\s,\[\]]+);", body):
        decl += [(n.strip(), ctype) for n in names.split(",")]
    assert decl == [("struct_size", "int32_t"), ("width", "int32_t"), ("height", "int32_t"), ("radius", "float"),
                    ("smooth_iterations", "int32_t"), ("smooth_radius", "int32_t"), ("smooth_depth", "float"),
                    ("light[3]", "float"), ("thickness_scale", "float")]
    ctypes_of = {"int32_t": C.c_int32, "float": C.c_float}
    want = [(n, ctypes_of[t]) if n != "light[3]" else ("light", C.c_float * 3) for n, t in decl]
    assert [n for n, _ in _lib.SphLiquidFrameOptions._fields_] == [n for n, _ in want]
    for (_, a), (_, b) in zip(_lib.SphLiquidFrameOptions._fields_, want):
        assert C.sizeof(a) == C.sizeof(b) and a._type_ == b._type_
    assert C.sizeof(_lib.SphLiquidFrameOptions) == 44
    assert [getattr(_lib.SphLiquidFrameOptions, n).offset for n, _ in _lib.SphLiquidFrameOptions._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 40]
    assert C.sizeof(_lib.SphColumnFrameOptions) == 20 and C.sizeof(_lib.SphFieldFrameOptions) == 28  # unchanged


def test_cli_and_class_know_the_frame():
    text = open(os.path.join(ROOT, "include", "simulator.h")).read()
    assert re.search(r"renderLiquid\s*\(\s*int \*width, int \*height\)", text)
    assert '"liquid"' in open(os.path.join(ROOT, "cudafluidsimulator_amd", "csrc", "headless.cpp")).read()


# ---- 1. the two forms of the front buffer ----

@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("size", [(64, 48), (333, 77)])
@pytest.mark.parametrize("name", ["random4096", "dense4096", "grid2048"])
def test_bounded_equals_brute_force(name, size, scale):
    pos = golden(name)
    r = F(scale) * H
    brute, _ = LF.front_buffer(pos, r, *size, brute=True)
    bounded, border = LF.front_buffer(pos, r, *size)
    assert (brute != EMPTY).any()
    assert np.array_equal(bounded, brute)
    assert border == 0, "a contribution on the border of the bounding box: the bound may hide a miss"


# ---- 2. by hand ----

def test_one_particle_on_the_axis():
    ax, ay = CF.rays(33, 33)
    assert ax[16] == 0 and ay[16] == 0
    one = np.array([[5, 5, 5]], F)
    for brute in (True, False):
        out = LF.render_liquid(one, H, COEFF, width=33, height=33, brute=brute)
        ys, xs = np.nonzero(out["front"] != EMPTY)
        assert list(zip(xs.tolist(), ys.tolist())) == [(16, 16)]
        # on the axis t = 0, b2 = 0, inv = 1: the depth of the sphere's pole
        wf = F(10) - np.sqrt(H * H)
        assert out["front"][16, 16] == LF.bits(wf) and out["smooth"][16, 16] == LF.bits(wf)   # (no neighbour to blend)
        assert out["normals"][16, 16].tolist() == [0, 0, 1] and not out["normals"][0, 0].any()
        assert np.array_equal(out["column"], CF.column_buffer(one, H, COEFF, 33, 33, brute=True)[0])
        assert out["scale"] == CF.value(out["column"][16, 16])
        # the colour: N = V = (0, 0, 1), tau = 1 (the pixel's own column is the frame's largest)
        L = np.array(LF.DEFAULT_LIGHT, F)
        L = L / np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
        S = np.array([L[0], L[1], L[2] + F(1)], F)
        Hh = S / np.sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2])
        spec = Hh[2]
        for _ in range(6):
            spec = spec * spec
        fres = F(0.02) + F(0.98) * F(0)
        lit = F(0.25) + F(0.75) * L[2]
        want = []
        for kappa, sky in ((6, 0.75), (2, 0.85), (0.75, 1.0)):
            T = F(1) / (F(1) + F(kappa) * F(1))
            col = ((F(1) - fres) * (T * lit) + fres * F(sky)) + spec
            assert type(col) is F
            want.append(int(min(max(col, F(0)), F(1)) * F(255) + F(0.5)))
        assert out["rgb"][16, 16].tolist() == want and 0 < want[0] < want[1] < want[2] < 255   # water: blue over green over red
        assert out["rgb"][0, 0].tolist() == [0, 0, 0]
        assert out["edge"][16, 16] == EMPTY


def test_near_plane_and_rows_that_are_not_finite():
    one = np.array([[5, 5, 5]], F)
    base = LF.front_buffer(one, H, 33, 33, brute=True)[0]
    # w = 0.5: in front of the near plane; w = 1.05: the centre is behind it, the entry point (0.95) is not
    for z in (14.5, 13.95):
        near = np.array([[5, 5, z]], F)
        for brute in (True, False):
            assert (LF.front_buffer(near, H, 33, 33, brute=brute)[0] == EMPTY).all(), (z, brute)
            assert np.array_equal(LF.front_buffer(np.concatenate([one, near]), H, 33, 33, brute=brute)[0], base)
    # w = 1.2: the pole lies at 1.1, behind the plane, and counts
    just = LF.front_buffer(np.array([[5, 5, 13.8]], F), H, 33, 33, brute=True)[0]
    assert just[16, 16] != EMPTY and just[16, 16].view(F) >= 1
    odd = np.array([[5, 5, 5], [np.nan, 5, 5], [5, np.inf, 5], [5, 5, -np.inf], [5, 5, np.nan]], F)
    for brute in (True, False):
        assert np.array_equal(LF.front_buffer(odd, H, 33, 33, brute=brute)[0], base)
    # the nearer of two spheres on one ray wins, whatever the order of the rows
    two = np.array([[5, 5, 5], [5, 5, 7]], F)
    for rows in (two, two[::-1]):
        got = LF.front_buffer(rows, H, 33, 33, brute=True)[0]
        assert got[16, 16] == LF.bits(F(8) - np.sqrt(H * H))


# ---- 3. the geometry against float64 ----

def exact_front_f64(pos, radius, width, height):
    """float64, the exact ray-sphere entry depth with rays in float64: the smallest root s of |s d - C|^2 = r^2,
    d = (ax, ay, -1), C = (X, Y, -w), which is the depth since d_z = -1; NaN where no sphere at or behind the near
    plane is hit.  Over the same boxes (checked against brute force above)."""
    px, py, hx, hy, bounded, wide = CF.boxes(pos, width, height, radius)
    assert bounded.all()
    p = np.asarray(pos, np.float64)
    Cc = np.stack([p[:, 0] - 5.0, p[:, 1] - 5.0, p[:, 2] - 15.0], axis=1)
    ax = 2.0 * ((np.arange(width) + 0.5) / (0.5 * width) - 1.0)
    ay = 2.0 * (((height - 1 - np.arange(height)) + 0.5) / (0.5 * height) - 1.0)
    front = np.full(width * height, np.inf)
    r2 = float(radius) ** 2
    for dy in range(-int(hy.max()), int(hy.max()) + 1):
        for dx in range(-int(hx.max()), int(hx.max()) + 1):
            i = np.nonzero((abs(dx) <= hx) & (abs(dy) <= hy))[0]
            c, r = px[i] + dx, py[i] + dy
            ok = (c >= 0) & (c < width) & (r >= 0) & (r < height)
            i, c, r = i[ok], c[ok], r[ok]
            d = np.stack([ax[c], ay[r], -np.ones(len(i))], axis=1)
            dd, dc, cc = (d * d).sum(1), (d * Cc[i]).sum(1), (Cc[i] ** 2).sum(1)
            disc = dc * dc - dd * (cc - r2)
            s = (dc - np.sqrt(np.maximum(disc, 0.0))) / dd
            hit = (disc > 0) & (s >= 1.0)
            np.minimum.at(front, (r * width + c)[hit], s[hit])
    return front.reshape(height, width)


# Measured with this restatement on random4096 at 800 x 600: the largest absolute error of wf over the pixels both
# evaluations fill.  Four times that is allowed, for other libm and numpy builds.
MEASURED_WF_ABS = 7.825e-05   # (27064 pixels; none filled by one of the two evaluations only)


def test_against_float64_exact_geometry():
    pos = golden("random4096")
    got, border = LF.front_buffer(pos, H, 800, 600)
    want = exact_front_f64(pos, H, 800, 600)
    both = (got != EMPTY) & np.isfinite(want)
    either = (got != EMPTY) | np.isfinite(want)
    err = np.abs(got.view(F)[both].astype(np.float64) - want[both]).max()
    print(f"largest absolute error of wf = {err:.3e} over {int(both.sum())} pixels; "
          f"{int(either.sum() - both.sum())} pixels filled by one evaluation only (grazing rays)")
    assert border == 0 and both.sum() > 10000
    assert either.sum() - both.sum() <= 1e-3 * both.sum()
    assert err <= 4 * MEASURED_WF_ABS


# ---- 4. the smoothing ----

def noisy_plane(shape=(24, 40), seed=3, holes=True):
    rng = np.random.default_rng(seed)
    v = (F(9) + F(0.05) * rng.standard_normal(shape)).astype(F)
    if holes:
        v[rng.random(shape) < 0.2] = np.nan
    return plane_of(v)


def test_smoothing_identities():
    z = noisy_plane()
    assert np.array_equal(LF.smooth(z, 0, 3, 0.2), z) and np.array_equal(LF.smooth(z, 3, 0, 0.2), z)
    out = LF.smooth(z, 3, 3, 0.2)
    assert np.array_equal(out == EMPTY, z == EMPTY), "empty stays empty, and nothing else becomes empty"
    assert (out != z).any()
    # a constant plane stays bit-constant, holes and borders included
    flat = np.where(z == EMPTY, EMPTY, LF.bits(F(9.3)))
    for k in (1, 3, 7):
        assert np.array_equal(LF.smooth(flat, 4, k, 0.2), flat)
    # every iteration reads the previous plane only: two passes are the pass of the pass
    assert np.array_equal(LF.smooth(z, 2, 2, 0.2), LF.smooth_once(LF.smooth_once(z, 2, 0.2), 2, 0.2))


def test_smoothing_respects_depth_steps():
    v = np.full((16, 32), 9, F)
    v[:, 16:] = F(9.5)   # a silhouette: a step of 0.5
    z = plane_of(v)
    assert np.array_equal(LF.smooth(z, 3, 3, 0.2), z), "a step larger than delta must not blend"
    assert np.array_equal(LF.smooth(z, 3, 3, 0.5), z), "a step of exactly delta has weight 0"
    out = LF.smooth(z, 1, 3, 1.0).view(F)
    assert (out[:, 13:16] > 9).all() and (out[:, 16:19] < F(9.5)).all(), "a step smaller than delta blends"
    assert (out[:, :13] == 9).all() and (out[:, 19:] == F(9.5)).all()   # ... within k pixels of it only
    assert (np.diff(out[8].astype(np.float64)) >= 0).all()
    # the worked weight of one neighbour: k = 1, the pixel left of the step sees three pixels of the other side
    one = LF.smooth(z, 1, 1, 1.0).view(F)[8, 15]
    d, g = F(0.5), F(1) - F(0.5) * F(0.5)
    s1, s2 = F(1) - F(1) / F(3), F(1) - F(2) / F(3)
    num, den = F(0), F(1)
    # (in the order of the definition: dy = -1: dx = -1, 0, 1; dy = 0: dx = -1, 1; dy = 1 ...; same-depth neighbours add
    # their weight to den, g = 1, and nothing to num)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            s = s2 if dx and dy else s1
            if dx == 1:
                wgt = (s * s) * (g * g)
                num, den = num + wgt * d, den + wgt
            else:
                den = den + (s * s) * (F(1) * F(1))
    assert one == F(9) + num / den


def test_smoothing_at_its_limits_is_finite():
    z = noisy_plane((40, 56), seed=5)
    out = LF.smooth(z, 8, 7, 0.2)
    assert np.isfinite(out[out != EMPTY].view(F)).all() and np.array_equal(out == EMPTY, z == EMPTY)
    v = out[out != EMPTY].view(F)
    assert v.min() >= z[z != EMPTY].view(F).min() and v.max() <= z[z != EMPTY].view(F).max()
    assert v.std() < 0.5 * z[z != EMPTY].view(F).std()
    for size in ((1, 1), (3, 5)):   # smaller than the window
        small = noisy_plane(size, holes=False)
        assert np.isfinite(LF.smooth(small, 8, 7, 1.0).view(F)).all()


# ---- 5. the normals ----

def tilted_plane(width, height, n=(0.3, -0.2, 1.0), depth=10.0):
    """the depth bits of the plane n . P = n . (0, 0, -depth) under every pixel's ray, and its unit normal"""
    n = np.array(n, np.float64)
    n /= np.sqrt((n * n).sum())
    ax, ay = (a.astype(np.float64) for a in CF.rays(width, height))
    z = (-depth * n[2]) / (n[0] * ax[None, :] + n[1] * ay[:, None] - n[2])
    return plane_of(z.astype(F)), n


# Measured on the 96 x 64 plane below: the largest difference of a component from the plane's own normal (the depths
# are rounded to fp32, eps 1e-6 at z = 10, against differences between neighbours of some 0.01).  Four times that is
# allowed.
MEASURED_NORMAL_ABS = 6.0e-06


def test_normal_of_a_tilted_plane():
    z, n = tilted_plane(96, 64)
    N = LF.normals(z).astype(np.float64)
    err = np.abs(N - n).max()
    length = np.abs(np.sqrt((N * N).sum(-1)) - 1).max()
    print(f"largest error of a normal component = {err:.3e}; of the length = {length:.3e}")
    assert err <= 4 * MEASURED_NORMAL_ABS and length <= 1e-6
    # beside empty pixels and at the viewport border the one-sided differences still lie in the plane
    rng = np.random.default_rng(11)
    holes = z.copy()
    holes[rng.random(z.shape) < 0.25] = EMPTY
    M = LF.normals(holes).astype(np.float64)
    here = holes != EMPTY
    lone_x = here & ~LF.shifted(here, 1, 0, False) & ~LF.shifted(here, -1, 0, False)
    lone_y = here & ~LF.shifted(here, 0, 1, False) & ~LF.shifted(here, 0, -1, False)
    ok = here & ~lone_x & ~lone_y
    assert lone_x.any() and lone_y.any() and ok.sum() > 1000
    assert np.abs(M[ok] - n).max() <= 4 * MEASURED_NORMAL_ABS
    assert not M[~here].any()


def test_normal_fallbacks():
    alone = plane_of([[np.nan, np.nan, np.nan], [np.nan, 9, np.nan], [np.nan, np.nan, np.nan]])
    assert LF.normals(alone)[1, 1].tolist() == [0, 0, 1]
    assert LF.normals(plane_of([[7]]))[0, 0].tolist() == [0, 0, 1]
    # one row: Ty falls back to (0, 1, 0), N = Tx x (0, 1, 0) = (-Tx.z, 0, Tx.x) normalised
    row = plane_of([[9, 9.01, 9.03]])
    ax, ay = CF.rays(3, 1)
    N = LF.normals(row)
    P = [np.array([ax[c] * row.view(F)[0, c], ay[0] * row.view(F)[0, c], -row.view(F)[0, c]], F) for c in range(3)]
    for c, T in ((0, P[1] - P[0]), (1, P[1] - P[0]), (2, P[2] - P[1])):   # the middle pixel: the smaller |dz| is behind it
        raw = np.array([F(0) * F(0) - T[2] * F(1), T[2] * F(0) - T[0] * F(0), T[0] * F(1) - F(0) * F(0)], F)
        want = raw / np.sqrt((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2])
        assert N[0, c].tolist() == want.tolist(), c
    # a tie takes the forward difference: equal steps on both sides
    tie = plane_of([[9, 9.5, 10]])
    T = np.array([ax[2] * F(10) - ax[1] * F(9.5), ay[0] * F(10) - ay[0] * F(9.5), F(-10) - F(-9.5)], F)
    raw = np.array([-T[2], F(0), T[0]], F)
    want = raw / np.sqrt((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2])
    assert LF.normals(tie)[0, 1].tolist() == want.tolist()
    # a degenerate cross product (NaN or zero length): (0, 0, 1)
    assert LF.normals(plane_of([[np.inf, np.inf]]))[0, 0].tolist() == [0, 0, 1]


# ---- 6. bytes and the edge test ----

def test_byte_conversion():
    eps = np.finfo(F).eps
    col = np.array([0, 1, -1, 2, np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 127.5 / 255, 254.5 / 255, 1 - eps / 2], F)
    tie = lambda k: int(F(F(k + 0.5) / F(255)) * F(255) + F(0.5))   # (whichever way the fp32 product falls)
    assert LF.to_byte(col).tolist() == [0, 255, 0, 255, 0, 255, 0, tie(0), tie(1), tie(127), tie(254), 255]
    assert LF.to_byte(np.array([0.999 / 255 / 2, 0.4999 / 255, 0.5001 / 255], F)).tolist() == [0, 0, 1]
    assert LF.to_byte(F(0.5)) == 128   # 127.5 + 0.5 = 128 exactly: a tie goes up


def test_edge_test_on_both_sides_of_equality():
    edge = R.edge_buffer(64, 48)
    ys, xs = np.nonzero(edge != EMPTY)
    assert len(ys) >= 4
    front = np.full((48, 64), EMPTY, U32)
    cells = [(ys[k], xs[k]) for k in range(3)]
    front[cells[0]] = edge[cells[0]]          # equal: the edge wins (GL_LESS, lines drawn first)
    front[cells[1]] = edge[cells[1]] + U32(1)  # the edge is nearer: white
    front[cells[2]] = edge[cells[2]] - U32(1)  # the water is nearer: its colour
    free = np.argwhere(edge == EMPTY)[0]
    front[tuple(free)] = F(9).view(U32)
    column = np.where(front != EMPTY, np.uint64(1 << 32), np.uint64(0))
    rgb, _ = LF.compose(front, front, column, edge, LF.DEFAULT_LIGHT, F(1))
    assert rgb[cells[0]].tolist() == [255] * 3 and rgb[cells[1]].tolist() == [255] * 3
    assert rgb[cells[2]].tolist() != [255] * 3 and rgb[cells[2]].any()
    assert rgb[tuple(free)].any() and rgb[tuple(free)].tolist() != [255] * 3
    # empty pixels: white on an edge, black elsewhere
    rest = front == EMPTY
    assert (rgb[rest & (edge != EMPTY)] == 255).all() and not rgb[rest & (edge == EMPTY)].any()
    # thickness: no column behind a pixel (or a scale of 0) leaves the water clear, more column darkens red first
    clear, _ = LF.compose(front, front, np.zeros_like(column), edge, LF.DEFAULT_LIGHT, F(1))
    none, _ = LF.compose(front, front, column, edge, LF.DEFAULT_LIGHT, F(0))
    assert np.array_equal(clear, none)
    a, b = clear[tuple(free)].astype(int), rgb[tuple(free)].astype(int)
    assert (a > b).all() and a[0] - b[0] > a[2] - b[2]
