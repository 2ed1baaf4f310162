"""Ray casting without a GPU: what the library, the header, the binding, the C++ class and the CLI declare; the
restatement (tests/ray_cast_restatement.py) held to itself -- its layer walk against its brute force, word for word
and with nothing in the padding -- to cases worked by hand, to the liquid frame's restatement through the reference
camera and to float64 through an oblique one; the shading and the edge cylinders by hand.

Figures measured with the committed restatement on random4096:
  against LF.front_buffer, reference camera, near = 1: largest |t - wf| = 5.7220458984375e-06 (200 x 150, r = h), no
  pixel filled by one side only; the bound below is four times that;
  against float64 ray-sphere entry, oblique camera 64 x 48: largest |t - exact| = 2.1316574306595726e-05 (r = h, t up
  to 17.3: eleven ulp, at grazing hits, where the entry moves fastest with b2); the bound below is four times that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import liquid_frame_restatement as LF
import ray_cast_restatement as RC
import ray_sets as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F = np.float32
H, D, BOX = 0.1, 100, 10.0
FRONT_DIFF = 5.7220458984375e-06     # measured, see above
EXACT_DIFF = 2.1316574306595726e-05  # measured, see above
MISS = RC.MISS


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))["pos_1"]


def one(o, d, tmin=0.0, tmax=np.inf):
    return RC.make_rays([o], [d], tmin, tmax)


def cast(pos, rays, radius=0.0):
    """brute force and walk agree; -> (t, ids)"""
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    b = RC.brute(pos, rays, H, D, radius)
    w, padding, _, _ = RC.walk(pos, rays, H, D, radius)
    assert np.array_equal(b, w) and padding == 0
    return RC.split(b)


# ---- what is declared ----

def header():
    return open(os.path.join(ROOT, "include", "sph_c_api.h")).read()


def test_library_exports_the_entry_points():
    L = sph.load_library()
    for name in ("sph_cast_rays", "sph_cast_host", "sph_render_view", "sph_download_view_buffer", "sph_get_cast_stats"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert L.sph_api_version() == 3 == _lib.SPH_API_VERSION
    assert re.search(r"^#define SPH_HAS_RAY_CAST 1$", header(), re.M) and _lib.SPH_HAS_RAY_CAST == 1
    assert re.search(r"^#define SPH_API_VERSION 3\b", header(), re.M)


def header_struct(name):
    """[(field, C type, array length or None)] of a struct of the header"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", header(), flags=re.S), re.S).group(1)
    out = []
    for ctype, names in re.findall(r"(\w+)\s+([^;]+);", body):
        for field in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", field)
            out.append((m.group(1), ctype, int(m.group(2)) if m.group(2) else None))
    return out


@pytest.mark.parametrize("name, size", [("SphRay", 32), ("SphCastOptions", 8), ("SphViewOptions", 96), ("SphCastStats", 48)])
def test_header_and_binding_agree_on_the_structs(name, size):
    ctypes_of = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    struct = getattr(_lib, name)
    want = [(f, ctypes_of[t] * k if k else ctypes_of[t]) for f, t, k in header_struct(name)]
    assert [(f, t) for f, t in struct._fields_] == want
    assert C.sizeof(struct) == size
    if name == "SphRay":
        assert _lib.ray_dtype().itemsize == 32 and [_lib.ray_dtype().fields[f][1] for f in ("o", "t_min", "d", "t_max")] == [0, 12, 16, 28]


def test_the_class_and_the_cli_know_the_view():
    for method in ("cast_rays", "cast_words", "render_view", "view_buffer", "cast_stats"):
        assert callable(getattr(sph.Simulator, method)), method
    cpp = open(os.path.join(ROOT, "include", "simulator.h")).read()
    assert "castRays" in cpp and "renderView" in cpp
    cli = open(os.path.join(ROOT, "cudafluidsimulator_amd", "csrc", "headless.cpp")).read()
    assert "SPH_FREE_VIEW" in cli and "view_%04d.ppm" in cli
    assert b"SPH_FREE_VIEW" in open(os.path.join(ROOT, "cudafluidsimulator_amd", "sph"), "rb").read()
    assert _lib.VIEW_SHADES == dict(flat=0, speed=1, density=2, pressure=3)


# ---- the walk against brute force ----

@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("name", ["random4096", "dense4096", "grid2048"])
def test_walk_equals_brute_force(name, scale):
    pos = golden(name)
    r = F(scale) * F(H)
    hits = 0
    for key, rays in RS.ray_sets(pos, H, D, BOX).items():
        b = RC.brute(pos, rays, H, D, r)
        w, padding, tests, _ = RC.walk(pos, rays, H, D, r)
        assert np.array_equal(b, w), f"{name}, r = {scale} h, {key}: {int((b != w).sum())} words differ"
        assert padding == 0, f"{name}, r = {scale} h, {key}: {padding} contributions in the padding"
        assert tests <= len(rays) * len(pos)
        hits += int((b != MISS).sum())
        if key in ("stray", "invalid"):
            assert (b == MISS).all(), key
    assert hits > 50, (name, scale, hits)


def test_the_walk_tests_few_candidates():
    pos = golden("random4096")
    rays = np.concatenate([RS.camera_rays(RS.REFERENCE, 64, 48, H), RS.camera_rays(RS.OBLIQUE, 64, 48, H)])
    _, _, tests, layers = RC.walk(pos, rays, H, D, F(H))
    assert tests < len(rays) * len(pos) // 100 and layers <= len(rays) * D


# ---- by hand ----

@pytest.mark.parametrize("radius", [0.0, 0.1, 0.07])
def test_one_particle_one_ray(radius):
    r = F(radius) if radius else F(0.5) * F(H)
    want = F(10) - np.sqrt(r * r)
    t, ids = cast([[5, 5, 5]], one((5, 5, 15), (0, 0, -1)), radius)
    assert t[0].view(np.uint32) == want.view(np.uint32) and ids[0] == 0
    # d scaled by 1024 and by 1 / 1024: t scales the other way (powers of two: exactly)
    for k in (1024.0, 1.0 / 1024.0):
        ts, _ = cast([[5, 5, 5]], one((5, 5, 15), (0, 0, -k)), radius)
        assert ts[0].view(np.uint32) == F(want / F(k)).view(np.uint32)


def test_a_tie_goes_to_the_smaller_id():
    a, b = [5 + 0.03, 5, 5], [5 - 0.03, 5, 5]    # mirrored about the ray: the same operations up to signs
    for pos in ([a, b], [b, a]):
        w = RC.brute(np.array(pos, F), one((5, 5, 15), (0, 0, -1)), H, D, 0.1)
        w2, padding, _, _ = RC.walk(np.array(pos, F), one((5, 5, 15), (0, 0, -1)), H, D, 0.1)
        assert w[0] == w2[0] != MISS and padding == 0
        assert int(w[0]) & 0xFFFFFFFF == 0
    alone = RC.brute(np.array([b], F), one((5, 5, 15), (0, 0, -1)), H, D, 0.1)
    assert alone[0] == w[0], "the two entries are not equal: not a tie"


def test_the_windows():
    pos = [[5, 5, 5], [5, 5, 3]]
    t, ids = cast(pos, one((5, 5, 15), (0, 0, -1)), 0.1)
    first = t[0]
    assert ids[0] == 0
    before, after = np.nextafter(first, F(0)), np.nextafter(first, F(np.inf))
    t2, ids2 = cast(pos, one((5, 5, 15), (0, 0, -1), 0, before), 0.1)
    assert ids2[0] == -1 and np.isinf(t2[0])                       # t_max just before the first entry
    t3, ids3 = cast(pos, one((5, 5, 15), (0, 0, -1), after, np.inf), 0.1)
    assert ids3[0] == 1 and t3[0] > first                          # t_min just past it: the second sphere answers
    t4, ids4 = cast(pos, one((5, 5, 15), (0, 0, -1), first, first), 0.1)
    assert ids4[0] == 0 and t4[0] == first                         # t_min == t_max
    t5, ids5 = cast(pos, one((5, 5, 15), (0, 0, -1), 0, first), 0.1)
    assert ids5[0] == 0                                            # the window's ends belong to it
    t6, ids6 = cast(pos, one((5, 5, 15), (0, 0, -1), after, after), 0.1)
    assert ids6[0] == -1


def test_a_ray_that_starts_inside_a_sphere_does_not_see_it():
    pos = [[5, 5, 5], [5, 5, 4.5]]
    t, ids = cast(pos, one((5, 5, 5.05), (0, 0, -1)), 0.1)
    assert ids[0] == 1 and t[0] > 0
    t, ids = cast(pos[:1], one((5, 5, 5.05), (0, 0, -1)), 0.1)
    assert ids[0] == -1
    # on the sphere itself: the entry is at t = 0, stored as +0
    w = RC.brute(np.array(pos[:1], F), one((5, 5, 5.1), (0, 0, -1)), H, D, 0.1)
    t, ids = RC.split(w)
    assert ids[0] in (0, -1) and (ids[0] == -1 or t[0].view(np.uint32) < 0x80000000)


def test_rows_that_are_not_finite_or_outside_the_grid_are_not_hit():
    ray = one((5, 5, 15), (0, 0, -1))
    for bad in ([np.nan, 5, 5], [5, np.inf, 5], [5, 5, -0.01], [5, 5, 10.0], [5, 5, 12.0], [-1.0, 5, 5]):
        t, ids = cast([bad, [5, 5, 2]], one((bad[0] if np.isfinite(bad[0]) else 5, bad[1] if np.isfinite(bad[1]) else 5, 15), (0, 0, -1)), 0.1)
        assert ids[0] in (1, -1), bad
    t, ids = cast([[5, 5, 10.0], [5, 5, 2]], ray, 0.1)
    assert ids[0] == 1      # z = 10 is z / h = 100 = D: outside, although its sphere would be met first
    t, ids = cast([[5, 5, float(np.nextafter(F(10), F(0)))], [5, 5, 2]], ray, 0.1)
    assert ids[0] == 0      # the last float below it is inside


def test_invalid_rays_miss():
    pos = golden("random4096")
    rays = RS.invalid_rays(BOX)
    assert not RC.valid(rays, H, D).any()
    t, ids = cast(pos, rays, 0.1)
    assert (ids == -1).all()
    # at the ends of what is valid a ray hits: dd = 2^-40, dd = 2^40, |o_a| = 64 boxes, each through particle 7
    edge = RS.boundary_rays(pos[7], H, D)
    assert RC.valid(edge, H, D).all()
    assert RC.dd_of(edge)[0] == F(2.0 ** -40) and RC.dd_of(edge)[1] == F(2.0 ** 40) and edge[2, 2] == F(64) * (F(D) * F(H))
    t, ids = cast(pos, edge, 0.1)
    assert (ids >= 0).all() and np.isfinite(t).all()
    assert t[0] > 2.0 ** 19 and t[1] < 2.0 ** -18 and 600 < t[2] < 640    # (up to a quarter box away, over |d| = 2^-20 and 2^20)
    # ... and one step beyond each end it misses
    beyond = edge.copy()
    beyond[0, 6], beyond[1, 5], beyond[2, 2] = np.nextafter(edge[0, 6], F(0)), np.nextafter(edge[1, 5], F(np.inf)), np.nextafter(edge[2, 2], F(np.inf))
    assert not RC.valid(beyond, H, D).any() and (cast(pos, beyond, 0.1)[1] == -1).all()


# ---- against the liquid frame's restatement, and against float64 ----

@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("size", [(200, 150), (333, 77)])
def test_the_reference_camera_sees_the_liquid_frames_front(size, scale):
    pos = golden("random4096")
    w, hh = size
    r = F(scale) * F(H)
    cam = RC.camera(RS.REFERENCE["eye"], RS.REFERENCE["target"], RS.REFERENCE["up"], w, hh, RS.REFERENCE["tan_half"], near=1.0, h=H)
    rays = RC.view_rays(cam)
    # d = (ax, ay, -1) with exactly section 10h's ax, ay
    import column_frame_restatement as CF
    ax, ay = CF.rays(w, hh)
    d = rays[:, 4:7].reshape(hh, w, 3)
    assert np.array_equal(d[..., 0].view(np.uint32), np.broadcast_to(ax[None, :], (hh, w)).view(np.uint32))
    assert np.array_equal(d[..., 1].view(np.uint32), np.broadcast_to(ay[:, None], (hh, w)).view(np.uint32))
    assert (d[..., 2] == -1).all() and (rays[:, 3] == 1).all() and np.isinf(rays[:, 7]).all()
    words, padding, _, _ = RC.walk(pos, rays, H, D, r)
    assert padding == 0
    t, ids = RC.split(words)
    front, border = LF.front_buffer(pos, r, w, hh)
    assert border == 0
    mine, theirs = (ids >= 0).reshape(hh, w), front != LF.EMPTY
    assert np.array_equal(mine, theirs), f"{int((mine != theirs).sum())} pixels filled by one side only"
    assert mine.sum() > 500
    wf = np.where(theirs, front, np.uint32(0)).view(F)
    diff = np.abs(t.reshape(hh, w).astype(np.float64) - wf.astype(np.float64))[mine].max()
    print(f"{w} x {hh}, r = {scale} h: {int(mine.sum())} pixels, largest |t - wf| = {diff!r}")
    assert diff <= 4 * FRONT_DIFF


def exact_entries(pos, rays, r):
    """float64: the smallest root of |o + t d - p| = r inside the window, inf where there is none"""
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    p = pos.astype(np.float64)
    best = np.full(len(rays), np.inf)
    for k in range(0, len(rays), 256):
        e = p[None, :, :] - o[k:k + 256, None, :]
        dd = (d[k:k + 256] ** 2).sum(axis=1)[:, None]
        b = (e * d[k:k + 256, None, :]).sum(axis=2)
        disc = b * b - dd * ((e ** 2).sum(axis=2) - float(r) ** 2)
        with np.errstate(all="ignore"):
            t = (b - np.sqrt(np.where(disc > 0, disc, np.nan))) / dd
        t = np.where((t >= rays[k:k + 256, 3, None]) & (t <= rays[k:k + 256, 7, None]), t, np.inf)
        best[k:k + 256] = t.min(axis=1)
    return best


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_an_oblique_camera_against_float64(scale):
    pos = golden("random4096")
    r = F(scale) * F(H)
    rays = RS.camera_rays(RS.OBLIQUE, 64, 48, H)
    words, padding, _, _ = RC.walk(pos, rays, H, D, r)
    t, ids = RC.split(words)
    exact = exact_entries(pos, rays, r)
    hit = ids >= 0
    # a sphere grazed within the error of b2 may be seen by one side only; none is here
    assert np.array_equal(hit, np.isfinite(exact)) and hit.sum() > 500
    err = np.abs(t[hit].astype(np.float64) - exact[hit]).max()
    print(f"oblique 64 x 48, r = {scale} h: {int(hit.sum())} hits, largest |t - exact| = {err!r}")
    assert err <= 4 * EXACT_DIFF
    # the winner is the sphere float64 finds, or one whose entry is as near within the error
    p = pos[ids[hit]].astype(np.float64)
    at = rays[hit, 0:3].astype(np.float64) + exact[hit, None] * rays[hit, 4:7].astype(np.float64)
    assert (np.abs(np.sqrt(((at - p) ** 2).sum(axis=1)) - float(r)) <= 4 * EXACT_DIFF * np.sqrt(3.0) * 2).all()


# ---- the camera, the shading and the edges by hand ----

def test_the_basis():
    fwd, s, u = RC.basis((5, 5, 15), (5, 5, 0), (0, 1, 0))
    assert [float(v) for v in fwd] == [0, 0, -1] and [float(v) for v in s] == [1, 0, 0] and [float(v) for v in u] == [0, 1, 0]
    assert RC.basis((5, 5, 15), (5, 5, 15), (0, 1, 0)) is None and RC.basis((5, 5, 15), (5, 5, 0), (0, 0, 2)) is None
    assert RC.basis((5, 5, 15), (np.nan, 5, 0), (0, 1, 0)) is None and RC.basis((5, 5, 15), (5, 5, 0), (0, 0, 0)) is None
    cam = RC.camera((1, 2, 3), (4, 5, 6), width=800, height=600, h=H)
    assert cam["tan"][1] == F(0.41421357) and cam["tan"][0] == F(0.41421357) * (F(800) / F(600)) and cam["near"] == F(H) and np.isinf(cam["far"])


def hand_view(pos, shade="flat", vel=None, rho=None, **opt):
    """a 1 x 1 view from (5, 5, 15) down -z: the centre ray is (0, 0, -1)"""
    pos = np.array(pos, F).reshape(-1, 3)
    vel = np.zeros_like(pos) if vel is None else np.array(vel, F)
    rho = np.zeros(len(pos), F) if rho is None else np.array(rho, F)
    cam = RC.camera((5, 5, 15), (5, 5, 0), (0, 1, 0), 1, 1, (2, 2), h=H)
    rays = RC.view_rays(cam)
    assert np.array_equal(rays[0], F([5, 5, 15, H, 0, 0, -1, np.inf]))
    return RC.render_view(pos, vel, rho, H, D, cam, 0.1, shade, box=BOX, **opt), cam, rays


def test_the_hand_worked_hit_is_lit_as_the_formula_says():
    out, cam, rays = hand_view([[5, 5, 5]], edge_radius=-1.0)
    t, ids = RC.split(out["words"].reshape(-1))
    assert ids[0] == 0 and t[0] == F(10) - np.sqrt(F(0.1) * F(0.1))
    # P = (5, 5, 15 - t), n0 = (0, 0, (15 - t) - 5): the normal is (0, 0, 1)
    n0z = (F(15) + t[0] * F(-1)) - F(5)
    assert n0z > 0 and n0z / np.sqrt((F(0) + F(0)) + n0z * n0z) == F(1)
    L = F(RC.DEFAULT_LIGHT)
    Lz = L[2] / np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
    lit = F(0.25) + F(0.75) * ((F(0) * F(1) + F(0) * F(1)) + F(1) * Lz)
    want = [int(np.uint32(c * lit * F(255) + F(0.5))) for c in RC.FLAT]
    assert out["rgb"][0, 0].tolist() == want and want[2] > want[1] > want[0] > 0
    # a light from behind: the ambient term alone; from the eye: the base colour itself
    dark, _, _ = hand_view([[5, 5, 5]], edge_radius=-1.0, light=(0.0, 0.0, -1.0))
    assert dark["rgb"][0, 0].tolist() == [int(np.uint32(c * F(0.25) * F(255) + F(0.5))) for c in RC.FLAT]
    full, _, _ = hand_view([[5, 5, 5]], edge_radius=-1.0, light=(0.0, 0.0, 3.0))
    assert full["rgb"][0, 0].tolist() == [int(np.uint32(c * F(255) + F(0.5))) for c in RC.FLAT]
    # a field shade: the ramp's bytes over 255, lit; a fixed scale and the automatic one of one particle (q = 0: blue)
    fast, _, _ = hand_view([[5, 5, 5]], "speed", vel=[[3, 0, 4]], edge_radius=-1.0, lo=0.0, hi=10.0, light=(0.0, 0.0, 3.0))
    assert fast["rgb"][0, 0].tolist() == [0, 255, 0]          # q = 128: green
    auto, _, _ = hand_view([[5, 5, 5]], "speed", vel=[[3, 0, 4]], edge_radius=-1.0, light=(0.0, 0.0, 3.0))
    assert auto["rgb"][0, 0].tolist() == [0, 0, 255]
    # no hit, no edge: black
    none, _, _ = hand_view([[5, 8, 5]], edge_radius=-1.0)
    assert none["words"][0, 0] == MISS and none["rgb"][0, 0].tolist() == [0, 0, 0]


def test_an_edge_in_front_of_at_and_behind_a_hit():
    # the centre ray of a 1 x 1 view from (0, 5, 15) down -z runs along x = 0: it meets the edge along y through
    # (x, z) = (0, 10) at te = 5 - rho, and the sphere of radius r at (0, 5, z) at t = (15 - z) - r
    def view(z, rho, r=0.1):
        pos = np.array([[0.0, 5.0, z]], F)
        cam = RC.camera((0, 5, 15), (0, 5, 0), (0, 1, 0), 1, 1, (2, 2), h=H)
        out = RC.render_view(pos, np.zeros_like(pos), np.zeros(1, F), H, D, cam, r, edge_radius=rho, box=BOX)
        te = RC.edge_entries(RC.view_rays(cam), BOX, F(rho) if rho > 0 else F(1))
        return out["rgb"][0, 0].tolist(), RC.split(out["words"].reshape(-1))[0][0], te[0]

    white = [255, 255, 255]
    rgb, t, te = view(9.0, 0.25)           # the sphere is entered at 5.9, the edge at 4.75: far in front
    assert te == F(5) - np.sqrt(F(0.25) * F(0.25)) and t == F(6) - np.sqrt(F(0.1) * F(0.1)) and te < t and rgb == white
    sphere, t, te = view(9.0, -1.0)        # no edges: the sphere's colour
    assert sphere != white and any(sphere)
    # at: binary fractions make an exact tie.  r = 0.0625 at z = 9.96875 is entered at 5.03125 - 0.0625, the edge of
    # radius 0.03125 at 5 - 0.03125: both 4.96875.  The edge wins the tie.
    z = F(9.96875)
    rgb, t, te = view(z, 0.03125, 0.0625)
    assert t == te == F(4.96875) and rgb == white
    colour = view(z, -1.0, 0.0625)[0]
    assert colour != white and any(colour)
    # just in front and just behind: one ulp of z to either side moves t by exactly that ulp (every operation is exact)
    ulp = np.spacing(z)
    rgb, t, te = view(np.nextafter(z, F(0)), 0.03125, 0.0625)          # the sphere one ulp further: the edge just in front
    assert t == F(4.96875) + ulp and te == F(4.96875) and rgb == white
    rgb, t, te = view(np.nextafter(z, F(20)), 0.03125, 0.0625)         # the sphere one ulp nearer: the edge just behind
    assert t == F(4.96875) - ulp and te == F(4.96875) and rgb == colour
    # far behind: an eye inside the box below the edge sees the sphere
    pos = np.array([[0.0, 5.0, 12.0 - 3.0]], F)
    cam = RC.camera((0, 5, 9.5), (0, 5, 0), (0, 1, 0), 1, 1, (2, 2), h=H)
    out = RC.render_view(pos, np.zeros_like(pos), np.zeros(1, F), H, D, cam, 0.1, edge_radius=0.25, box=BOX)
    te = RC.edge_entries(RC.view_rays(cam), BOX, F(0.25))[0]
    t = RC.split(out["words"].reshape(-1))[0][0]
    assert t == F(0.5) - np.sqrt(F(0.1) * F(0.1)) and te == F(9.5) - np.sqrt(F(0.25) * F(0.25)) and t < te   # the edge along y through (0, 0)
    assert out["rgb"][0, 0].tolist() != [255, 255, 255] and out["rgb"][0, 0].any()
    # an edge is as long as the box: the same ray outside y in [0, 10] meets none
    cam = RC.camera((0, 10.5, 15), (0, 10.5, 0), (0, 1, 0), 1, 1, (2, 2), h=H)
    assert np.isinf(RC.edge_entries(RC.view_rays(cam), BOX, F(0.25))[0])
    cam = RC.camera((0, 10.0, 15), (0, 10.0, 0), (0, 1, 0), 1, 1, (2, 2), h=H)
    assert np.isfinite(RC.edge_entries(RC.view_rays(cam), BOX, F(0.25))[0])    # its end belongs to it
