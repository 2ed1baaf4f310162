"""The surface mesh without a GPU: the numpy restatement (tests/surface_restatement.py) on
synthetic fields -- watertight, the right topology, the right side out, every vertex on its edge --, the tables of
csrc/surface_tables.h against the restatement's, and the C-ABI's new declarations."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import surface_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
H = 0.1          # the blobs' radius: f = A (H^2 - r^2)^3 inside it, 0 outside -- one particle's density
A = 2.0e7


def blob(shape, origin, spacing, centres, h=H):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(*[origin[2 - k] + np.arange(n) * spacing for k, n in enumerate((nz, ny, nx))], indexing="ij")
    f = np.zeros(shape)
    for c in centres:
        r2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
        f += np.where(r2 < h * h, A * (h * h - r2) ** 3, 0.0)
    return f.astype(F)


def radius_of(iso, h=H):
    return math.sqrt(h * h - (iso / A) ** (1.0 / 3.0))


def cases():
    sp = H / 8
    one = blob((21, 21, 21), (0.0, 0.0, 0.0), sp, [(10 * sp,) * 3])
    two = blob((33, 33, 33), (0.0, 0.0, 0.0), sp, [(10 * sp, 16 * sp, 16 * sp), (22 * sp, 16 * sp, 16 * sp)], h=5 * sp)
    rng = np.random.default_rng(5)
    noise = rng.random((9, 10, 11)).astype(F)
    noise[[0, -1]] = 0
    noise[:, [0, -1]] = 0
    noise[:, :, [0, -1]] = 0
    leaving = blob((21, 21, 21), (0.0, 0.0, 0.0), sp, [(2 * sp, 10 * sp, 19 * sp)])
    half = float(one.max()) / 2
    return {"one blob": (one, sp, half, True, 2),
            "iso on a lattice value": (one, sp, float(one[10, 10, 13]), True, 2),
            "two blobs": (two, sp, float(two.max()) / 2, True, 4),
            "noise": (noise, sp, 0.5, True, None),
            "leaving the lattice": (leaving, sp, half, False, None)}


CASES = cases()


@pytest.fixture(scope="module")
def meshes():
    return {name: SR.extract(f, (0.0, 0.0, 0.0), sp, iso) for name, (f, sp, iso, _, _) in CASES.items()}


def count_crossed_edges(f, iso):
    inside = f >= F(iso)
    n = 0
    for dx, dy, dz in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]:
        nz, ny, nx = f.shape
        n += int((inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]).sum())
    return n


@pytest.mark.parametrize("name", list(CASES))
def test_the_mesh_is_manifold_and_every_vertex_sits_on_its_edge(name, meshes):
    f, sp, iso, closed, chi = CASES[name]
    verts, tris, detail = meshes[name]
    assert len(tris) > 0 and tris.max() < len(verts) and verts.dtype == F and tris.dtype == np.uint32
    most, lone = SR.edge_pairing(tris)
    assert most == 1, "a directed edge occurs twice"
    if closed:
        assert len(lone) == 0, f"{len(lone)} directed edges without their reverse"
        assert 2 * (3 * len(tris) // 2) == 3 * len(tris)
    if chi is not None:
        assert SR.euler(verts, tris) == chi
    assert len(verts) == count_crossed_edges(f, iso)
    # 0 <= t <= 1, and the vertex lies in the box of its edge
    assert (detail["t"] >= 0).all() and (detail["t"] <= 1).all()
    nz, ny, nx = f.shape
    L, d = detail["L"], detail["d"]
    i = np.stack([L % nx, L // nx % ny, L // (nx * ny)], axis=1)
    off = np.array(SR.DIRS)[d]
    pa = (i.astype(F) * F(sp)).astype(F)
    pb = ((i + off).astype(F) * F(sp)).astype(F)
    assert (verts >= np.minimum(pa, pb)).all() and (verts <= np.maximum(pa, pb)).all()
    if name == "iso on a lattice value":
        assert (detail["t"] == 0).any(), "no vertex on a lattice point: the case is not covered"
        a, b, c = (verts[tris[:, k]] for k in range(3))
        assert ((a == b).all(1) | (b == c).all(1) | (a == c).all(1)).any(), "no degenerate triangle"


def test_the_blobs_have_their_outside_out_and_the_right_volume(meshes):
    for name in ("one blob", "iso on a lattice value", "two blobs"):
        assert SR.signed_volume(*meshes[name][:2]) > 0, name
    f, sp, iso, _, _ = CASES["one blob"]
    r = radius_of(iso)
    vol = SR.signed_volume(*meshes["one blob"][:2])
    lo, hi = (4 / 3 * math.pi * (r + s * math.sqrt(3) * sp) ** 3 for s in (-1, 1))
    assert lo < vol < hi, (lo, vol, hi)


def test_the_open_mesh_is_open_only_on_the_shell(meshes):
    f, sp, iso, _, _ = CASES["leaving the lattice"]
    verts, tris, _ = meshes["leaving the lattice"]
    _, lone = SR.edge_pairing(tris)
    assert len(lone) > 0, "the surface does not leave the lattice"
    nz, ny, nx = f.shape
    a, b = verts[lone[:, 0]], verts[lone[:, 1]]
    on_face = np.zeros(len(lone), bool)
    for axis, n in enumerate((nx, ny, nz)):
        for face in (F(0), F(n - 1) * F(sp)):
            on_face |= (a[:, axis] == face) & (b[:, axis] == face)
    assert on_face.all()


def test_nothing_crosses_nothing_comes_out():
    f = np.zeros((3, 4, 5), F)
    verts, tris, _ = SR.extract(f, (0, 0, 0), 0.1, 1.0)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)
    f[1, 1, 1] = np.nan                                      # a NaN is outside
    assert len(SR.extract(f, (0, 0, 0), 0.1, 1.0)[0]) == 0


# ---- csrc/surface_tables.h against the restatement's tables ----
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/surface_selftest.cpp under ASan + UBSan, run once: {name: [rows of ints]}"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("surface") / "surface_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "cudafluidsimulator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "surface_selftest.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and not p.stderr, f"sanitizer report or failure:\n{p.stderr}"
    out = {}
    for line in p.stdout.splitlines():
        name, *vals = line.split()
        out.setdefault(name, []).append([int(v) for v in vals])
    return out


def test_the_headers_tables_are_the_restatements(selftest):
    assert selftest["dir"] == [[d, SR.corner_number(off), SR.corner_number(off)] for d, off in enumerate(SR.DIRS)]
    assert selftest["path"] == [[s] + [SR.corner_number(c) for c in SR.tet_path(perm)] for s, perm in enumerate(SR.PERMS)]
    want = []
    for s in range(6):
        for case in range(16):
            tris = SR.TABLE[s][case]
            swapped = sum(1 << k for k, sw in enumerate(SR.SWAPPED[s][case]) if sw)
            want.append([s, case, len(tris), swapped] + [SR.corner_number(off) << 3 | d for tri in tris for off, d in tri])
    assert selftest["tet"] == want
    cells = []
    for b in range(256):
        n = 0
        for s, perm in enumerate(SR.PERMS):
            case = sum((b >> SR.corner_number(c) & 1) << p for p, c in enumerate(SR.tet_path(perm)))
            n += len(SR.TABLE[s][case])
        cells.append([b, n])
    assert selftest["cell"] == cells
    # both windings occur: the table is not one-sided by accident
    assert any(r[3] for r in selftest["tet"]) and any(r[2] and not r[3] for r in selftest["tet"])


# ---- the C-ABI's new declarations ----
def test_header_library_and_binding_carry_the_surface():
    text = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
    assert re.search(r"#define\s+SPH_HAS_SURFACE\s+1", text)
    names = ("sph_extract_surface", "sph_surface_host", "sph_get_surface_time")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.EXPORTED_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    exported = set(re.findall(r" T (sph_\w+)", out))
    assert set(names) <= exported
    assert C.sizeof(_lib.SphSurfaceOptions) == 44 and _lib.SphSurfaceOptions.iso.offset == 40
    m = re.search(r"typedef struct SphSurfaceOptions \{(.*?)\} SphSurfaceOptions;", code, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+([^;]+);", m.group(1))
    words = sum(len(decl.split(",")) * (3 if "[3]" in decl else 1) for _, decl in fields)
    assert words * 4 == 44
