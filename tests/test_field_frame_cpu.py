"""The field frame's surface and definition, checked without a GPU: the library exports the three entry
points, header and binding agree, the API version stays 3, and the numpy restatement of the definition
(tests/field_frame_restatement.py) gives the answers worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import field_frame_restatement as FF
import render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
NEW_SYMBOLS = ["sph_render_field", "sph_download_field_buffer", "sph_field_range"]
F = np.float32
BITS = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731


def test_library_exports_the_field_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    exported = set(re.findall(r" T (sph_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER), name


def test_version_stays_3_and_the_feature_macro_is_there():
    assert re.search(r"#define\s+SPH_API_VERSION\s+3\b", HEADER)
    assert _lib.SPH_API_VERSION == 3
    assert sph.load_library().sph_api_version() == 3  # needs no device
    assert re.search(r"#define\s+SPH_HAS_FIELD_FRAME\s+1\b", HEADER)
    assert _lib.SPH_HAS_FIELD_FRAME == 1


def test_header_and_binding_agree_on_fields_and_struct():
    for k, name in enumerate(("SPH_FIELD_SPEED", "SPH_FIELD_DENSITY", "SPH_FIELD_PRESSURE")):
        assert re.search(r"%s\s*=\s*%d\b" % (name, k), HEADER), name
        assert getattr(_lib, name) == k
    assert _lib.FIELDS == {"speed": 0, "density": 1, "pressure": 2}
    body = re.search(r"typedef struct SphFieldFrameOptions \{(.*?)\} SphFieldFrameOptions;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", body):
        decl += [(n.strip(), ctype) for n in names.split(",")]
    assert decl == [("struct_size", "int32_t"), ("width", "int32_t"), ("height", "int32_t"), ("point_size", "int32_t"),
                    ("field", "int32_t"), ("value_lo", "float"), ("value_hi", "float")]
    ctypes_of = {"int32_t": C.c_int32, "float": C.c_float}
    assert _lib.SphFieldFrameOptions._fields_ == [(n, ctypes_of[t]) for n, t in decl]
    assert C.sizeof(_lib.SphFieldFrameOptions) == 28
    assert [getattr(_lib.SphFieldFrameOptions, n).offset for n, _ in decl] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(_lib.SphRenderOptions) == 20  # unchanged


def test_scalars():
    vel = np.array([[3, 4, 12], [0, 0, 0], [-1, 0, 0]], F)
    rho = np.array([998, 1000, 1003.5], F)
    assert FF.scalar(vel, rho, "speed").tolist() == [13.0, 0.0, 1.0]
    assert FF.scalar(vel, rho, "density").tolist() == [998.0, 1000.0, 1003.5]
    assert FF.scalar(vel, rho, "pressure").tolist() == [0.0, 0.0, 3.5]
    # each operation rounded on its own: 1e-23^2 underflows to a denormal, not to what a wider type gives
    tiny = np.array([[1e-23, 0, 0]], F)
    assert FF.scalar(tiny, rho[:1], "speed")[0] == np.sqrt(F(1e-23) * F(1e-23))


def test_one_particle_at_the_box_centre_with_a_known_velocity():
    pos, vel, rho = np.array([[5, 5, 5]], F), np.array([[3, 4, 12]], F), np.array([1000], F)
    out = FF.render_field(pos, vel, rho, "speed")
    ys, xs = np.nonzero(out["count"])
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(x, y) for x in (399, 400, 401) for y in (298, 299, 300)]
    hit = out["count"] > 0
    assert (out["value"][hit] == BITS(13.0)).all() and (out["value"][~hit] == FF.EMPTY).all()
    assert (out["depth"][hit] == BITS(10.0)).all() and (out["depth"][~hit] == FF.EMPTY).all()
    assert out["range"] == (F(13), F(13))                      # automatic: its own value at both ends ...
    assert tuple(out["rgb"][299, 400]) == (0, 0, 255)          # ... hi == lo: q = 0
    assert tuple(out["rgb"][0, 0]) == (0, 0, 0)
    # 13 on the scale 0..26: 0.5 * 256 = 128 exactly -> pure green
    out = FF.render_field(pos, vel, rho, "speed", lo=0.0, hi=26.0)
    assert out["range"] == (F(0), F(26)) and tuple(out["rgb"][299, 400]) == (0, 255, 0)
    # the same depth and count as the flat frame
    flat = R.render(pos)
    assert np.array_equal(out["depth"], flat["depth"]) and np.array_equal(out["count"], flat["count"])


def test_two_particles_at_different_depths_the_nearer_value_wins():
    pos = np.array([[5, 5, 2], [5, 5, 8]], F)
    vel = np.array([[1, 0, 0], [0, 7, 0]], F)   # the farther one has the SMALLER value: depth decides first
    out = FF.render_field(pos, vel, np.zeros(2, F), "speed", point_size=1)
    assert out["count"][299, 400] == 2 and out["count"].sum() == 2
    assert out["depth"][299, 400] == BITS(7.0) and out["value"][299, 400] == BITS(7.0)
    assert out["range"] == (F(1), F(7))         # the range covers the hidden particle too
    assert tuple(out["rgb"][299, 400]) == (255, 3, 0)   # s = hi: 256 clamps to q = 255


def test_two_particles_at_the_same_depth_the_smaller_value_wins():
    pos = np.array([[5, 5, 5], [5, 5, 5]], F)
    for speeds in ((5, 2), (2, 5)):
        vel = np.array([[speeds[0], 0, 0], [0, 0, speeds[1]]], F)
        out = FF.render_field(pos, vel, np.zeros(2, F), "speed", point_size=1)
        assert out["count"][299, 400] == 2
        assert out["depth"][299, 400] == BITS(10.0) and out["value"][299, 400] == BITS(2.0)


def test_colour_ramp_at_the_segment_ends():
    want = {0: (0, 0, 255), 63: (0, 252, 255), 64: (0, 255, 255), 127: (0, 255, 3),
            128: (0, 255, 0), 191: (252, 255, 0), 192: (255, 255, 0), 255: (255, 3, 0)}
    got = FF.ramp(np.array(sorted(want)))
    assert [tuple(c) for c in got.tolist()] == [want[q] for q in sorted(want)]
    # the whole table, written out from the four rows of the definition
    table = []
    for q in range(256):
        if q < 64:
            table.append((0, 4 * q, 255))
        elif q < 128:
            table.append((0, 255, 255 - 4 * (q - 64)))
        elif q < 192:
            table.append((4 * (q - 128), 255, 0))
        else:
            table.append((255, 255 - 4 * (q - 192), 0))
    assert all(0 <= c <= 255 for row in table for c in row)
    assert [tuple(c) for c in FF.ramp(np.arange(256)).tolist()] == table


def test_quantise():
    s = np.array([0, 1, 1.99, 2, 3, 4, 5], F)
    assert FF.quantise(s, 1.0, 3.0).tolist() == [0, 0, 126, 128, 255, 255, 255]   # clipped at both ends
    assert FF.quantise(s, 2.0, 2.0).tolist() == [0] * 7                           # hi == lo
    # (s - lo) and (hi - lo) both overflow: inf / inf = NaN -> q = 0; a finite s - lo over inf is 0
    big = F(3e38)
    assert FF.quantise(np.array([big, 0], F), -big, big).tolist() == [0, 0]
    # 1/3 of the way: floor(85.33) = 85
    assert FF.quantise(np.array([1], F), 0.0, 3.0).tolist() == [85]


def test_edge_in_front_of_a_particle_and_behind_it():
    px, py, wb = R.project(R.edge_points()[9 * R.EDGE_SAMPLES + 2048:][:1], 800, 600)
    col, row = int(px[0]), int(py[0])
    edge = R.edge_buffer()
    e = int(edge[row, col])
    assert e != int(R.EMPTY)
    count = np.zeros((600, 800), np.uint32)
    count[row, col] = 1
    value = BITS(2.0)                         # on the scale 0..4: q = 128, green
    for d, colour in ((e + 1, (255, 255, 255)),   # edge in front of the particle: white
                      (e, (255, 255, 255)),       # equal depth: lines were drawn first, GL_LESS keeps them
                      (e - 1, (0, 255, 0))):      # particle in front: its colour
        packed = np.full((600, 800), FF.EMPTY64, np.uint64)
        packed[row, col] = (d << 32) | value
        assert tuple(FF.compose(packed, count, edge, 0.0, 4.0)[row, col]) == colour, d
    packed = np.full((600, 800), FF.EMPTY64, np.uint64)
    assert tuple(FF.compose(packed, np.zeros_like(count), edge, 0.0, 4.0)[row, col]) == (255, 255, 255)
    assert tuple(FF.compose(packed, np.zeros_like(count), edge, 0.0, 4.0)[0, 0]) == (0, 0, 0)
