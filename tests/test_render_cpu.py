"""The frame renderer's surface and definition, checked without a GPU: the library exports the
render entry points, header / binding / version agree, and the numpy restatement of the image
definition (tests/render_restatement.py) gives the answers worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sph_render_frame", "sph_frame_host", "sph_download_frame_buffers",
               "sph_get_render_time", "sph_api_version"]
BITS = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731


def test_library_exports_the_render_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    exported = set(re.findall(r" T (sph_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTED_SYMBOLS, name


def test_header_binding_and_library_agree_on_version_3():
    text = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
    assert re.search(r"#define\s+SPH_API_VERSION\s+3\b", text)
    assert _lib.SPH_API_VERSION == 3
    assert sph.load_library().sph_api_version() == 3  # needs no device
    assert re.search(r"SPH_SHADE_FLAT\s*=\s*0", text) and re.search(r"SPH_SHADE_COUNT\s*=\s*1", text)
    assert (_lib.SPH_SHADE_FLAT, _lib.SPH_SHADE_COUNT) == (0, 1)


def test_render_options_layout():
    assert C.sizeof(_lib.SphRenderOptions) == 20
    assert [f[0] for f in _lib.SphRenderOptions._fields_] == ["struct_size", "width", "height", "point_size", "shade"]
    assert C.sizeof(sph.SphOptions) == 28  # unchanged


def test_box_corners_land_on_the_pixels_worked_by_hand():
    # front face z = 10 (w = 5): xw = (0.5 * -+5 / 5 + 1) * 400 = 200 / 600, yw = 150 / 450
    # back face z = 0 (w = 15): xw = (1 -+ 1/6) * 400 = 333.33.. / 466.66.., yw = 250 / 350
    want = {(0, 0, 10): (200, 449), (10, 0, 10): (600, 449), (10, 10, 10): (600, 149), (0, 10, 10): (200, 149),
            (0, 0, 0): (333, 349), (10, 0, 0): (466, 349), (10, 10, 0): (466, 249), (0, 10, 0): (333, 249)}
    for p, (col, row) in want.items():
        px, py, wb = R.project(np.array([p], np.float32), 800, 600)
        assert (int(px[0]), int(py[0])) == (col, row), p
        assert int(wb[0]) == BITS(15.0 - p[2])
    # the click box of display.cpp:22-32 is the front face
    assert (200, 600, 150, 450) == (200, 600, 600 - 450, 600 - 150)
    edge = R.edge_buffer()
    for col, row in want.values():
        assert edge[row, col] != R.EMPTY


def test_one_particle_at_the_box_centre():
    out = R.render(np.array([[5, 5, 5]], np.float32))
    ys, xs = np.nonzero(out["count"])
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(x, y) for x in (399, 400, 401) for y in (298, 299, 300)]
    assert (out["count"][out["count"] > 0] == 1).all()
    assert (out["depth"][out["count"] > 0] == BITS(10.0)).all()
    assert (out["depth"][out["count"] == 0] == R.EMPTY).all()
    assert (out["rgb"][299, 400] == (0, 0, 255)).all()
    assert (out["rgb"][0, 0] == (0, 0, 0)).all()


def test_two_particles_on_one_pixel_keep_the_nearer_depth_and_both_counts():
    depth, count = R.particle_buffers(np.array([[5, 5, 2], [5, 5, 8]], np.float32), point_size=1)
    assert count[299, 400] == 2 and count.sum() == 2
    assert depth[299, 400] == BITS(7.0)  # z = 8 is nearer: w = 7 < 13


def test_edge_against_particle_depth():
    # a sample near the middle of the edge (10,0,0)-(10,0,10): w just under 10
    px, py, wb = R.project(R.edge_points()[9 * R.EDGE_SAMPLES + 2048:][:1], 800, 600)
    col, row = int(px[0]), int(py[0])
    edge = R.edge_buffer()
    e = int(edge[row, col])
    assert e != int(R.EMPTY)
    count = np.zeros((600, 800), np.uint32)
    count[row, col] = 1
    for d, colour in ((e + 1, (255, 255, 255)),   # edge in front of the particle: white
                      (e, (255, 255, 255)),       # equal depth: lines were drawn first, GL_LESS keeps them
                      (e - 1, (0, 0, 255))):      # particle in front: blue
        depth = np.full((600, 800), R.EMPTY, np.uint32)
        depth[row, col] = d
        assert tuple(R.compose(depth, count, edge)[row, col]) == colour, d
    depth = np.full((600, 800), R.EMPTY, np.uint32)
    assert tuple(R.compose(depth, np.zeros_like(count), edge)[row, col]) == (255, 255, 255)


def test_particle_in_a_viewport_corner_is_clipped_not_wrapped():
    # 4 x 4 image: x = y = 0, z = 10 -> xw = yw = 1 -> column 1, row 2; point size 5 reaches past three borders
    depth, count = R.particle_buffers(np.array([[0, 0, 10]], np.float32), width=4, height=4, point_size=5)
    assert count.tolist() == [[1, 1, 1, 1]] * 4
    depth, count = R.particle_buffers(np.array([[0, 0, 10]], np.float32), width=4, height=4, point_size=3)
    assert count.tolist() == [[0, 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]]


def test_count_shade_levels():
    count = np.array([[0, 1, 2, 3, 4, 127, 128, 100000]], np.uint32)
    depth = np.where(count > 0, np.uint32(1), R.EMPTY).astype(np.uint32)
    edge = np.full_like(depth, R.EMPTY)
    rgb = R.compose(depth, count, edge, "count")[0]
    assert rgb.tolist() == [[0, 0, 0], [0, 0, 255], [32, 32, 255], [32, 32, 255], [64, 64, 255],
                            [192, 192, 255], [224, 224, 255], [224, 224, 255]]
