"""The column frame's surface and definition, checked without a GPU: the library exports the three entry
points, header and binding agree, the API version stays 3, and the numpy restatement of the definition
(tests/column_frame_restatement.py) gives the answers worked by hand, agrees with its
own brute-force form and stays close to a float64 evaluation of the exact geometry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import column_frame_restatement as CF
import field_frame_restatement as FF
import render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "sph_c_api.h")).read()
NEW_SYMBOLS = ["sph_render_column", "sph_download_column_buffer", "sph_column_range"]
F = np.float32
# h = 0.1 and the poly6 coefficient of every default run, formed in fp32 the way main() does (main.cpp:57-63) --
# written out here, not asked of the library: importing this module must not load it (test_defaults_are_the_library's)
H = F(0.1)
COEFF = F(315.0) / (F(64.0) * F(3.14159265) * F(float(H) ** 9))


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))["pos_1"]


def test_defaults_are_the_librarys():
    s = sph.default_settings(4096, True)
    assert F(s.h) == H and F(s.d_kernel_coeff) == COEFF


def test_library_exports_the_column_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", sph.library_path()], text=True)
    exported = set(re.findall(r" T (sph_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER), name
        assert hasattr(sph.load_library(), name)
    for name in ("render_column", "column_buffer", "column_range"):
        assert callable(getattr(sph.Simulator, name)), name


def test_version_stays_3_and_the_feature_macro_is_there():
    assert re.search(r"#define\s+SPH_API_VERSION\s+3\b", HEADER)
    assert _lib.SPH_API_VERSION == 3
    assert sph.load_library().sph_api_version() == 3  # needs no device
    assert re.search(r"#define\s+SPH_HAS_COLUMN_FRAME\s+1\b", HEADER)
    assert _lib.SPH_HAS_COLUMN_FRAME == 1


def test_header_and_binding_agree_on_the_struct():
    body = re.search(r"typedef struct SphColumnFrameOptions \{(.*?)\} SphColumnFrameOptions;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", body):
        decl += [(n.strip(), ctype) for n in names.split(",")]
    assert decl == [("struct_size", "int32_t"), ("width", "int32_t"), ("height", "int32_t"),
                    ("value_lo", "float"), ("value_hi", "float")]
    ctypes_of = {"int32_t": C.c_int32, "float": C.c_float}
    assert _lib.SphColumnFrameOptions._fields_ == [(n, ctypes_of[t]) for n, t in decl]
    assert C.sizeof(_lib.SphColumnFrameOptions) == 20
    assert [getattr(_lib.SphColumnFrameOptions, n).offset for n, _ in decl] == [0, 4, 8, 12, 16]
    assert C.sizeof(_lib.SphFieldFrameOptions) == 28 and C.sizeof(_lib.SphRenderOptions) == 20  # unchanged


def test_one_particle_on_the_axis_hits_exactly_the_centre_pixel():
    # 33 x 33: the ray through the centre of pixel (16, 16) is the axis itself, ax = ay = 0
    ax, ay = CF.rays(33, 33)
    assert ax[16] == 0 and ay[16] == 0
    out = CF.render_column(np.array([[5, 5, 5]], F), H, COEFF, width=33, height=33, brute=True)
    ys, xs = np.nonzero(out["column"])
    assert list(zip(xs.tolist(), ys.tolist())) == [(16, 16)]
    # b2 = 0: a2 = h2, and the word is the definition's expression written out
    h2 = H * H
    c = (F(0.02) * (((COEFF * h2) * h2) * h2)) * ((F(32) / F(35)) * np.sqrt(h2))
    assert c.dtype == F
    word = int(c * F(4294967296))
    assert int(out["column"][16, 16]) == word
    # ... and MASS coeff (32/35) h^7 in float64 (2.8647897 against 2.8647890 with the default settings)
    exact = 0.02 * float(COEFF) * (32.0 / 35.0) * float(H) ** 7
    assert abs(word / 2.0 ** 32 - exact) <= 1e-6 * exact
    # automatic range: hi is its own value, q = 255, deep water
    assert out["range"] == (F(0), CF.value(word)) and tuple(out["rgb"][16, 16]) == (0, 48, 128)
    assert tuple(out["rgb"][0, 0]) == (0, 0, 0)
    # the bounded form sees the same
    assert np.array_equal(CF.render_column(np.array([[5, 5, 5]], F), H, COEFF, width=33, height=33)["column"], out["column"])


def test_sums_cap_and_nan():
    one = np.array([[5, 5, 5]], F)
    a = CF.column_buffer(one, H, COEFF, 33, 33, brute=True)[0]
    b = CF.column_buffer(np.repeat(one, 2, axis=0), H, COEFF, 33, 33, brute=True)[0]
    assert np.array_equal(b, a * np.uint64(2)) and int(b[16, 16]) == 2 * int(a[16, 16])
    # the cap: with the coefficient x 10^6 the term on the axis is 2.86e6 >= 2^20 and counts 2^52, two of them 2^53.
    # (Not every term of a frame: c falls with a^7, below 0.87 h it stays under 2^20 even then.)
    big = F(COEFF * F(1e6))
    assert int(CF.column_buffer(one, H, big, 33, 33, brute=True)[0][16, 16]) == 1 << 52
    assert int(CF.column_buffer(np.repeat(one, 2, axis=0), H, big, 33, 33, brute=True)[0][16, 16]) == 1 << 53
    a2 = np.linspace(0, float(H * H), 4097).astype(F)[1:]
    t = CF.terms(a2, big)
    assert (t[:-1] <= t[1:]).all() and int(t[-1]) == 1 << 52 and 0 < int(t[0]) < 1 << 52
    assert (t == 1 << 52).sum() > 1 and int(t[t < (1 << 52)].max()) < 1 << 52   # below the cap every term is below 2^52
    pos = golden("random4096")
    capped, _ = CF.column_buffer(pos, H, big, 64, 48, brute=True)
    plain, _ = CF.column_buffer(pos, H, COEFF, 64, 48, brute=True)
    assert ((capped != 0) == (plain != 0)).all() and (capped >= np.uint64(1 << 52)).any()
    # a NaN a2 is no hit; a NaN c (inf x 0 cannot arise here; a NaN coefficient can) is 0; so is a negative c
    assert CF.terms(np.array([np.nan, -1.0, 0.0], F), COEFF).tolist() == [0, 0, 0]
    assert CF.terms(np.array([1e-2], F), F(np.nan)).tolist() == [0]
    assert CF.terms(np.array([1e-2], F), F(-COEFF)).tolist() == [0]
    # a particle that is not finite adds nothing, in both forms
    odd = np.array([[5, 5, 5], [np.nan, 5, 5], [5, np.inf, 5], [5, 5, -np.inf]], F)
    assert np.array_equal(CF.column_buffer(odd, H, COEFF, 33, 33, brute=True)[0], a)
    assert np.array_equal(CF.column_buffer(odd, H, COEFF, 33, 33)[0], a)
    # a particle within h of the eye's plane is outside the bound: the bounded form tests it against every pixel
    near = np.array([[5, 5, 14.95], [4.9, 5.1, 14.8]], F)
    assert np.array_equal(CF.column_buffer(near, H, COEFF, 33, 33, brute=True)[0], CF.column_buffer(near, H, COEFF, 33, 33)[0])


def test_value_is_one_rounding_of_the_word():
    words = np.array([0, 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 32), (1 << 64) - 1], np.uint64)
    # ties to even at 2^24 + 1 -> 2^24 and 2^24 + 3 -> 2^24 + 4; 2^64 - 1 -> 2^64
    want = [0.0, 2.0 ** -32, 2.0 ** -8, (2.0 ** 24 + 4) * 2.0 ** -32, 1.0, 2.0 ** 32]
    assert CF.value(words).tolist() == want and CF.value(words).dtype == F


def test_quantiser_and_ramp():
    s = np.array([0, 1, 1.99, 2, 3, 4], F)
    assert FF.quantise(s, 1.0, 3.0).tolist() == [0, 0, 126, 128, 255, 255]   # both ends clip
    assert FF.quantise(s, 2.0, 2.0).tolist() == [0] * 6                      # hi == lo
    assert FF.quantise(s, 0.0, 4.0).tolist() == [0, 64, 127, 128, 192, 255]
    table = [(223 - ((7 * q) >> 3), 239 - ((3 * q) >> 2), 255 - (q >> 1)) for q in range(256)]
    assert all(0 <= c <= 255 for row in table for c in row)
    assert table[0] == (223, 239, 255) and table[255] == (0, 48, 128)
    assert [tuple(c) for c in CF.ramp(np.arange(256)).tolist()] == table
    # white wherever the edge layer has a sample, whatever lies behind; black where nothing is
    edge = R.edge_buffer(64, 48)
    col = np.zeros((48, 64), np.uint64)
    col[10, 10] = col[np.nonzero(edge != R.EMPTY)[0][0], np.nonzero(edge != R.EMPTY)[1][0]] = 1 << 32
    rgb = CF.compose(col, edge, 0.0, 2.0)
    assert (rgb[edge != R.EMPTY] == 255).all() and edge[10, 10] == R.EMPTY
    assert tuple(rgb[10, 10]) == table[128] and tuple(rgb[0, 0]) == (0, 0, 0)


@pytest.mark.parametrize("size", [(64, 48), (333, 77)])
@pytest.mark.parametrize("name", ["random4096", "dense4096", "grid2048"])
def test_bounded_equals_brute_force(name, size):
    pos = golden(name)
    brute, _ = CF.column_buffer(pos, H, COEFF, *size, brute=True)
    bounded, border = CF.column_buffer(pos, H, COEFF, *size)
    assert (brute != 0).any()
    assert np.array_equal(bounded, brute)
    assert border == 0, "a contribution on the border of the bounding box: the bound may hide a miss"


def exact_columns_f64(pos, h, coeff, width, height):
    """float64, the exact geometry |P|^2 - (P.d)^2 / |d|^2 with P = (X, Y, -w), d = (ax, ay, -1): the columns as
    float64 sums over the same boxes (checked against brute force above)"""
    px, py, hx, hy, bounded, wide = CF.boxes(pos, width, height, h)
    assert bounded.all()
    p = np.asarray(pos, np.float64)
    P = np.stack([p[:, 0] - 5.0, p[:, 1] - 5.0, p[:, 2] - 15.0], axis=1)
    ax = 2.0 * ((np.arange(width) + 0.5) / (0.5 * width) - 1.0)
    ay = 2.0 * (((height - 1 - np.arange(height)) + 0.5) / (0.5 * height) - 1.0)
    col = np.zeros(width * height)
    for dy in range(-int(hy.max()), int(hy.max()) + 1):
        for dx in range(-int(hx.max()), int(hx.max()) + 1):
            i = np.nonzero((abs(dx) <= hx) & (abs(dy) <= hy))[0]
            c, r = px[i] + dx, py[i] + dy
            ok = (c >= 0) & (c < width) & (r >= 0) & (r < height)
            i, c, r = i[ok], c[ok], r[ok]
            d = np.stack([ax[c], ay[r], -np.ones(len(i))], axis=1)
            b2 = (P[i] ** 2).sum(1) - (P[i] * d).sum(1) ** 2 / (d ** 2).sum(1)
            a2 = np.maximum(float(h) ** 2 - b2, 0.0)
            np.add.at(col, r * width + c, 0.02 * float(coeff) * (32.0 / 35.0) * a2 ** 3.5)
    return col.reshape(height, width)


# Measured with this restatement on random4096 at 800 x 600: the largest absolute error is MEASURED_ABS of the largest
# column.  Four times that is allowed, for other libm and numpy builds.
MEASURED_ABS = 1.956e-05   # (the largest relative error on pixels above 0.1 % of the largest column: 4.6e-04)


def test_against_float64_exact_geometry():
    pos = golden("random4096")
    got = CF.column_buffer(pos, H, COEFF, 800, 600)[0].astype(np.float64) / 2.0 ** 32
    want = exact_columns_f64(pos, H, COEFF, 800, 600)
    top = want.max()
    err = np.abs(got - want).max() / top
    big = want > 1e-3 * top
    rel = (np.abs(got - want)[big] / want[big]).max()
    print(f"largest absolute error / largest column = {err:.3e}; largest relative error above 0.1 % of it = {rel:.3e}")
    assert top > 0 and err <= 4 * MEASURED_ABS
