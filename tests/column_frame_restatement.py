"""The column frame restated in numpy, operation by operation.

Every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its
own like the strict-fp32 device code.  Shares no code with the HIP side; the projection and the box-edge
layer are those of render_restatement.py, the quantiser is the field frame's (field_frame_restatement.py).

Two forms: `brute=True` tests every particle against every pixel, as the definition reads; the default
visits, per particle, a box around its own pixel at least as wide as the bound of section 10h and reports
how many contributions fell on the border of that box (none may: a miss would hide behind the bound)."""
import numpy as np

import field_frame_restatement as FF
import render_restatement as R

F = np.float32
U64 = np.uint64
MASS = F(0.02)
K = F(32) / F(35)
CAP = F(1048576)            # 2^20: terms at or above it count 2^52
TWO32 = F(4294967296)
TO_VALUE = F(2.3283064365386963e-10)   # 2^-32
BOX_LIMIT = 48              # half-widths beyond it: the particle is tested against every pixel


def rays(width, height):
    """(ax per column, ay per row): the rays through the pixel centres, row 0 on top"""
    W, H = F(width), F(height)
    c = np.arange(width).astype(F)
    r = (height - 1 - np.arange(height)).astype(F)
    ax = F(2) * (((c + F(0.5)) / (F(0.5) * W)) - F(1))
    ay = F(2) * (((r + F(0.5)) / (F(0.5) * H)) - F(1))
    assert ax.dtype == F and ay.dtype == F
    return ax, ay


def camera_space(pos):
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    return pos[:, 0] - F(5), pos[:, 1] - F(5), F(15) - pos[:, 2]


def a2_of(X, Y, w, ax, ay, h2):
    """h2 minus the squared distance from the particle to the ray, taken from the ray's point at the particle's depth"""
    with np.errstate(all="ignore"):
        inv = F(1) / ((F(1) + ax * ax) + ay * ay)
        ex = X - ax * w
        ey = Y - ay * w
        t = ex * ax + ey * ay
        b2 = (ex * ex + ey * ey) - (t * t) * inv
        a2 = h2 - b2
    assert a2.dtype == F
    return a2


def terms(a2, coeff):
    """the uint64 term of every pair: 0 unless a2 > 0 (a NaN is not)"""
    a2 = np.asarray(a2, dtype=F)
    q = np.zeros(a2.shape, U64)
    hit = a2 > 0
    a = a2[hit]
    with np.errstate(all="ignore"):
        c = (MASS * (((F(coeff) * a) * a) * a)) * (K * np.sqrt(a))
    assert c.dtype == F
    t = np.zeros(c.shape, U64)
    small = (c > 0) & (c < CAP)          # (a NaN and a negative c: 0)
    t[small] = (c[small] * TWO32).astype(U64)
    t[c >= CAP] = U64(1 << 52)
    q[hit] = t
    return q


def boxes(pos, width, height, h):
    """own pixel (px, py), half-widths (hx, hy) of the bound -- rounded up, plus one -- and which particles it holds
    for (w > h); evaluated in float64: the box may be wider than the bound, never narrower"""
    with np.errstate(all="ignore"):   # (a particle that is not finite: its pixel is not used)
        px, py, _ = R.project(pos, width, height)
    X, Y, w = (a.astype(np.float64) for a in camera_space(pos))
    h = float(F(h))
    with np.errstate(all="ignore"):
        sp = np.sqrt(1.0 + (X / w) ** 2 + (Y / w) ** 2)
        k = h * sp / (w - h)
        hx = np.ceil(0.25 * width * k * (1 + 1e-9)) + 1
        hy = np.ceil(0.25 * height * k * (1 + 1e-9)) + 1
    finite = np.isfinite(X) & np.isfinite(Y) & np.isfinite(w)
    bounded = finite & (w - h > 0) & (hx <= BOX_LIMIT) & (hy <= BOX_LIMIT)
    hx = np.where(bounded, hx, 0).astype(np.int64)
    hy = np.where(bounded, hy, 0).astype(np.int64)
    return px, py, hx, hy, bounded, finite & ~bounded


def column_buffer(pos, h, coeff, width=800, height=600, brute=False, hits=None):
    """((height, width) uint64 column words, contributions on a box border); hits: a flat int64 array of width x height
    entries that counts the non-zero terms per pixel (bounded form)"""
    X, Y, w = camera_space(pos)
    ax, ay = rays(width, height)
    h2 = F(h) * F(h)
    col = np.zeros(width * height, U64)
    n = len(X)
    if brute:
        every, border = np.arange(n), 0
    else:
        px, py, hx, hy, bounded, wide = boxes(pos, width, height, h)
        every, border = np.nonzero(wide)[0], 0    # (a non-finite particle gives NaN or infinite b2 on every ray: nothing)
        idx = np.nonzero(bounded)[0]
        for dy in range(-int(hy[idx].max(initial=0)), int(hy[idx].max(initial=0)) + 1):
            rows = idx[abs(dy) <= hy[idx]]
            for dx in range(-int(hx[rows].max(initial=0)), int(hx[rows].max(initial=0)) + 1):
                i = rows[abs(dx) <= hx[rows]]
                c, r = px[i] + dx, py[i] + dy
                ok = (c >= 0) & (c < width) & (r >= 0) & (r < height)
                i, c, r = i[ok], c[ok], r[ok]
                q = terms(a2_of(X[i], Y[i], w[i], ax[c], ay[r], h2), coeff)
                np.add.at(col, r * width + c, q)
                if hits is not None:
                    np.add.at(hits, (r * width + c)[q > 0], 1)
                border += int(((q > 0) & ((abs(dx) == hx[i]) | (abs(dy) == hy[i]))).sum())
    chunk = max(1, (1 << 22) // (width * height))
    col = col.reshape(height, width)
    for k in range(0, len(every), chunk):
        i = every[k:k + chunk]
        a2 = a2_of(X[i, None, None], Y[i, None, None], w[i, None, None], ax[None, None, :], ay[None, :, None], h2)
        col += terms(a2, coeff).sum(axis=0, dtype=U64)   # (uint64 wraps: the sum is modulo 2^64)
    return col, border


def value(words):
    """the scalar of a column word: one conversion to float32 (round to nearest even), then an exact scaling"""
    return np.asarray(words, dtype=U64).astype(F) * TO_VALUE


def ramp(q):
    """(..., 3) uint8: thin film (223, 239, 255) at q = 0 to deep water (0, 48, 128) at q = 255, integers only"""
    q = np.asarray(q, dtype=np.int64)
    return np.stack([223 - ((7 * q) >> 3), 239 - ((3 * q) >> 2), 255 - (q >> 1)], axis=-1).astype(np.uint8)


def compose(col, edge, lo, hi):
    rgb = np.zeros(col.shape + (3,), np.uint8)
    hit = col != 0
    rgb[hit] = ramp(FF.quantise(value(col[hit]), lo, hi))
    rgb[edge != R.EMPTY] = (255, 255, 255)   # the fluid is translucent: no depth test
    return rgb


def render_column(pos, h, coeff, lo=0.0, hi=0.0, width=800, height=600, brute=False):
    lo, hi = F(lo), F(hi)
    assert np.isfinite(lo) and np.isfinite(hi) and not hi < lo
    col, border = column_buffer(pos, h, coeff, width, height, brute)
    if lo == 0 and hi == 0:   # automatic: from +0 to the value of the largest word
        lo, hi = F(0), value(col.max(initial=0))
    edge = R.edge_buffer(width, height)
    return dict(column=col, edge=edge, range=(F(lo), F(hi)), rgb=compose(col, edge, lo, hi), border=border)
