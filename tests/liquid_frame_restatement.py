"""The liquid frame restated in numpy, operation by operation.

Every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its
own like the strict-fp32 device code.  Shares no code with the HIP side; the rays, the camera space, the
bounding boxes and the column words are those of column_frame_restatement.py, the box-edge layer is that of
render_restatement.py.

The front buffer comes in two forms: `brute=True` tests every particle against every pixel, as the definition
reads; the default visits, per particle, a box around its own pixel at least as wide as the bound of section 10h
for the sphere radius and reports how many contributions fell on the border of that box (none may)."""
import numpy as np

import column_frame_restatement as CF
import render_restatement as R

F = np.float32
U32 = np.uint32
EMPTY = R.EMPTY
DEFAULT_LIGHT = (-0.35, 0.8, 0.5)
KAPPA = (F(6), F(2), F(0.75))
SKY = (F(0.75), F(0.85), F(1.0))


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U32)


def front_words(X, Y, w, ax, ay, r2):
    """the word of every pair: the bits of the depth wf at which the ray enters the sphere, EMPTY unless a2 > 0 and
    wf >= 1 (a NaN is neither)"""
    with np.errstate(all="ignore"):
        inv = F(1) / ((F(1) + ax * ax) + ay * ay)
        ex = X - ax * w
        ey = Y - ay * w
        t = ex * ax + ey * ay
        b2 = (ex * ex + ey * ey) - (t * t) * inv
        a2 = r2 - b2
        hit = a2 > 0
        wf = (w + t * inv) - np.sqrt(np.where(hit, a2, F(0)) * inv)
        assert wf.dtype == F
        ok = hit & (wf >= F(1))
    return np.where(ok, bits(wf), EMPTY)


def front_buffer(pos, radius, width=800, height=600, brute=False):
    """((height, width) uint32 front words, contributions on a box border)"""
    X, Y, w = CF.camera_space(pos)
    ax, ay = CF.rays(width, height)
    r2 = F(radius) * F(radius)
    front = np.full(width * height, EMPTY, U32)
    n = len(X)
    if brute:
        every, border = np.arange(n), 0
    else:
        px, py, hx, hy, bounded, wide = CF.boxes(pos, width, height, radius)
        every, border = np.nonzero(wide)[0], 0
        idx = np.nonzero(bounded)[0]
        for dy in range(-int(hy[idx].max(initial=0)), int(hy[idx].max(initial=0)) + 1):
            rows = idx[abs(dy) <= hy[idx]]
            for dx in range(-int(hx[rows].max(initial=0)), int(hx[rows].max(initial=0)) + 1):
                i = rows[abs(dx) <= hx[rows]]
                c, r = px[i] + dx, py[i] + dy
                ok = (c >= 0) & (c < width) & (r >= 0) & (r < height)
                i, c, r = i[ok], c[ok], r[ok]
                q = front_words(X[i], Y[i], w[i], ax[c], ay[r], r2)
                np.minimum.at(front, r * width + c, q)
                border += int(((q != EMPTY) & ((abs(dx) == hx[i]) | (abs(dy) == hy[i]))).sum())
    chunk = max(1, (1 << 22) // (width * height))
    front = front.reshape(height, width)
    for k in range(0, len(every), chunk):
        i = every[k:k + chunk]
        q = front_words(X[i, None, None], Y[i, None, None], w[i, None, None], ax[None, None, :], ay[None, :, None], r2)
        front = np.minimum(front, q.min(axis=0))
    return front, border


def shifted(plane, dx, dy, fill):
    """plane[r + dy, c + dx] per pixel (c, r), `fill` where that lies outside"""
    h, w = plane.shape
    out = np.full_like(plane, fill)
    r0, r1 = max(0, -dy), min(h, h - dy)
    c0, c1 = max(0, -dx), min(w, w - dx)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = plane[r0 + dy:r1 + dy, c0 + dx:c1 + dx]
    return out


def smooth_once(zbits, k, delta):
    """one iteration over a (height, width) plane of depth bits (EMPTY = empty): a new plane"""
    delta = F(delta)
    here = zbits != EMPTY
    zp = np.where(here, zbits, U32(0)).view(F)
    num = np.zeros(zbits.shape, F)
    den = np.ones(zbits.shape, F)
    norm = F(2 * k * k + 1)
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            if dx == 0 and dy == 0:
                continue
            qb = shifted(zbits, dx, dy, EMPTY)
            there = here & (qb != EMPTY)
            zq = np.where(there, qb, U32(0)).view(F)
            with np.errstate(all="ignore"):
                d = zq - zp
                u = d / delta
                g = F(1) - u * u
                use = there & (g > 0)
                s = F(1) - F(dx * dx + dy * dy) / norm
                wgt = (s * s) * (g * g)
                num = np.where(use, num + wgt * d, num)
                den = np.where(use, den + wgt, den)
    with np.errstate(all="ignore"):
        out = zp + num / den
    assert out.dtype == F and s.dtype == F
    return np.where(here, bits(out), EMPTY)


def smooth(front, iterations, k, delta):
    z = front
    if k > 0:
        for _ in range(iterations):
            z = smooth_once(z, k, delta)
    return z


def at_least_zero(v):
    return np.where(v > 0, v, F(0))   # (a NaN: 0)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def over_length(a):
    with np.errstate(all="ignore"):
        n = np.sqrt(dot(a, a))
        return [a[0] / n, a[1] / n, a[2] / n]


def tangent(P, ahead, ok_a, behind, ok_b, none):
    with np.errstate(all="ignore"):
        fwd = [ahead[i] - P[i] for i in range(3)]
        back = [P[i] - behind[i] for i in range(3)]
        pick_back = ok_b & (~ok_a | (np.abs(back[2]) < np.abs(fwd[2])))   # (forward on a tie)
    neither = ~ok_a & ~ok_b
    return [np.where(neither, F(none[i]), np.where(pick_back, back[i], fwd[i])) for i in range(3)]


def normals(zbits):
    """(height, width, 3) float32 unit normals of a plane of smoothed depth bits; 0 where the pixel is empty"""
    h, w = zbits.shape
    ax, ay = CF.rays(w, h)
    ax, ay = np.broadcast_to(ax[None, :], (h, w)), np.broadcast_to(ay[:, None], (h, w))

    def points(dx, dy):
        zb = shifted(zbits, dx, dy, EMPTY)
        ok = zb != EMPTY
        z = np.where(ok, zb, U32(0)).view(F)
        a = shifted(ax, dx, dy, F(0))
        b = shifted(ay, dx, dy, F(0))
        with np.errstate(all="ignore"):
            return [a * z, b * z, -z], ok

    P, here = points(0, 0)
    Pe, e = points(1, 0)
    Pw, wk = points(-1, 0)
    Pn, n = points(0, -1)
    Ps, s = points(0, 1)
    Tx = tangent(P, Pe, e, Pw, wk, (1, 0, 0))
    Ty = tangent(P, Pn, n, Ps, s, (0, 1, 0))
    with np.errstate(all="ignore"):
        N = [Tx[1] * Ty[2] - Tx[2] * Ty[1], Tx[2] * Ty[0] - Tx[0] * Ty[2], Tx[0] * Ty[1] - Tx[1] * Ty[0]]
        len2 = dot(N, N)
        good = len2 > 0
        ln = np.sqrt(np.where(good, len2, F(1)))
        N = [np.where(good, N[0] / ln, F(0)), np.where(good, N[1] / ln, F(0)), np.where(good, N[2] / ln, F(1))]
    out = np.stack(N, axis=-1)
    assert out.dtype == F
    out[~here] = 0
    return out


def to_byte(col):
    """(uint32)(min(max(col, 0), 1) 255 + 0.5); a NaN: 0"""
    c = at_least_zero(np.asarray(col, dtype=F))
    c = np.where(c < 1, c, F(1))
    return (c * F(255) + F(0.5)).astype(U32).astype(np.uint8)


def colours(N, col_words, light, s_ref):
    """(height, width, 3) uint8: the water colour of every pixel from its normal and column word"""
    h, w = col_words.shape
    ax, ay = CF.rays(w, h)
    ax, ay = np.broadcast_to(ax[None, :], (h, w)), np.broadcast_to(ay[:, None], (h, w))
    L = over_length([F(light[0]), F(light[1]), F(light[2])])
    n = [N[..., 0], N[..., 1], N[..., 2]]
    with np.errstate(all="ignore"):
        vlen = np.sqrt((F(1) + ax * ax) + ay * ay)
        V = [-ax / vlen, -ay / vlen, F(1) / vlen]
        Hh = over_length([L[0] + V[0], L[1] + V[1], L[2] + V[2]])
        nl = at_least_zero(dot(n, L))
        spec = at_least_zero(dot(n, Hh))
        for _ in range(6):
            spec = spec * spec
        f = F(1) - at_least_zero(dot(n, V))
        fres = F(0.02) + F(0.98) * (((f * f) * (f * f)) * f)
        s_ref = F(s_ref)
        tau = CF.value(col_words) / s_ref if s_ref != 0 else np.zeros((h, w), F)
        lit = F(0.25) + F(0.75) * nl
        out = []
        for kappa, sky in zip(KAPPA, SKY):
            T = F(1) / (F(1) + kappa * tau)
            col = ((F(1) - fres) * (T * lit) + fres * sky) + spec
            assert col.dtype == F
            out.append(to_byte(col))
    return np.stack(out, axis=-1)


def compose(front, zbits, col_words, edge, light, s_ref):
    N = normals(zbits)
    rgb = np.zeros(front.shape + (3,), np.uint8)
    here = front != EMPTY
    rgb[here] = colours(N, col_words, light, s_ref)[here]
    rgb[(edge != EMPTY) & (edge <= front)] = (255, 255, 255)   # (EMPTY is the largest word: an empty pixel is behind)
    return rgb, N


def render_liquid(pos, h, coeff, radius=0.0, smooth_iterations=3, smooth_radius=3, smooth_depth=0.0,
                  light=(0.0, 0.0, 0.0), thickness_scale=0.0, width=800, height=600, brute=False, cache=None):
    """the options of Simulator.render_liquid: smooth_iterations and smooth_radius are counts (0 = none); cache: a dict
    that keeps the two splatted buffers of a (state, radius, size) for the next call"""
    radius = F(radius) if radius else F(h)
    assert 0 < radius <= F(h) and 0 <= smooth_iterations <= 8 and 0 <= smooth_radius <= 7
    delta = F(smooth_depth) if smooth_depth else F(2) * radius
    if not any(light):
        light = DEFAULT_LIGHT
    key = (np.ascontiguousarray(pos, dtype=F).tobytes(), float(radius), float(h), float(coeff), width, height, brute)
    if cache is None or key not in cache:
        splat = front_buffer(pos, radius, width, height, brute) + CF.column_buffer(pos, h, coeff, width, height, brute)
        if cache is not None:
            cache[key] = splat
    else:
        splat = cache[key]
    front, border, column, cborder = splat
    z = smooth(front, smooth_iterations, smooth_radius, delta)
    s_ref = F(thickness_scale) if thickness_scale else CF.value(column.max(initial=0))
    edge = R.edge_buffer(width, height)
    rgb, N = compose(front, z, column, edge, light, s_ref)
    return dict(front=front, smooth=z, normals=N, column=column, rgb=rgb, edge=edge, scale=F(s_ref), border=border + cborder)
