"""Ray casting and the view frame restated in numpy, operation by operation.

Every value of the definition is an np.float32 array and every operation one numpy ufunc call, so each is rounded
on its own like the strict-fp32 device code.  Shares no code with the HIP side; the quantiser, the ramp and the
scalar of a particle are the field frame's (field_frame_restatement.py), the byte conversion the liquid frame's.

The hit words come in two forms.  `brute` tests every particle against every ray, as the definition reads.  `walk`
is the layer walk of the design: per ray the layers of cells along its dominant axis, per layer the cells of a
rectangle; its geometry is evaluated in float64 with the padded radius R = r + pad, and it reports how many
contributions lay in cells that only the padding brought in (none may: a miss would hide behind the bound)."""
import numpy as np

import field_frame_restatement as FF
import liquid_frame_restatement as LF

F = np.float32
U32 = np.uint32
U64 = np.uint64
MISS = U64(0xFFFFFFFFFFFFFFFF)
DEFAULT_LIGHT = (-0.35, 0.8, 0.5)
FLAT = (F(0.1), F(0.35), F(0.9))
DEFAULT_TAN_Y = F(0.41421357)
DD_LO, DD_HI = F(2.0 ** -40), F(2.0 ** 40)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U32)


def make_rays(origins, directions, t_min=0.0, t_max=np.inf):
    """(m, 8) float32: ox oy oz t_min dx dy dz t_max, the layout of SphRay"""
    o = np.asarray(origins, dtype=F).reshape(-1, 3)
    rays = np.zeros((len(o), 8), F)
    rays[:, 0:3] = o
    rays[:, 4:7] = np.asarray(directions, dtype=F).reshape(-1, 3)
    rays[:, 3] = t_min
    rays[:, 7] = t_max
    return rays


def visible(pos, h, D):
    """each coordinate passes point_cell: p >= 0 and p / h < D"""
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = pos / F(h)
    assert q.dtype == F
    return ((pos >= 0) & (q < F(D))).all(axis=1)


def dd_of(rays):
    dx, dy, dz = rays[:, 4], rays[:, 5], rays[:, 6]
    with np.errstate(all="ignore"):
        dd = (dx * dx + dy * dy) + dz * dz
    assert dd.dtype == F
    return dd


def valid(rays, h, D):
    with np.errstate(all="ignore"):
        reach = F(64) * (F(D) * F(h))
        dd = dd_of(rays)
        ok = np.isfinite(rays[:, 0:3]).all(axis=1) & np.isfinite(rays[:, 4:7]).all(axis=1)
        ok &= (rays[:, 3] >= 0) & (rays[:, 3] <= rays[:, 7])
        ok &= (dd >= DD_LO) & (dd <= DD_HI)
        ok &= (np.abs(rays[:, 0:3]) <= reach).all(axis=1)
    return ok


def pair_words(o, d, tmin, tmax, dd, p, ids, vis, r2):
    """the word of every pair; o, d, p: three arrays each, everything broadcast against everything"""
    with np.errstate(all="ignore"):
        ex, ey, ez = p[0] - o[0], p[1] - o[1], p[2] - o[2]
        b = (ex * d[0] + ey * d[1]) + ez * d[2]
        tc = b / dd
        fx, fy, fz = ex - tc * d[0], ey - tc * d[1], ez - tc * d[2]
        b2 = (fx * fx + fy * fy) + fz * fz
        a2 = r2 - b2
        hit = vis & (a2 > 0)
        t = tc - np.sqrt(np.where(hit, a2, F(0)) / dd)
        ok = hit & (t >= tmin) & (t <= tmax)
        t = np.where(t == 0, F(0), t)   # -0 is stored as +0
    assert t.dtype == F and b2.dtype == F
    w = (bits(t).reshape(t.shape).astype(U64) << U64(32)) | ids
    return np.where(ok, w, MISS)


def radius_of(radius, h):
    r = F(radius) if radius else F(0.5) * F(h)
    assert 0 < r <= F(h)
    return r


def brute(pos, rays, h, D, radius=0.0, chunk=1 << 22):
    """(m,) uint64: the minimum over all pairs, as the definition reads"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 8)
    r = radius_of(radius, h)
    r2 = r * r
    vis = visible(pos, h, D)
    ids = np.arange(len(pos), dtype=U64)
    ok = valid(rays, h, D)
    dd = dd_of(rays)
    out = np.full(len(rays), MISS, U64)
    if not len(pos):
        return out
    step = max(1, chunk // len(pos))
    p = [pos[None, :, a] for a in range(3)]
    for k in range(0, len(rays), step):
        q = rays[k:k + step]
        w = pair_words([q[:, a, None] for a in range(3)], [q[:, 4 + a, None] for a in range(3)], q[:, 3, None], q[:, 7, None],
                       dd[k:k + step, None], p, ids[None, :], vis[None, :], r2)
        out[k:k + step] = np.where(ok[k:k + step], w.min(axis=1), MISS)
    return out


def pad_of(rays, h, D):
    """float64: h / 16 + 2^-17 (max |o_a| + D h) per ray (section 10n: the bound on the fp32 error of b2, t and the
    walk's own arithmetic, and a sixteenth of a cell on top)"""
    hf = float(F(h))
    return hf / 16 + 2.0 ** -17 * (np.abs(rays[:, 0:3].astype(np.float64)).max(axis=1) + D * hf)


def cell_table(pos, h, D):
    """the visible particles sorted by flattened cell: (order, start per cell [D^3 + 1])"""
    vis = np.flatnonzero(visible(pos, h, D))
    with np.errstate(all="ignore"):
        c = (pos[vis] / F(h)).astype(np.int64)
    key = c[:, 0] + D * (c[:, 1] + D * c[:, 2])
    order = vis[np.argsort(key, kind="stable")]
    start = np.searchsorted(np.sort(key), np.arange(D ** 3 + 1))
    return order, start


def walk(pos, rays, h, D, radius=0.0):
    """-> (m,) uint64 words, contributions in the padding, candidate tests, layers looked into"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 8)
    m = len(rays)
    r = radius_of(radius, h)
    r2 = r * r
    out = np.full(m, MISS, U64)
    order, start = cell_table(pos, h, D)
    if not len(order):
        return out, 0, 0, 0
    hf = float(F(h))
    dd = dd_of(rays)
    live = np.flatnonzero(valid(rays, h, D))
    R64 = float(r) + pad_of(rays, h, D)
    o64, d64 = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    tmin64, tmax64 = rays[:, 3].astype(np.float64), rays[:, 7].astype(np.float64)
    ax_m = np.argmax(np.abs(d64), axis=1)
    others = np.array([[1, 2], [0, 2], [0, 1]])
    padding = tests = layers = 0
    for i in range(D):
        if not len(live):
            break
        q = live
        am = ax_m[q]
        om, dm = o64[q, am], d64[q, am]
        k = np.where(dm > 0, i, D - 1 - i)
        with np.errstate(all="ignore"):
            span = {}
            for name, R in (("pad", R64[q]), ("bare", np.full(len(q), float(r)))):
                ta, tb = (k * hf - R - om) / dm, ((k + 1) * hf + R - om) / dm
                tin, tout = np.minimum(ta, tb), np.maximum(ta, tb)
                ts, te = np.maximum(tin, tmin64[q]), np.minimum(tout, tmax64[q])
                lo, hi = [], []
                for j in range(2):
                    a = others[am, j]
                    ca, cb = o64[q, a] + ts * d64[q, a], o64[q, a] + te * d64[q, a]
                    lo.append(np.floor((np.minimum(ca, cb) - R) / hf))
                    hi.append(np.floor((np.maximum(ca, cb) + R) / hf))
                span[name] = (tin, ts <= te, lo, hi)
        tin, some, lo, hi = span["pad"]
        best_t = (out[q] >> U64(32)).astype(U32).view(F).astype(np.float64)
        done = (out[q] != MISS) & (best_t < tin)   # the ray enters the widened layer behind its best entry: it stops
        live = q[~done]
        use = some & ~done & (hi[0] >= 0) & (lo[0] <= D - 1) & (hi[1] >= 0) & (lo[1] <= D - 1)
        if not use.any():
            continue
        layers += int(use.sum())
        q, am, k = q[use], am[use], k[use]
        lo = [np.clip(a[use], 0, D - 1).astype(np.int64) for a in lo]
        hi = [np.clip(a[use], 0, D - 1).astype(np.int64) for a in hi]
        _, bsome, blo, bhi = span["bare"]
        bsome, blo, bhi = bsome[use], [a[use] for a in blo], [a[use] for a in bhi]
        for du in range(int((hi[0] - lo[0]).max()) + 1):
            for dv in range(int((hi[1] - lo[1]).max()) + 1):
                cu, cv = lo[0] + du, lo[1] + dv
                sel = (cu <= hi[0]) & (cv <= hi[1])
                if not sel.any():
                    continue
                c3 = np.zeros((int(sel.sum()), 3), np.int64)
                idx = np.arange(len(c3))
                c3[idx, am[sel]] = k[sel]
                c3[idx, others[am[sel], 0]] = cu[sel]
                c3[idx, others[am[sel], 1]] = cv[sel]
                cell = c3[:, 0] + D * (c3[:, 1] + D * c3[:, 2])
                cnt = start[cell + 1] - start[cell]
                if not cnt.sum():
                    continue
                ray = np.repeat(q[sel], cnt)
                inner = np.repeat(bsome[sel] & (cu[sel] >= blo[0][sel]) & (cu[sel] <= bhi[0][sel]) & (cv[sel] >= blo[1][sel]) & (cv[sel] <= bhi[1][sel]), cnt)
                part = order[np.repeat(start[cell], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
                w = pair_words([rays[ray, a] for a in range(3)], [rays[ray, 4 + a] for a in range(3)], rays[ray, 3], rays[ray, 7], dd[ray],
                               [pos[part, a] for a in range(3)], part.astype(U64), True, r2)
                tests += len(w)
                padding += int(((w != MISS) & ~inner).sum())
                np.minimum.at(out, ray, w)
    return out, padding, tests, layers


def split(words):
    """(t as float32 with inf for a miss, ids as int64 with -1 for a miss)"""
    words = np.asarray(words, dtype=U64)
    miss = words == MISS
    t = (words >> U64(32)).astype(U32).view(F)
    return np.where(miss, F(np.inf), t), np.where(miss, -1, (words & U64(0xFFFFFFFF)).astype(np.int64))


# ---- the view camera ----

def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def basis(eye, target, up):
    """(fwd, s, u), three float32 each; None where g or s0 vanishes or is not finite"""
    eye, target, up = ([F(v) for v in x] for x in (eye, target, up))
    with np.errstate(all="ignore"):
        g = [target[a] - eye[a] for a in range(3)]
        gg = dot(g, g)
        if not (np.isfinite(gg) and gg > 0):
            return None
        glen = np.sqrt(gg)
        fwd = [g[a] / glen for a in range(3)]
        s0 = cross(fwd, up)
        ss = dot(s0, s0)
        if not (np.isfinite(ss) and ss > 0):
            return None
        slen = np.sqrt(ss)
        s = [s0[a] / slen for a in range(3)]
        u = cross(s, fwd)
    assert all(type(v) is F for v in fwd + s + u)
    return fwd, s, u


def camera(eye, target, up=(0.0, 1.0, 0.0), width=800, height=600, tan_half=(0.0, 0.0), near=0.0, far=0.0, h=0.1):
    """the options with every default resolved"""
    width, height = width or 800, height or 600
    tx, ty = F(tan_half[0]), F(tan_half[1])
    if tx == 0 and ty == 0:
        ty = DEFAULT_TAN_Y
        tx = ty * (F(width) / F(height))
    b = basis(eye, target, up)
    assert b is not None
    return dict(eye=[F(v) for v in eye], fwd=b[0], s=b[1], u=b[2], tan=(tx, ty), near=F(near) if near else F(h),
                far=F(far) if far else F(np.inf), width=width, height=height)


def view_rays(cam):
    """(width x height, 8) float32: the pixel-centre rays, row 0 first"""
    W, H = cam["width"], cam["height"]
    c = np.arange(W).astype(F)
    r = (H - 1 - np.arange(H)).astype(F)
    ax = cam["tan"][0] * (((c + F(0.5)) / (F(0.5) * F(W))) - F(1))
    ay = cam["tan"][1] * (((r + F(0.5)) / (F(0.5) * F(H))) - F(1))
    ax, ay = np.broadcast_to(ax[None, :], (H, W)), np.broadcast_to(ay[:, None], (H, W))
    rays = np.zeros((H, W, 8), F)
    for a in range(3):
        rays[..., a] = cam["eye"][a]
        d = (cam["fwd"][a] + ax * cam["s"][a]) + ay * cam["u"][a]
        assert d.dtype == F
        rays[..., 4 + a] = d
    rays[..., 3] = cam["near"]
    rays[..., 7] = cam["far"]
    return rays.reshape(-1, 8)


# ---- the picture ----

def edge_entries(rays, box, rho):
    """(m,) float32: the smallest entry into one of the twelve edge cylinders inside the ray's window, inf where none"""
    box, rho = F(box), F(rho)
    rho2 = rho * rho
    least = np.full(len(rays), F(np.inf), F)
    o, d = rays[:, 0:3], rays[:, 4:7]
    with np.errstate(all="ignore"):
        for a, (b, c) in enumerate(((1, 2), (0, 2), (0, 1))):
            dd2 = d[:, b] * d[:, b] + d[:, c] * d[:, c]
            for cb in (F(0), box):
                for cc in (F(0), box):
                    eb, ec = cb - o[:, b], cc - o[:, c]
                    tc = (eb * d[:, b] + ec * d[:, c]) / dd2
                    fb, fc = eb - tc * d[:, b], ec - tc * d[:, c]
                    a2 = rho2 - (fb * fb + fc * fc)
                    hit = (dd2 > 0) & (a2 > 0)
                    te = tc - np.sqrt(np.where(hit, a2, F(0)) / dd2)
                    along = o[:, a] + te * d[:, a]
                    ok = hit & (te >= rays[:, 3]) & (te <= rays[:, 7]) & (along >= 0) & (along <= box)
                    assert te.dtype == F and along.dtype == F
                    least = np.where(ok & (te < least), te, least)
    return least


def shade_pixels(words, rays, cam, pos, vel, rho, shade="flat", lo=0.0, hi=0.0, light=(0.0, 0.0, 0.0)):
    """(m, 3) uint8: the colour of every ray's hit (black for a miss), edges not drawn"""
    t, ids = split(words)
    hit = ids >= 0
    i = np.where(hit, ids, 0)
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    rgb = np.zeros((len(rays), 3), np.uint8)
    if not len(pos) or not hit.any():
        return rgb
    if not any(light):
        light = DEFAULT_LIGHT
    L = LF.over_length([F(light[0]), F(light[1]), F(light[2])])
    with np.errstate(all="ignore"):
        tt = np.where(hit, t, F(0))
        n0 = [(rays[:, a] + tt * rays[:, 4 + a]) - pos[i, a] for a in range(3)]
        len2 = dot(n0, n0)
        good = len2 > 0
        ln = np.sqrt(np.where(good, len2, F(1)))
        N = [np.where(good, n0[a] / ln, -cam["fwd"][a]) for a in range(3)]
        nl0 = dot(N, L)
        nl = np.where(nl0 > 0, nl0, F(0))
        lit = F(0.25) + F(0.75) * nl
        if shade == "flat":
            base = [np.full(len(rays), c, F) for c in FLAT]
        else:
            s = FF.scalar(vel, rho, shade)
            lo, hi = F(lo), F(hi)
            if lo == 0 and hi == 0:
                lo, hi = s.min(), s.max()
            ramp = FF.ramp(FF.quantise(s[i], lo, hi))
            base = [ramp[:, ch].astype(F) / F(255) for ch in range(3)]
        for ch in range(3):
            col = base[ch] * lit
            assert col.dtype == F
            rgb[:, ch] = LF.to_byte(col)
    rgb[~hit] = 0
    return rgb


def render_view(pos, vel, rho, h, D, cam, radius=0.0, shade="flat", lo=0.0, hi=0.0, light=(0.0, 0.0, 0.0), edge_radius=0.0,
                box=None, words=None):
    """dict(words (H, W) uint64, rgb (H, W, 3) uint8); words: those of the rays, where already known"""
    rays = view_rays(cam)
    box = F(box) if box is not None else F(h) * F(D)
    if words is None:
        words, padding, _, _ = walk(pos, rays, h, D, radius)
        assert padding == 0, "a contribution in the padding of the restatement's walk"
    words = np.asarray(words, dtype=U64).reshape(-1)
    rgb = shade_pixels(words, rays, cam, pos, vel, rho, shade, lo, hi, light)
    if not edge_radius < 0:
        rho_e = F(edge_radius) if edge_radius else F(0.002) * box
        te = edge_entries(rays, box, rho_e)
        t, ids = split(words)
        rgb[np.isfinite(te) & ((ids < 0) | (te <= t))] = (255, 255, 255)
    H, W = cam["height"], cam["width"]
    return dict(words=words.reshape(H, W), rgb=rgb.reshape(H, W, 3))
