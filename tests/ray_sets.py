"""What tests/test_ray_cast_cpu.py (restatements, without a GPU) and tests/test_gpu_ray_cast.py (the kernels) share: the
cameras and the ray sets the ray cast is held to, the smallest that can go wrong.  Imports nothing from the product.
Cameras are given for the reference's box of 10 and scaled to the box of the state."""
import numpy as np

import ray_cast_restatement as RC

F = np.float32
SIZES = [(64, 48), (5, 3), (1, 1)]
REFERENCE = dict(eye=(5.0, 5.0, 15.0), target=(5.0, 5.0, 0.0), up=(0.0, 1.0, 0.0), tan_half=(2.0, 2.0))   # the frames' camera
OBLIQUE = dict(eye=(-4.0, 13.0, 9.0), target=(5.0, 5.0, 5.0), up=(0.0, 1.0, 0.0), tan_half=(0.0, 0.0))
BATCHES = (1, 63, 64, 65)   # below, at and above one wave


def scaled(cam, box, **more):
    """the camera for a box of `box` instead of 10"""
    k = float(box) / 10.0
    out = dict(cam, eye=tuple(k * v for v in cam["eye"]), target=tuple(k * v for v in cam["target"]))
    out.update(more)
    return out


def inside_eye(pos, box):
    """a camera at the component-wise median of the particles (no particles: the middle of the box), looking along
    (1, 0.3, -0.5)"""
    pos = np.zeros((0, 3)) if pos is None else np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    eye = tuple(float(v) for v in (np.median(pos, axis=0) if len(pos) else np.full(3, float(box) / 2)))
    k = float(box) / 10.0
    return dict(eye=eye, target=(eye[0] + k, eye[1] + 0.3 * k, eye[2] - 0.5 * k), up=(0.0, 1.0, 0.0), tan_half=(0.0, 0.0))


def cameras(pos, box):
    return {"reference": scaled(REFERENCE, box), "oblique": scaled(OBLIQUE, box), "inside": inside_eye(pos, box)}


def camera_rays(cam, width, height, h, near=0.0, far=0.0):
    return RC.view_rays(RC.camera(cam["eye"], cam["target"], cam["up"], width, height, cam["tan_half"], near, far, h))


def random_rays(count, box, seed):
    """origins in and around the box, directions anywhere, lengths over three decades"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.3 * box, 1.3 * box, (count, 3))
    d = rng.normal(size=(count, 3)) * 10.0 ** rng.uniform(-1.5, 1.5, (count, 1))
    return RC.make_rays(o, d)


def axis_rays(h, D, box, through=None):
    """axis-parallel rays of both signs on every axis: origins on cell-face planes (k h exactly, in fp32), along the
    box's edges, through cell centres and through the point `through` (a particle: the rays meet its centre); and the
    four body diagonals through the corners, both ways"""
    hf, box = F(h), float(box)
    ks = sorted({0, 1, D // 2, D - 1, D})
    o, d = [], []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for sign in (1.0, -1.0):
            start = -0.25 * box if sign > 0 else 1.25 * box
            for kb in ks:
                for kc in ks:
                    p = np.zeros(3)
                    p[a], p[b], p[c] = start, float(F(kb) * hf), float(F(kc) * hf)   # in face planes; kb, kc in {0, D}: along an edge
                    o.append(p)
                    d.append(np.eye(3)[a] * sign)
            for centre in [np.full(3, (D // 2 + 0.5) * float(hf))] + ([np.array(through, np.float64)] if through is not None else []):
                p = centre.copy()
                p[a] = start
                o.append(p)
                d.append(np.eye(3)[a] * sign)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                dirn = np.array([sx, sy, sz])
                o.append(np.where(dirn > 0, -0.25 * box, 1.25 * box))
                d.append(dirn)
    return RC.make_rays(np.array(o), np.array(d))


def stray_rays(box):
    """rays that miss the box, point away from it, or start beyond it"""
    box = float(box)
    o = [(-box, 0.5 * box, 0.5 * box), (0.5 * box, 0.5 * box, 2 * box), (0.5 * box, 3 * box, 0.5 * box), (-0.1 * box, -0.1 * box, 0.5 * box),
         (2 * box, 2 * box, 2 * box)]
    d = [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (-1.0, -1.0, 0.0), (1.0, 1.0, 0.5)]
    return RC.make_rays(np.array(o), np.array(d))


def invalid_rays(box):
    """each misses: a NaN origin, a NaN direction, an infinite direction, a zero d, dd beyond 2^-40 and 2^40, an origin
    beyond 64 boxes, t_min > t_max, a negative t_min, a NaN t_max"""
    box = float(box)
    mid = (0.5 * box,) * 3
    rows = [((np.nan, mid[1], mid[2]), (0, 0, -1), 0, np.inf), (mid, (0, np.nan, -1), 0, np.inf), (mid, (np.inf, 0, 0), 0, np.inf),
            (mid, (0, 0, 0), 0, np.inf), (mid, (0, 0, -2.0 ** -21), 0, np.inf), (mid, (0, 2.0 ** 21, 0), 0, np.inf),
            ((mid[0], mid[1], 65 * box), (0, 0, -1), 0, np.inf), (mid, (0, 0, -1), 2.0, 1.0), (mid, (0, 0, -1), -1.0, np.inf),
            (mid, (0, 0, -1), 0, np.nan)]
    return np.concatenate([RC.make_rays([o], [d], tmin, tmax) for o, d, tmin, tmax in rows])


def boundary_rays(through, h, D):
    """valid rays at the ends of what is valid, each through the point `through` (a particle: they hit it): dd = 2^-40,
    dd = 2^40, and an origin 64 boxes out on an axis (|o_a| = 64 (D h), formed in fp32)"""
    x, y, z = (float(v) for v in through)
    far = float(F(64) * (F(D) * F(h)))
    box = float(F(D) * F(h))
    return RC.make_rays([(x, y, z + 0.25 * box), (x, y - 0.25 * box, z), (x, y, far)], [(0, 0, -2.0 ** -20), (0, 2.0 ** 20, 0), (0, 0, -1)])


def ray_sets(pos, h, D, box, sizes=SIZES):
    """name -> (m, 8) float32 rays"""
    out = {}
    for name, cam in cameras(pos, box).items():
        for (w, hh) in (sizes if name != "inside" else sizes[:1]):
            out[f"{name} {w}x{hh}"] = camera_rays(cam, w, hh, h)
    for count in BATCHES:
        out[f"random {count}"] = random_rays(count, float(box), 100 + count)
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    middle = pos[np.argmin(np.abs(pos.astype(np.float64) - np.median(pos, axis=0)).sum(axis=1))] if len(pos) else None
    out["axis"] = axis_rays(h, D, box, middle)
    if middle is not None:
        out["boundary"] = boundary_rays(middle, h, D)
    out["stray"] = stray_rays(box)
    out["invalid"] = invalid_rays(box)
    return out
