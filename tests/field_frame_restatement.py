"""The field frame ("The field frame") restated in numpy, operation by operation.

Every value is an np.float32 array and every operation one numpy ufunc call, so each is rounded on its
own like the strict-fp32 device code.  Shares no code with the HIP side; the projection and the box-edge
layer are those of render_restatement.py (the flat frame's restatement)."""
import numpy as np

import render_restatement as R

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
EMPTY64 = np.uint64(0xFFFFFFFFFFFFFFFF)
GAS_CONSTANT = F(1)
REST_DENSITY = F(1000)
FIELDS = ("speed", "density", "pressure")


def scalar(vel, rho, field):
    """the per-particle scalar s (float32) from the velocities and densities sph_download_state returns"""
    vel = np.ascontiguousarray(vel, dtype=F).reshape(-1, 3)
    rho = np.ascontiguousarray(rho, dtype=F).reshape(-1)
    if field == "speed":
        vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
        s = np.sqrt((vx * vx + vy * vy) + vz * vz)
    elif field == "density":
        s = rho.copy()
    elif field == "pressure":
        s = np.maximum(F(0), GAS_CONSTANT * (rho - REST_DENSITY))
    else:
        raise ValueError(field)
    assert s.dtype == F
    # s >= +0 and no NaN: the order of the bit patterns is the order of the values
    assert (s.view(np.uint32) <= np.uint32(0x7F800000)).all(), "the field frame is defined for s >= +0 only"
    return s


def packed_buffers(pos, s, width=800, height=600, point_size=3):
    """(packed, count): per pixel the minimum of (bits(w) << 32) | bits(s) as uint64, and the hit count"""
    sb = np.ascontiguousarray(s, dtype=F).view(np.uint32).astype(np.uint64)
    return R.splat(pos, lambda wb: (wb.astype(np.uint64) << np.uint64(32)) | sb, EMPTY64, np.uint64, width, height, point_size)


def split(packed):
    """(depth bits, value bits) of a packed buffer: two uint32 arrays"""
    return (packed >> np.uint64(32)).astype(np.uint32), (packed & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def quantise(s, lo, hi):
    """q = (int)fminf(fmaxf(floorf(((s - lo) / (hi - lo)) * 256), 0), 255); 0 where hi == lo or the quotient is NaN"""
    s = np.asarray(s, dtype=F)
    lo, hi = F(lo), F(hi)
    if hi == lo:
        return np.zeros(s.shape, np.int64)
    with np.errstate(all="ignore"):
        u = ((s - lo) / (hi - lo)) * F(256)
        assert u.dtype == F
        q = np.minimum(np.maximum(np.floor(u), F(0)), F(255))
    return np.where(np.isnan(u), F(0), q).astype(np.int64)


def ramp(q):
    """(..., 3) uint8 colours of the integer ramp blue - cyan - green - yellow - red"""
    q = np.asarray(q, dtype=np.int64)
    r = np.select([q < 128, q < 192], [0, 4 * (q - 128)], 255)
    g = np.select([q < 64, q < 192], [4 * q, 255], 255 - 4 * (q - 192))
    b = np.select([q < 64, q < 128], [255, 255 - 4 * (q - 64)], 0)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def compose(packed, count, edge, lo, hi):
    """(height, width, 3) uint8"""
    depth, value = split(packed)
    h, w = depth.shape
    rgb = np.zeros((h, w, 3), np.uint8)
    hit = count > 0
    rgb[hit] = ramp(quantise(value[hit].view(F), lo, hi))
    white = (edge != EMPTY) & (edge <= depth)
    rgb[white] = (255, 255, 255)
    return rgb


def render_field(pos, vel, rho, field="speed", lo=0.0, hi=0.0, width=800, height=600, point_size=3):
    s = scalar(vel, rho, field)
    lo, hi = F(lo), F(hi)
    assert np.isfinite(lo) and np.isfinite(hi) and not hi < lo
    if lo == 0 and hi == 0 and len(s):  # automatic: over all particles, visible or not
        lo, hi = s.min(), s.max()
    packed, count = packed_buffers(pos, s, width, height, point_size)
    edge = R.edge_buffer(width, height)
    depth, value = split(packed)
    return dict(depth=depth, count=count, edge=edge, value=value, range=(F(lo), F(hi)),
                rgb=compose(packed, count, edge, lo, hi))
