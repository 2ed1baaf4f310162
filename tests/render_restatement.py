"""The visualiser's frame restated in numpy, operation by operation.

Every value is an np.float32 array and every operation is one numpy ufunc call, so each is
rounded on its own like the strict-fp32 device code.  Shares no code with the HIP side."""
import numpy as np

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)

BOX_VERTICES = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0],
                         [0, 0, 10], [10, 0, 10], [10, 10, 10], [0, 10, 10]], dtype=F)
BOX_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
EDGE_SAMPLES = 4096


def project(pos, width, height):
    """pixel column, pixel row (row 0 = top of the window) and depth bits of each point"""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    W, H = F(width), F(height)
    w = F(15) - z
    xw = (((F(0.5) * (x - F(5))) / w) + F(1)) * (F(0.5) * W)
    yw = (((F(0.5) * (y - F(5))) / w) + F(1)) * (F(0.5) * H)
    assert xw.dtype == F and yw.dtype == F and w.dtype == F
    px = np.floor(xw).astype(np.int64)
    py = (height - 1) - np.floor(yw).astype(np.int64)
    return px, py, np.ascontiguousarray(w).view(np.uint32)


def splat(pos, word, empty, dtype, width, height, point_size):
    """(minimum, count): per pixel the minimum of word(depth bits) over the particles whose square covers it
    (`empty` where none does) as a (height, width) `dtype` array, and how many do as a uint32 one"""
    least = np.full(width * height, empty, dtype)
    count = np.zeros(width * height, np.uint32)
    px, py, wb = project(pos, width, height)
    w = word(wb)
    r = (point_size - 1) // 2
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = px + dx, py + dy
            ok = (x >= 0) & (x < width) & (y >= 0) & (y < height)
            idx = y[ok] * width + x[ok]
            np.minimum.at(least, idx, w[ok])
            np.add.at(count, idx, np.uint32(1))
    return least.reshape(height, width), count.reshape(height, width)


def particle_buffers(pos, width=800, height=600, point_size=3):
    """(depth bits, count): two (height, width) uint32 arrays"""
    return splat(pos, lambda wb: wb, EMPTY, np.uint32, width, height, point_size)


def edge_points():
    """the 12 x 4096 sample points of the box edges"""
    t = np.arange(EDGE_SAMPLES, dtype=F) / F(EDGE_SAMPLES - 1)
    pts = []
    for ia, ib in BOX_EDGES:
        a, b = BOX_VERTICES[ia], BOX_VERTICES[ib]
        pts.append(np.stack([a[c] + t * (b[c] - a[c]) for c in range(3)], axis=1).astype(F))
    return np.concatenate(pts)


def edge_buffer(width=800, height=600):
    edge = np.full(width * height, EMPTY, np.uint32)
    px, py, wb = project(edge_points(), width, height)
    ok = (px >= 0) & (px < width) & (py >= 0) & (py < height)
    np.minimum.at(edge, py[ok] * width + px[ok], wb[ok])
    return edge.reshape(height, width)


def compose(depth, count, edge, shade="flat"):
    """(height, width, 3) uint8"""
    h, w = depth.shape
    rgb = np.zeros((h, w, 3), np.uint8)
    hit = count > 0
    if shade == "flat":
        rgb[hit] = (0, 0, 255)
    else:
        c = count[hit].astype(np.int64)
        level = np.zeros_like(c)
        for k in range(1, 8):  # floor(log2(c)) capped at 7, integers only
            level += (c >= (1 << k))
        col = np.stack([32 * level, 32 * level, np.full_like(level, 255)], axis=1)
        rgb[hit] = col.astype(np.uint8)
    white = (edge != EMPTY) & (edge <= depth)
    rgb[white] = (255, 255, 255)
    return rgb


def render(pos, width=800, height=600, point_size=3, shade="flat"):
    depth, count = particle_buffers(pos, width, height, point_size)
    edge = edge_buffer(width, height)
    return dict(depth=depth, count=count, edge=edge, rgb=compose(depth, count, edge, shade))
