"""Python mirror of the reference's `Simulator` (src/simulator.h:53-74).

Same method names and semantics -- setup(), simulate(), simulateAndTime(times),
getPosition(), moveParticles((x, y)) -- over the C-ABI of libsph_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (SphError, SphKernelTimes, SphOptions, SphSettings, SphTimes,
                   load_library)


class Times(SphTimes):
    """times.h:5-10.  display() prints the reference's table (times.h:12-35)."""

    def display(self):
        it = self.iters
        rows = [("%-12s%18s%12s" % ("Operation", "Per frame", "Total")), "-" * 45]
        g = self.buildGrid / it if it else 0.0
        s = self.sphUpdate / it if it else 0.0
        m = self.memcpy / it if it else 0.0
        rows.append("%-11s%11.5f%15.5f" % ("Grid construction", g, self.buildGrid))
        rows.append("%-12s%16.5f%15.5f" % ("SPH update", s, self.sphUpdate))
        rows.append("%-12s%15.5f%15.5f" % ("Data transfer", m, self.memcpy))
        return "\n".join(rows)


Settings = SphSettings


def default_settings(num_particles, random_init):
    """The constants main() derives (main.cpp:57-63)."""
    s = SphSettings()
    rc = load_library().sph_default_settings(C.byref(s), int(num_particles),
                                             1 if random_init else 0)
    if rc:
        raise SphError("sph_default_settings failed")
    return s


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _lattice(o, shape, origin, spacing):
    """struct_size, nx / ny / nz, origin and spacing of a lattice struct (SphSampleLattice, SphSurfaceOptions) from
    `shape` = (nz, ny, nx), origin as (x, y, z) and spacing as (x, y, z) or one number; returns (nz, ny, nx) as ints."""
    nz, ny, nx = (int(d) for d in shape)
    o.struct_size = C.sizeof(type(o))
    o.nx, o.ny, o.nz = nx, ny, nz
    o.origin[:] = [float(v) for v in origin]
    o.spacing[:] = [float(v) for v in (spacing if np.ndim(spacing) else (spacing,) * 3)]
    return nz, ny, nx


def _rows(p, n, cols, dtype):
    """An array of its own of the n x cols values behind the C pointer p (cols = None: n values); n == 0 (p may be
    null): the empty array of that shape."""
    shape = (n,) if cols is None else (n, cols)
    return np.array(np.ctypeslib.as_array(p, shape=shape), copy=True) if n else np.zeros(shape, dtype)


class Simulator:
    def __init__(self, settings, sweep="list", flags=0, device=-1, capacity=0, math="strict", key_order="flattened"):
        self.settings = settings
        self._L = load_library()
        self._h = C.c_void_p()
        self._opt = SphOptions()
        self._opt.struct_size = C.sizeof(SphOptions)
        self._opt.device = device
        self._opt.math_mode = _lib.SPH_MATH_FAST if math == "fast" else _lib.SPH_MATH_STRICT
        self._opt.sweep = _lib.SWEEPS[sweep]
        self._opt.flags = flags
        self._opt.capacity = capacity
        self._opt.key_order = 1 if key_order == "morton" else 0
        rc = self._L.sph_create(C.byref(settings), C.byref(self._opt), C.byref(self._h))
        if rc:
            msg = self._L.sph_last_error(None).decode()
            self._h = C.c_void_p()
            raise SphError(f"sph_create failed ({rc}): {msg}")
        self.mouseClicked = False
        self.clickCoords = (0, 0)

    # -- plumbing --
    def _check(self, rc, what):
        if rc:
            raise SphError(f"{what} failed ({rc}): {self._L.sph_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.sph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n(self):
        return self.settings.numParticles

    # -- the reference's methods --
    def setup(self):
        self._check(self._L.sph_setup(self._h), "sph_setup")

    def simulate(self):
        self._check(self._L.sph_step(self._h, None), "sph_step")
        if self.mouseClicked:  # simulator.cu:482-489
            self.moveParticles(self.clickCoords)
            self.mouseClicked = False

    def simulateAndTime(self, times):
        self._check(self._L.sph_step(self._h, C.byref(times)), "sph_step")

    def moveParticles(self, mouse_pos):
        self._check(self._L.sph_apply_click(self._h, int(mouse_pos[0]), int(mouse_pos[1])),
                    "sph_apply_click")

    def getPosition(self):
        """(n, 3) float32 view of the handle's host buffer, original-id order,
        valid until the next step (simulator.cu:407-409)."""
        p = self._L.sph_positions_host(self._h)
        if not p:
            raise SphError("sph_positions_host failed")
        if self.n == 0:
            return np.zeros((0, 3), np.float32)
        return np.ctypeslib.as_array(p, shape=(self.n, 3))

    # -- extras (tests, bench) --
    def upload_state(self, pos, vel=None):
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        if vel is not None:
            vel = np.ascontiguousarray(vel, dtype=np.float32)
        self._check(self._L.sph_upload_state(self._h, _fp(pos), _fp(vel), len(pos)),
                    "sph_upload_state")

    def download_state(self):
        n = self.n
        pos = np.zeros((n, 3), np.float32)
        vel = np.zeros((n, 3), np.float32)
        rho = np.zeros(n, np.float32)
        prs = np.zeros(n, np.float32)
        self._check(self._L.sph_download_state(self._h, _fp(pos), _fp(vel), _fp(rho),
                                               _fp(prs)), "sph_download_state")
        return dict(pos=pos, vel=vel, rho=rho, prs=prs)

    def download_force(self):
        f = np.zeros((self.n, 3), np.float32)
        self._check(self._L.sph_download_force(self._h, _fp(f)), "sph_download_force")
        return f

    def download_grid(self):
        n = self.n
        ids = np.zeros(n, np.uint32)
        keys = np.zeros(n, np.uint32)
        cells = np.zeros((self._L.sph_num_table_cells(self._h), 2), np.int32)
        self._check(self._L.sph_download_grid(
            self._h, ids.ctypes.data_as(C.POINTER(C.c_uint32)),
            keys.ctypes.data_as(C.POINTER(C.c_uint32)),
            cells.ctypes.data_as(C.POINTER(C.c_int32))), "sph_download_grid")
        return dict(ids=ids, keys=keys, cells=cells)

    def debug_counters(self):
        out = (C.c_uint64 * 16)()
        self._check(self._L.sph_debug_counters(self._h, out), "sph_debug_counters")
        return list(out)

    def save_state(self, path):
        self._check(self._L.sph_save_state(self._h, str(path).encode()), "sph_save_state")

    def load_state(self, path):
        self._check(self._L.sph_load_state(self._h, str(path).encode()), "sph_load_state")

    # -- the visualiser's frame (display.cpp:35-90), drawn on the device --
    def render_frame(self, width=0, height=0, point_size=0, shade="flat"):
        """Queue one frame of the current state (sph_render_frame); does not block."""
        o = _lib.SphRenderOptions()
        o.struct_size = C.sizeof(_lib.SphRenderOptions)
        o.width, o.height, o.point_size = int(width), int(height), int(point_size)
        o.shade = _lib.SHADES[shade] if isinstance(shade, str) else int(shade)
        self._check(self._L.sph_render_frame(self._h, C.byref(o)), "sph_render_frame")

    def _frame_size(self):
        """(pointer, H, W) of the last rendered frame in pinned memory; blocks until it has landed."""
        w, h = C.c_int(0), C.c_int(0)
        p = self._L.sph_frame_host(self._h, C.byref(w), C.byref(h))
        if not p:
            raise SphError("sph_frame_host failed: " + self._L.sph_last_error(self._h).decode())
        return p, h.value, w.value

    def _frame_range(self, call, name):
        lo, hi = C.c_float(0), C.c_float(0)
        self._check(call(self._h, C.byref(lo), C.byref(hi)), name)
        return np.float32(lo.value), np.float32(hi.value)

    def frame_host(self):
        """(H, W, 3) uint8 view of the last rendered frame, row 0 = top of the window; blocks until
        it has landed, valid until the next render."""
        p, h, w = self._frame_size()
        return np.ctypeslib.as_array(p, shape=(h, w, 3))

    def render(self, width=0, height=0, point_size=0, shade="flat"):
        """The frame display.cpp would draw (defaults: 800 x 600, points of size 3, flat blue) as an
        (H, W, 3) uint8 array of its own."""
        self.render_frame(width, height, point_size, shade)
        return np.array(self.frame_host(), copy=True)

    def frame_buffers(self):
        """depth bits, covering-particle count and box-edge depth bits of the last frame: three
        (H, W) uint32 arrays."""
        h, w = self._frame_size()[1:]
        out = [np.zeros((h, w), np.uint32) for _ in range(3)]
        u32p = C.POINTER(C.c_uint32)
        self._check(self._L.sph_download_frame_buffers(self._h, *[a.ctypes.data_as(u32p) for a in out]),
                    "sph_download_frame_buffers")
        return dict(depth=out[0], count=out[1], edge=out[2])

    # -- the field frame: particles coloured by a field of the nearest one (sph_render_field) --
    def render_field(self, field="speed", lo=0.0, hi=0.0, width=0, height=0, point_size=0):
        """Queue one frame coloured by `field` ("speed", "density", "pressure") over the scale lo..hi
        (both 0: the minimum and maximum over all particles, reduced on the device); does not block.
        frame_host() / frame_buffers() serve it like a flat frame."""
        o = _lib.SphFieldFrameOptions()
        o.struct_size = C.sizeof(_lib.SphFieldFrameOptions)
        o.width, o.height, o.point_size = int(width), int(height), int(point_size)
        o.field = _lib.FIELDS[field] if isinstance(field, str) else int(field)
        o.value_lo, o.value_hi = float(lo), float(hi)
        self._check(self._L.sph_render_field(self._h, C.byref(o)), "sph_render_field")

    def field_buffer(self):
        """(H, W) uint32: the bits of the field value of the particle that colours each pixel of the
        last field frame, 0xFFFFFFFF where none covers it."""
        h, w = self._frame_size()[1:]
        out = np.zeros((h, w), np.uint32)
        self._check(self._L.sph_download_field_buffer(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "sph_download_field_buffer")
        return out

    def field_range(self):
        """(lo, hi) as np.float32: the colour scale the last field frame used; blocks until it is known."""
        return self._frame_range(self._L.sph_field_range, "sph_field_range")

    # -- the column frame: how much fluid lies behind each pixel (sph_render_column) --
    def render_column(self, lo=0.0, hi=0.0, width=0, height=0):
        """Queue one column-density frame of the current state over the scale lo..hi (both 0: from 0 to the
        frame's largest column, reduced on the device); does not block.  frame_host() serves its RGB."""
        o = _lib.SphColumnFrameOptions()
        o.struct_size = C.sizeof(_lib.SphColumnFrameOptions)
        o.width, o.height = int(width), int(height)
        o.value_lo, o.value_hi = float(lo), float(hi)
        self._check(self._L.sph_render_column(self._h, C.byref(o)), "sph_render_column")

    def column_buffer(self):
        """(H, W) uint64: the column word of each pixel of the last column frame (value = word / 2**32, 0 where
        no particle reaches the pixel's ray)."""
        h, w = self._frame_size()[1:]
        out = np.zeros((h, w), np.uint64)
        self._check(self._L.sph_download_column_buffer(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))),
                    "sph_download_column_buffer")
        return out

    def column_range(self):
        """(lo, hi) as np.float32: the colour scale the last column frame used; blocks until it is known."""
        return self._frame_range(self._L.sph_column_range, "sph_column_range")

    # -- the liquid frame: the fluid as a shaded water surface (sph_render_liquid) --
    def render_liquid(self, radius=0.0, smooth_iterations=3, smooth_radius=3, smooth_depth=0.0, light=(0.0, 0.0, 0.0),
                      thickness_scale=0.0, width=0, height=0):
        """Queue one liquid frame of the current state; does not block.  frame_host() serves its RGB.  radius: of the
        spheres (0: h); smooth_iterations (0..8) passes of a bilateral filter over (2 smooth_radius + 1)^2 pixels
        (smooth_radius 0..7) that ignores neighbours further than smooth_depth (0: 2 radius) away in depth; light: the
        direction towards the light in view space (all 0: the default); thickness_scale: the column value of optical
        depth 1 (0: the frame's largest column, reduced on the device)."""
        o = _lib.SphLiquidFrameOptions()
        o.struct_size = C.sizeof(_lib.SphLiquidFrameOptions)
        o.width, o.height = int(width), int(height)
        o.radius = float(radius)
        # (the C options keep 0 for "default": a count of 0 is spelled -1 there)
        o.smooth_iterations = -1 if int(smooth_iterations) == 0 else int(smooth_iterations)
        o.smooth_radius = -1 if int(smooth_radius) == 0 else int(smooth_radius)
        o.smooth_depth = float(smooth_depth)
        o.light[0], o.light[1], o.light[2] = (float(v) for v in light)
        o.thickness_scale = float(thickness_scale)
        self._check(self._L.sph_render_liquid(self._h, C.byref(o)), "sph_render_liquid")

    def liquid_buffers(self):
        """{"front", "smooth": (H, W) uint32, the bits of the front depth and of the smoothed depth, 0xFFFFFFFF where
        the pixel is empty; "normals": (H, W, 3) float32; "column": (H, W) uint64} of the last liquid frame."""
        h, w = self._frame_size()[1:]
        out = dict(front=np.zeros((h, w), np.uint32), smooth=np.zeros((h, w), np.uint32),
                   normals=np.zeros((h, w, 3), np.float32), column=np.zeros((h, w), np.uint64))
        u32p = C.POINTER(C.c_uint32)
        self._check(self._L.sph_download_liquid_buffers(
            self._h, out["front"].ctypes.data_as(u32p), out["smooth"].ctypes.data_as(u32p),
            out["normals"].ctypes.data_as(C.POINTER(C.c_float)), out["column"].ctypes.data_as(C.POINTER(C.c_uint64))),
            "sph_download_liquid_buffers")
        return out

    def render_time(self, reset=False):
        """(seconds, frames): GPU time of clear + splat + compose summed over `frames` renders."""
        sec, fr = C.c_double(0), C.c_int64(0)
        self._check(self._L.sph_get_render_time(self._h, C.byref(sec), C.byref(fr), 1 if reset else 0),
                    "sph_get_render_time")
        return sec.value, fr.value

    # -- the field sample: the SPH-interpolated field on a regular lattice (sph_sample_field) --
    def sample_field(self, field="density", origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1), shape=(1, 1, 1)):
        """`field` ("density", "speed", "pressure") of the current state at the lattice points
        origin + (ix, iy, iz) * spacing -- origin and spacing as (x, y, z), spacing also as one number --
        as an np.float32 array of its own of `shape` = (nz, ny, nx).  Points outside the grid give 0."""
        lat = _lib.SphSampleLattice()
        nz, ny, nx = _lattice(lat, shape, origin, spacing)
        lat.field = _lib.FIELDS[field] if isinstance(field, str) else int(field)
        self._check(self._L.sph_sample_field(self._h, C.byref(lat)), "sph_sample_field")
        p = self._L.sph_sample_host(self._h, None, None, None)
        if not p:
            raise SphError("sph_sample_host failed: " + self._L.sph_last_error(self._h).decode())
        return np.array(np.ctypeslib.as_array(p, shape=(nz, ny, nx)), copy=True)

    def sample_time(self, reset=False):
        """(seconds, samples): GPU time of the sampling kernel summed over `samples` calls."""
        sec, cnt = C.c_double(0), C.c_int64(0)
        self._check(self._L.sph_get_sample_time(self._h, C.byref(sec), C.byref(cnt), 1 if reset else 0),
                    "sph_get_sample_time")
        return sec.value, cnt.value

    # -- the surface mesh: the density iso-surface as indexed triangles (sph_extract_surface) --
    def extract_surface(self, iso, origin=(0.0, 0.0, 0.0), spacing=0.1, shape=(2, 2, 2)):
        """The surface density == `iso` of the current state over the lattice origin + (ix, iy, iz) * spacing,
        `shape` = (nz, ny, nx) as for sample_field, by marching tetrahedra on the device: {"vertices": float32
        (V, 3), "triangles": uint32 (T, 3)}, arrays of their own.  Normals (a, b, c -> (b - a) x (c - a)) point out
        of the fluid; the mesh is closed when the lattice's outer shell lies outside it."""
        o = _lib.SphSurfaceOptions()
        _lattice(o, shape, origin, spacing)
        o.iso = float(iso)
        self._check(self._L.sph_extract_surface(self._h, C.byref(o)), "sph_extract_surface")
        vp, tp = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._L.sph_surface_host(self._h, C.byref(vp), C.byref(nv), C.byref(tp), C.byref(nt)),
                    "sph_surface_host")
        return {"vertices": _rows(vp, nv.value, 3, np.float32), "triangles": _rows(tp, nt.value, 3, np.uint32)}

    def surface_time(self, reset=False):
        """(sample_seconds, extract_seconds, calls): GPU time of the surface's sampling kernel and of its
        count + scan + emit launches, summed over `calls` extractions."""
        a, b, cnt = C.c_double(0), C.c_double(0), C.c_int64(0)
        self._check(self._L.sph_get_surface_time(self._h, C.byref(a), C.byref(b), C.byref(cnt), 1 if reset else 0),
                    "sph_get_surface_time")
        return a.value, b.value, cnt.value

    # -- run diagnostics: exact sums, extrema and a histogram, reduced on the device (sph_diagnose) --
    def diagnose(self, hist=None, value_range=None):
        """Queue the reduction of the current state (sph_diagnose); does not block."""
        o = _lib.diagnostics_options(hist, value_range)
        self._check(self._L.sph_diagnose(self._h, C.byref(o)), "sph_diagnose")

    def diagnostics_raw(self):
        """The words of the last diagnose() as an SphDiagnosticsRaw; blocks until they have landed."""
        raw = _lib.SphDiagnosticsRaw()
        self._check(self._L.sph_diagnostics_host(self._h, C.byref(raw)), "sph_diagnostics_host")
        return raw

    def diagnostics(self, hist=None, value_range=None):
        """Mass, centre of mass, momentum, kinetic and potential energy, mean / min / max density, mean pressure,
        the fastest particle, the CFL number and the box of the particles of the current state as Python floats,
        and under "raw" the exact words behind them (sums as Python ints in Q32.32, extrema as float32,
        `saturated`).  hist = "speed" | "density" | "pressure" adds raw["hist"], 256 np.uint64 counts over
        value_range = (lo, hi), or over the field's own minimum and maximum (raw["hist_range"])."""
        self.diagnose(hist, value_range)
        return _lib.diagnostics_dict(self.diagnostics_raw(), self.settings)

    def diagnostics_time(self, reset=False):
        """(seconds, calls): GPU time of the diagnostics launches summed over `calls` calls."""
        sec, cnt = C.c_double(0), C.c_int64(0)
        self._check(self._L.sph_get_diagnostics_time(self._h, C.byref(sec), C.byref(cnt), 1 if reset else 0),
                    "sph_get_diagnostics_time")
        return sec.value, cnt.value

    # -- passive tracers: caller-seeded points carried by the interpolated velocity field (sph_tracers_*) --
    def set_tracers(self, pos):
        """Replace the tracers by the (m, 3) points `pos` (any float32 values; m == 0 clears them).  They belong to
        the caller: setup(), upload_state() and load_state() leave them alone."""
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        self._check(self._L.sph_tracers_set(self._h, _fp(pos) if len(pos) else None, len(pos)), "sph_tracers_set")

    def advect_tracers(self, dt=None):
        """One explicit Euler move of every tracer through the velocity field of the current state; dt = None:
        settings.timestep, dt = 0: sample without moving.  Queues the work; does not block."""
        dt = self.settings.timestep if dt is None else dt
        self._check(self._L.sph_tracers_advect(self._h, C.c_float(dt)), "sph_tracers_advect")

    def tracers(self):
        """{"pos": (m, 3), "den": (m,), "vel": (m, 3)} float32 arrays of their own, in the order the tracers were
        set: the positions after the last advect, the density sum and the velocity it sampled before the move."""
        pd, u, m = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int(0)
        self._check(self._L.sph_tracers_host(self._h, C.byref(pd), C.byref(u), C.byref(m)), "sph_tracers_host")
        pd, u = _rows(pd, m.value, 4, np.float32), _rows(u, m.value, 4, np.float32)
        return dict(pos=np.ascontiguousarray(pd[:, :3]), den=np.ascontiguousarray(pd[:, 3]), vel=np.ascontiguousarray(u[:, :3]))

    def tracer_stats(self, reset=False):
        """dict(calls, waves_shared, waves_direct, groups, seconds): sums since create or the last reset; `seconds`
        is the GPU time of key + sort + walk, the three counters are what the walk kernel counted."""
        st = _lib.SphTracerStats()
        self._check(self._L.sph_get_tracer_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_tracer_stats")
        return dict(calls=st.calls, waves_shared=st.waves_shared, waves_direct=st.waves_direct, groups=st.groups,
                    seconds=st.seconds)

    # -- derived per-particle fields: vorticity, divergence, density gradient, neighbour count (sph_derive) --
    def derive(self):
        """{"vorticity": (n, 3), "divergence": (n,), "grad_rho": (n, 3), "rho": (n,)} float32 and {"neighbours": (n,)}
        uint32 arrays of their own, in particle-id order, of the current state: the SPH curl and divergence of the
        velocity, the gradient of the density (it points into the fluid at a free surface), the density sum itself
        and the number of particles within h (the particle included)."""
        self._check(self._L.sph_derive(self._h), "sph_derive")
        wd, gr, nb, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.c_int(0)
        self._check(self._L.sph_derived_host(self._h, C.byref(wd), C.byref(gr), C.byref(nb), C.byref(n)), "sph_derived_host")
        wd, gr = _rows(wd, n.value, 4, np.float32), _rows(gr, n.value, 4, np.float32)
        return dict(vorticity=np.ascontiguousarray(wd[:, :3]), divergence=np.ascontiguousarray(wd[:, 3]),
                    grad_rho=np.ascontiguousarray(gr[:, :3]), rho=np.ascontiguousarray(gr[:, 3]),
                    neighbours=_rows(nb, n.value, None, np.uint32))

    def derive_stats(self, reset=False):
        """dict(calls, runs_staged, runs_direct, seconds): sums since create or the last reset; `seconds` is the GPU
        time of the sweep, the two counters are the runs the default path walked from LDS and from global memory."""
        st = _lib.SphDeriveStats()
        self._check(self._L.sph_get_derive_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_derive_stats")
        return dict(calls=st.calls, runs_staged=st.runs_staged, runs_direct=st.runs_direct, seconds=st.seconds)

    # -- bodies: the connected pieces of fluid and the piece every particle belongs to (sph_label_bodies) --
    def label_bodies(self, link=0.0):
        """{"labels": (n,) uint32 in particle-id order, "table": (num_bodies, 8) uint32 in ascending label order with
        the columns of _lib.BODY_TABLE (label, count, the bounding box's minimum and maximum as float32 bit patterns:
        table[:, 2:].view(np.float32)), "num_bodies", "largest"}: arrays of their own.  Two particles closer than
        `link` (0: h; else 0 < link <= h) are linked, a body is a connected component of that graph, its label the
        smallest particle id in it; `largest` is the label of the body with the most particles."""
        opt = _lib.SphBodyOptions(C.sizeof(_lib.SphBodyOptions), link)
        self._check(self._L.sph_label_bodies(self._h, C.byref(opt)), "sph_label_bodies")
        lab, tab, n, k, big = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_int(0), C.c_uint32(0)
        self._check(self._L.sph_bodies_host(self._h, C.byref(lab), C.byref(n), C.byref(tab), C.byref(k), C.byref(big)), "sph_bodies_host")
        return dict(labels=_rows(lab, n.value, None, np.uint32), table=_rows(tab, k.value, 8, np.uint32),
                    num_bodies=k.value, largest=big.value)

    def body_stats(self, reset=False):
        """dict(calls, links, unions, rounds, gave_up, seconds): sums since create or the last reset; `links` is the
        number of linked pairs, `unions` n - num_bodies, `rounds` the sweeps of the check path (SPH_BODIES_PLAIN=1),
        `seconds` the GPU time of the kernels."""
        st = _lib.SphBodyStats()
        self._check(self._L.sph_get_body_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_body_stats")
        return dict(calls=st.calls, links=st.links, unions=st.unions, rounds=st.rounds, gave_up=st.gave_up, seconds=st.seconds)

    # -- per-body moments: mass, momentum, spin and shape of every body (sph_measure_bodies) --
    def measure_bodies(self, link=0.0, max_bodies=0):
        """label_bodies()'s dict of the current state plus "moments": a structured array of their own of the raw rows
        (_lib.body_moments_dtype(): label, count, saturated, sum (18, 2) uint64 low / high words of the exact Q32.32
        sums named by _lib.BODY_SUMS), one per body in the table's order, and "size_hist": (32,) uint32, the number
        of bodies with floor(log2(count)) == b.  The moments of more than `max_bodies` bodies (0: no cap) are refused.
        body_values() turns the rows into floats."""
        opt = _lib.SphBodyMeasureOptions(C.sizeof(_lib.SphBodyMeasureOptions), link, int(max_bodies), 0)
        self._check(self._L.sph_measure_bodies(self._h, C.byref(opt)), "sph_measure_bodies")
        lab, tab, n, k, big = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_int(0), C.c_uint32(0)
        self._check(self._L.sph_bodies_host(self._h, C.byref(lab), C.byref(n), C.byref(tab), C.byref(k), C.byref(big)), "sph_bodies_host")
        rows, m, hist = C.POINTER(_lib.SphBodyMomentsRaw)(), C.c_int(0), C.POINTER(C.c_uint32)()
        self._check(self._L.sph_body_moments_host(self._h, C.byref(rows), C.byref(m), C.byref(hist)), "sph_body_moments_host")
        words = _rows(C.cast(rows, C.POINTER(C.c_uint64)), m.value, C.sizeof(_lib.SphBodyMomentsRaw) // 8, np.uint64)
        return dict(labels=_rows(lab, n.value, None, np.uint32), table=_rows(tab, k.value, 8, np.uint32),
                    num_bodies=k.value, largest=big.value,
                    moments=words.view(_lib.body_moments_dtype()).reshape(-1),
                    size_hist=_rows(hist, _lib.BODY_SIZE_BINS, None, np.uint32))

    def body_values(self, moments):
        """The floats behind measure_bodies()["moments"], a structured array (_lib.body_values_dtype()) with one entry
        per body: mass, com, velocity, momentum, kinetic, kinetic_internal (less the energy of the body moving as a
        whole), mean_rho, mean_prs, covariance (xx yy zz xy xz yz of the positions about com), gyration, angular
        (about com) and saturated.  Pure host code."""
        return _lib.body_values(moments, self.settings)

    def body_measure_stats(self, reset=False):
        """dict(calls, seconds): sums since create or the last reset; `seconds` is the GPU time of the moment launches
        alone (the labelling's is body_stats()["seconds"])."""
        st = _lib.SphBodyMeasureStats()
        self._check(self._L.sph_get_body_measure_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_body_measure_stats")
        return dict(calls=st.calls, seconds=st.seconds)

    # -- body tracks: which body is which body of the last call, merges and splits (sph_track_bodies) --
    def track_bodies(self, link=0.0, max_edges=0, moments=False):
        """label_bodies()'s dict of the current state plus its join with the labelling of the last successful
        track_bodies() on this simulator (the reference): "tracks", a structured array (_lib.body_track_dtype()) with
        one entry per body in the table's order -- track, parents, main_parent (row of the previous table, 0xFFFFFFFF
        without parents), main_overlap, flags (_lib.SPH_TRACK_*); "previous" (_lib.body_fate_dtype()), one entry per
        body of the reference -- track, label, count, children, main_child, main_overlap, flags (_lib.SPH_FATE_*);
        "edges" (_lib.body_edge_dtype()): prev, cur, count, flags (_lib.SPH_EDGE_*) in ascending (cur, prev) order; and
        "summary", a dict with the keys of _lib.TRACK_SUMMARY.  A body continues the previous body it shares the most
        particles with where that body's largest piece is this one, and keeps its track; every other body is born with
        a new track.  A result of more than `max_edges` edges (0: no cap) is refused and leaves the reference alone.
        moments=True: also "moments" and "size_hist" as measure_bodies() returns them, of the same labelling."""
        opt = _lib.SphBodyTrackOptions(C.sizeof(_lib.SphBodyTrackOptions), link, int(max_edges),
                                       _lib.SPH_TRACK_WITH_MOMENTS if moments else 0)
        self._check(self._L.sph_track_bodies(self._h, C.byref(opt)), "sph_track_bodies")
        lab, tab, n, k, big = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_int(0), C.c_uint32(0)
        self._check(self._L.sph_bodies_host(self._h, C.byref(lab), C.byref(n), C.byref(tab), C.byref(k), C.byref(big)), "sph_bodies_host")
        tr, fa, ed = C.POINTER(_lib.SphBodyTrack)(), C.POINTER(_lib.SphBodyFate)(), C.POINTER(_lib.SphBodyEdge)()
        nt, nf, ne, summ = C.c_int(0), C.c_int(0), C.c_int(0), _lib.SphBodyTrackSummary()
        self._check(self._L.sph_body_tracks_host(self._h, C.byref(tr), C.byref(nt), C.byref(fa), C.byref(nf), C.byref(ed), C.byref(ne),
                                                 C.byref(summ)), "sph_body_tracks_host")

        def structs(p, count, struct, dtype):
            words = _rows(C.cast(p, C.POINTER(C.c_uint32)), count, C.sizeof(struct) // 4, np.uint32)
            return words.view(dtype).reshape(-1)

        out = dict(labels=_rows(lab, n.value, None, np.uint32), table=_rows(tab, k.value, 8, np.uint32),
                   num_bodies=k.value, largest=big.value,
                   tracks=structs(tr, nt.value, _lib.SphBodyTrack, _lib.body_track_dtype()),
                   previous=structs(fa, nf.value, _lib.SphBodyFate, _lib.body_fate_dtype()),
                   edges=structs(ed, ne.value, _lib.SphBodyEdge, _lib.body_edge_dtype()),
                   summary={name: int(getattr(summ, name)) for name in _lib.TRACK_SUMMARY})
        if moments:
            rows, m, hist = C.POINTER(_lib.SphBodyMomentsRaw)(), C.c_int(0), C.POINTER(C.c_uint32)()
            self._check(self._L.sph_body_moments_host(self._h, C.byref(rows), C.byref(m), C.byref(hist)), "sph_body_moments_host")
            words = _rows(C.cast(rows, C.POINTER(C.c_uint64)), m.value, C.sizeof(_lib.SphBodyMomentsRaw) // 8, np.uint64)
            out.update(moments=words.view(_lib.body_moments_dtype()).reshape(-1),
                       size_hist=_rows(hist, _lib.BODY_SIZE_BINS, None, np.uint32))
        return out

    def track_reset(self):
        """Forgets the reference of track_bodies(): the next call finds no previous bodies and starts tracks at 0."""
        self._check(self._L.sph_track_reset(self._h), "sph_track_reset")

    def body_track_stats(self, reset=False):
        """dict(calls, partials, edges, seconds): sums since create or the last reset; `partials` is the number of
        partial edges the calls sorted (the one number that depends on the kernel path), `edges` the edges, `seconds`
        the GPU time of the track launches alone (the labelling's is body_stats()["seconds"])."""
        st = _lib.SphBodyTrackStats()
        self._check(self._L.sph_get_body_track_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_body_track_stats")
        return dict(calls=st.calls, partials=st.partials, edges=st.edges, seconds=st.seconds)

    # -- neighbour lists: every particle's neighbours within a radius, as CSR (sph_neighbour_lists) --
    def neighbour_lists(self, radius=0.0, walk_order=False, max_entries=0):
        """{"offsets": (n + 1,) uint64, "neighbours": (entries,) uint32}: arrays of their own.  The neighbours of
        particle id i -- the particles within `radius` of it (0: h; else 0 < radius <= h), itself excluded -- are
        neighbours[offsets[i]:offsets[i + 1]], in ascending id order, or (walk_order) in the order in which the density
        sweep's walk of its row meets them.  A result of more than `max_entries` ids (0: 1 << 28) is refused."""
        opt = _lib.SphNeighbourOptions(C.sizeof(_lib.SphNeighbourOptions), radius,
                                       _lib.SPH_NEIGHBOURS_WALK_ORDER if walk_order else 0, 0, int(max_entries))
        self._check(self._L.sph_neighbour_lists(self._h, C.byref(opt)), "sph_neighbour_lists")
        off, nb, n, entries = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_uint64(0)
        self._check(self._L.sph_neighbours_host(self._h, C.byref(off), C.byref(nb), C.byref(n), C.byref(entries)), "sph_neighbours_host")
        return dict(offsets=_rows(off, n.value + 1, None, np.uint64), neighbours=_rows(nb, entries.value, None, np.uint32))

    def neighbour_stats(self, reset=False):
        """dict(calls, entries, longest, runs_staged, runs_direct, seconds): sums since create or the last reset;
        `entries` sums the lists' ids over the calls, `longest` is the longest list of the last call, the two run
        counters are derive_stats()'s over the count and the emit walk, `seconds` the GPU time of count + scan + emit +
        sort."""
        st = _lib.SphNeighbourStats()
        self._check(self._L.sph_get_neighbour_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_neighbour_stats")
        return dict(calls=st.calls, entries=st.entries, longest=st.longest, runs_staged=st.runs_staged,
                    runs_direct=st.runs_direct, seconds=st.seconds)

    # -- pair statistics: g(r) and the velocity structure functions, per bin of separation (sph_pair_statistics) --
    def pair_statistics(self, bins=0, radius=0.0):
        """{"pairs": (B,) uint64, "sums": a (B, 4) object array of Python ints, "words": (B, 4, 2) uint64 -- the low and
        the high word of every sum --, "saturated": (B,) uint64, "edges2": (B,) float32, "rows": the raw rows
        (_lib.pair_bin_dtype())}: arrays of their own.  The unordered pairs of particles within `radius` (0: h; else
        0 < radius <= h) of each other in `bins` bins (0: 32; at most 128) of equal width in r; bin k holds the pairs
        with edges2[k - 1] < d2 <= edges2[k].  sums[k] are the exact Q32.32 sums (value = int / 2**32) named by
        _lib.PAIR_SUMS: d2, |dv|^2, e.dv and (e.dv)^2 / d2.  pair_values() turns them into floats."""
        opt = _lib.SphPairOptions(C.sizeof(_lib.SphPairOptions), 0, radius, int(bins), 0)
        self._check(self._L.sph_pair_statistics(self._h, C.byref(opt)), "sph_pair_statistics")
        rows, edges, b = C.POINTER(_lib.SphPairBinRaw)(), C.POINTER(C.c_float)(), C.c_int(0)
        self._check(self._L.sph_pair_statistics_host(self._h, C.byref(rows), C.byref(edges), C.byref(b)), "sph_pair_statistics_host")
        words = _rows(C.cast(rows, C.POINTER(C.c_uint64)), b.value, C.sizeof(_lib.SphPairBinRaw) // 8, np.uint64)
        raw = words.view(_lib.pair_bin_dtype()).reshape(-1)
        sums = np.empty((b.value, 4), object)
        for k in range(b.value):
            for s in range(4):
                lo, hi = int(raw["sums"][k, s, 0]), int(raw["sums"][k, s, 1])
                sums[k, s] = ((hi - (1 << 64) if hi >> 63 else hi) << 64) | lo
        return dict(pairs=raw["pairs"].copy(), sums=sums, words=raw["sums"].copy(), saturated=raw["saturated"].copy(),
                    edges2=_rows(edges, b.value, None, np.float32), rows=raw)

    def pair_values(self, stats=None, bins=0, radius=0.0):
        """The floats behind pair_statistics() -- of `stats`, a dict it returned, or of a call made here with `bins` and
        `radius` --, a structured array (_lib.pair_values_dtype()) with one entry per bin: r_lo, r_hi, pairs, mean_r2,
        s2 (<|dv|^2>), s2_par (<u_par^2>), approach (<r u_par>: negative where the pairs are closing), g (the radial
        distribution function against an ideal gas of n particles in the box; the walls are not corrected for) and
        saturated.  Pure host code."""
        stats = self.pair_statistics(bins, radius) if stats is None else stats
        return _lib.pair_values(stats["rows"], stats["edges2"], self.settings, self.settings.numParticles)

    def pair_stats(self, reset=False):
        """dict(calls, pairs, runs_staged, runs_direct, seconds): sums since create or the last reset; `pairs` sums the
        tables' pairs over the calls, the two run counters are derive_stats()'s, `seconds` the GPU time of clear + walk
        + join."""
        st = _lib.SphPairStats()
        self._check(self._L.sph_get_pair_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_pair_stats")
        return dict(calls=st.calls, pairs=st.pairs, runs_staged=st.runs_staged, runs_direct=st.runs_direct, seconds=st.seconds)

    # -- ray casting: what a line of sight hits first, and a frame from any camera (sph_cast_rays, sph_render_view) --
    def cast_words(self, origins, directions, t_min=0.0, t_max=np.inf, radius=0.0):
        """(m,) uint64 of its own: per ray o + t d the word (bits(t) << 32) | id of the nearest sphere it enters with
        t_min <= t <= t_max, _lib.CAST_MISS where there is none.  origins, directions: (m, 3); t_min, t_max: numbers or
        (m,) arrays; radius: of the spheres (0: 0.5 h)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        rays = np.zeros(len(o), _lib.ray_dtype())
        rays["o"] = o
        rays["d"] = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        rays["t_min"], rays["t_max"] = t_min, t_max
        opt = _lib.SphCastOptions(C.sizeof(_lib.SphCastOptions), radius)
        self._check(self._L.sph_cast_rays(self._h, rays.ctypes.data_as(C.POINTER(_lib.SphRay)), len(rays), C.byref(opt)), "sph_cast_rays")
        words, m = C.POINTER(C.c_uint64)(), C.c_int(0)
        self._check(self._L.sph_cast_host(self._h, C.byref(words), C.byref(m)), "sph_cast_host")
        return _rows(words, m.value, None, np.uint64)

    def cast_rays(self, origins, directions, t_min=0.0, t_max=np.inf, radius=0.0):
        """(t, ids): (m,) float32 and (m,) int64 of cast_words()' words, inf / -1 for a miss."""
        words = self.cast_words(origins, directions, t_min, t_max, radius)
        miss = words == np.uint64(_lib.CAST_MISS)
        t = (words >> np.uint64(32)).astype(np.uint32).view(np.float32)
        ids = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
        return np.where(miss, np.float32(np.inf), t), np.where(miss, -1, ids)

    def render_view(self, eye, target, up=(0.0, 1.0, 0.0), width=0, height=0, tan_half=(0.0, 0.0), near=0.0, far=0.0, radius=0.0,
                    shade="flat", lo=0.0, hi=0.0, light=(0.0, 0.0, 0.0), edge_radius=0.0):
        """Queue one lit frame of the current state from a pinhole camera at `eye` looking at `target`; does not block.
        frame_host() serves its RGB, view_buffer() its words.  tan_half: (x, y) tangents of the half angles (both 0:
        45 degrees in y, x by the aspect ratio); near / far: the rays' window (0: h / inf); shade: "flat", "speed",
        "density", "pressure" over lo..hi (both 0: the range over all particles); light: towards the light, in world
        space (all 0: the default); edge_radius: of the box edges (0: 0.002 boxDim; negative: none)."""
        o = _lib.SphViewOptions()
        o.struct_size = C.sizeof(_lib.SphViewOptions)
        o.width, o.height = int(width), int(height)
        o.eye[:], o.target[:], o.up[:] = [float(v) for v in eye], [float(v) for v in target], [float(v) for v in up]
        o.tan_half_x, o.tan_half_y = float(tan_half[0]), float(tan_half[1])
        o.near, o.far, o.radius = float(near), float(far), float(radius)
        o.shade = _lib.VIEW_SHADES[shade] if isinstance(shade, str) else int(shade)
        o.value_lo, o.value_hi = float(lo), float(hi)
        o.light[:] = [float(v) for v in light]
        o.edge_radius = float(edge_radius)
        self._check(self._L.sph_render_view(self._h, C.byref(o)), "sph_render_view")

    def view_buffer(self):
        """(H, W) uint64: the word of each pixel's ray of the last view frame (cast_words()' words)."""
        h, w = self._frame_size()[1:]
        out = np.zeros((h, w), np.uint64)
        self._check(self._L.sph_download_view_buffer(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "sph_download_view_buffer")
        return out

    def cast_stats(self, reset=False):
        """dict(calls, rays, layers, tests, seconds): sums since create or the last reset over casts and views; `layers`
        and `tests` count the grid layers looked into and the ray-particle pairs tested, `seconds` is the GPU time of
        cast_rays()' kernels (a view's is in render_time())."""
        st = _lib.SphCastStats()
        self._check(self._L.sph_get_cast_stats(self._h, C.byref(st), 1 if reset else 0), "sph_get_cast_stats")
        return dict(calls=st.calls, rays=st.rays, layers=st.layers, tests=st.tests, seconds=st.seconds)

    def phase(self, name):
        self._check(getattr(self._L, "sph_phase_" + name)(self._h), "sph_phase_" + name)

    def sync(self):
        self._check(self._L.sph_sync(self._h), "sph_sync")

    def kernel_times(self, reset=False):
        kt = SphKernelTimes()
        self._check(self._L.sph_get_kernel_times(self._h, C.byref(kt), 1 if reset else 0),
                    "sph_get_kernel_times")
        return kt


def sort_check(keys, key_bits=20, device=-1):
    """Run the grid build's radix sort alone (tests)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = len(keys)
    perm = np.zeros(n, np.uint32)
    sk = np.zeros(n, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = load_library().sph_sort_check(device, keys.ctypes.data_as(u32p), n, key_bits,
                                       perm.ctypes.data_as(u32p), sk.ctypes.data_as(u32p))
    if rc:
        raise SphError(f"sph_sort_check failed ({rc})")
    return perm, sk
