"""ctypes binding of libsph_hip.so -- declarations mirror include/sph_c_api.h."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libsph_hip.so"

SPH_MATH_STRICT, SPH_MATH_FAST = 0, 1
SPH_SWEEP_LIST, SPH_SWEEP_DIRECT, SPH_SWEEP_LDS = 0, 1, 2
SWEEPS = {"list": 0, "direct": 1, "lds": 2, "linked": 3}
SPH_FLAG_COUNT_PAIRS, SPH_FLAG_STORE_FORCE, SPH_FLAG_NO_READBACK = 1, 2, 4
SPH_FLAG_EXTERNAL_STATE = 8
SPH_FLAG_MAPPED_POSITIONS = 16

# every symbol include/sph_c_api.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "sph_default_settings", "sph_create", "sph_destroy", "sph_setup", "sph_upload_state",
    "sph_step", "sph_apply_click", "sph_positions_host", "sph_download_state",
    "sph_download_force", "sph_download_grid", "sph_sync", "sph_num_particles",
    "sph_get_kernel_times", "sph_last_error", "sph_phase_grid", "sph_phase_density",
    "sph_phase_force", "sph_phase_readback", "sph_sort_check", "sph_build_info",
    "sph_set_stream", "sph_bind_buffers", "sph_slab_sort", "sph_slab_partition", "sph_slab_copy_segments", "sph_slab_density",
    "sph_slab_force", "sph_initial_positions", "sph_save_state", "sph_load_state",
    "sph_debug_counters", "sph_get_stream", "sph_slab_partition_async", "sph_slab_sort_async",
    "sph_slab_patch_halo", "sph_slab_force_ranges", "sph_num_table_cells", "sph_slab_apply_click", "sph_slab_records",
    "sph_render_frame", "sph_frame_host", "sph_download_frame_buffers", "sph_get_render_time", "sph_api_version",
    "sph_render_field", "sph_download_field_buffer", "sph_field_range",
    "sph_render_column", "sph_download_column_buffer", "sph_column_range",
    "sph_render_liquid", "sph_download_liquid_buffers",
    "sph_sample_field", "sph_sample_host", "sph_get_sample_time",
    "sph_extract_surface", "sph_surface_host", "sph_get_surface_time",
    "sph_diagnose", "sph_diagnostics_host", "sph_diagnostics_values", "sph_diagnostics_add",
    "sph_get_diagnostics_time", "sph_slab_diagnose",
    "sph_tracers_set", "sph_tracers_advect", "sph_tracers_host", "sph_get_tracer_stats",
    "sph_derive", "sph_derived_host", "sph_get_derive_stats",
    "sph_label_bodies", "sph_bodies_host", "sph_get_body_stats",
    "sph_measure_bodies", "sph_body_moments_host", "sph_body_values", "sph_get_body_measure_stats",
    "sph_track_bodies", "sph_body_tracks_host", "sph_track_reset", "sph_get_body_track_stats",
    "sph_neighbour_lists", "sph_neighbours_host", "sph_get_neighbour_stats",
    "sph_pair_edges", "sph_pair_statistics", "sph_pair_statistics_host", "sph_pair_values", "sph_get_pair_stats",
    "sph_cast_rays", "sph_cast_host", "sph_render_view", "sph_download_view_buffer", "sph_get_cast_stats",
]
SPH_API_VERSION = 3
SPH_SHADE_FLAT, SPH_SHADE_COUNT = 0, 1
SHADES = {"flat": SPH_SHADE_FLAT, "count": SPH_SHADE_COUNT}
SPH_HAS_FIELD_FRAME = 1
SPH_FIELD_SPEED, SPH_FIELD_DENSITY, SPH_FIELD_PRESSURE = 0, 1, 2
FIELDS = {"speed": SPH_FIELD_SPEED, "density": SPH_FIELD_DENSITY, "pressure": SPH_FIELD_PRESSURE}
SPH_HAS_COLUMN_FRAME = 1
SPH_HAS_LIQUID_FRAME = 1
SPH_HAS_FIELD_SAMPLE = 1
SPH_HAS_SURFACE = 1
SPH_HAS_DIAGNOSTICS = 1
SPH_HAS_TRACERS = 1
MAX_TRACERS = 1 << 24
SPH_HAS_DERIVED = 1
SPH_HAS_BODIES = 1
SPH_HAS_BODY_MOMENTS = 1
SPH_HAS_BODY_TRACKS = 1
SPH_TRACK_WITH_MOMENTS = 1
SPH_EDGE_MAIN_PARENT, SPH_EDGE_MAIN_CHILD = 1, 2
SPH_TRACK_CONTINUES, SPH_TRACK_BORN, SPH_TRACK_MERGED = 1, 2, 4
SPH_FATE_CONTINUES, SPH_FATE_ENDED, SPH_FATE_SPLIT = 1, 2, 4
SPH_HAS_NEIGHBOURS = 1
SPH_NEIGHBOURS_WALK_ORDER = 1
SPH_HAS_PAIR_STATS = 1
PAIR_MAX_BINS = 128
PAIR_SUMS = ("d2", "w2", "a", "l2")   # SPH_PAIR_SUM_*
SPH_HAS_RAY_CAST = 1
CAST_MAX_RAYS = 1 << 24
CAST_MISS = 0xFFFFFFFFFFFFFFFF
SPH_VIEW_FLAT, SPH_VIEW_FIELD = 0, 1
VIEW_SHADES = {"flat": SPH_VIEW_FLAT, "speed": SPH_VIEW_FIELD + SPH_FIELD_SPEED, "density": SPH_VIEW_FIELD + SPH_FIELD_DENSITY,
               "pressure": SPH_VIEW_FIELD + SPH_FIELD_PRESSURE}
BODY_TABLE = ("label", "count", "min_x", "min_y", "min_z", "max_x", "max_y", "max_z")   # words of a table row
DIAG_SUMS = ("x", "y", "z", "vx", "vy", "vz", "rho", "prs", "v2")   # SPH_DIAG_SUM_*
BODY_SUMS = DIAG_SUMS + ("xx", "yy", "zz", "xy", "xz", "yz", "lx", "ly", "lz")   # ... then SPH_BODY_SUM_*
BODY_SIZE_BINS = 32
DIAG_EXTREMA = ("x", "y", "z", "speed", "rho", "prs")               # SPH_DIAG_EXT_*
DIAG_BINS = 256


class SphError(RuntimeError):
    pass


class SphSettings(C.Structure):
    _fields_ = [("randomInit", C.c_uint8), ("pad_", C.c_uint8 * 3),
                ("numParticles", C.c_int32), ("h", C.c_float),
                ("v_kernel_coeff", C.c_float), ("d_kernel_coeff", C.c_float),
                ("boxDim", C.c_float), ("numCellsPerDim", C.c_float),
                ("timestep", C.c_float)]


class SphTimes(C.Structure):
    _fields_ = [("buildGrid", C.c_double), ("sphUpdate", C.c_double),
                ("memcpy", C.c_double), ("iters", C.c_int32)]


class SphOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32),
                ("math_mode", C.c_int32), ("sweep", C.c_int32), ("flags", C.c_int32),
                ("capacity", C.c_int32), ("key_order", C.c_int32)]


class SphRenderOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("point_size", C.c_int32), ("shade", C.c_int32)]


class SphFieldFrameOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("point_size", C.c_int32), ("field", C.c_int32),
                ("value_lo", C.c_float), ("value_hi", C.c_float)]


class SphColumnFrameOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("value_lo", C.c_float), ("value_hi", C.c_float)]


class SphLiquidFrameOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("radius", C.c_float), ("smooth_iterations", C.c_int32), ("smooth_radius", C.c_int32),
                ("smooth_depth", C.c_float), ("light", C.c_float * 3), ("thickness_scale", C.c_float)]


class SphSampleLattice(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("field", C.c_int32)]


class SphSurfaceOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("iso", C.c_float)]


class SphSum128(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_int64)]


class SphDiagnosticsOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hist_field", C.c_int32),
                ("value_lo", C.c_float), ("value_hi", C.c_float)]


class SphDiagnosticsRaw(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("n", C.c_int64),
                ("sum", SphSum128 * 9), ("min_bits", C.c_uint32 * 6), ("max_bits", C.c_uint32 * 6),
                ("saturated", C.c_uint64), ("hist_field", C.c_int32),
                ("hist_lo_bits", C.c_uint32), ("hist_hi_bits", C.c_uint32), ("pad2_", C.c_int32),
                ("hist", C.c_uint64 * DIAG_BINS)]


class SphDiagnostics(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("n", C.c_int64),
                ("mass", C.c_double), ("com", C.c_double * 3), ("momentum", C.c_double * 3),
                ("kinetic", C.c_double), ("potential", C.c_double),
                ("mean_rho", C.c_double), ("mean_prs", C.c_double),
                ("min_rho", C.c_double), ("max_rho", C.c_double),
                ("max_speed", C.c_double), ("cfl", C.c_double),
                ("box_min", C.c_double * 3), ("box_max", C.c_double * 3), ("saturated", C.c_uint64)]


def diagnostics_options(hist=None, value_range=None):
    """SphDiagnosticsOptions for a histogram of `hist` (a FIELDS name or SPH_FIELD_*; None: no histogram) over
    value_range = (lo, hi) (None: the minimum and maximum of the field, reduced on the device)"""
    o = SphDiagnosticsOptions()
    o.struct_size = C.sizeof(SphDiagnosticsOptions)
    o.hist_field = -1 if hist is None else FIELDS[hist] if isinstance(hist, str) else int(hist)
    if value_range is not None:
        o.value_lo, o.value_hi = float(value_range[0]), float(value_range[1])
    return o


def diagnostics_dict(raw, settings):
    """The dict Simulator.diagnostics() returns, from the words `raw` (SphDiagnosticsRaw): the derived floats of
    sph_diagnostics_values and, under "raw", the sums as Python ints (Q32.32: value = int / 2**32), the extrema as
    float32, the histogram as an np.uint64 array and `saturated`."""
    import numpy as np
    v = SphDiagnostics()
    rc = load_library().sph_diagnostics_values(C.byref(raw), C.byref(settings), C.byref(v))
    if rc:
        raise SphError(f"sph_diagnostics_values failed ({rc})")
    out = dict(n=v.n, mass=v.mass, com=tuple(v.com), momentum=tuple(v.momentum), kinetic=v.kinetic,
               potential=v.potential, mean_rho=v.mean_rho, mean_prs=v.mean_prs, min_rho=v.min_rho, max_rho=v.max_rho,
               max_speed=v.max_speed, cfl=v.cfl, box_min=tuple(v.box_min), box_max=tuple(v.box_max),
               saturated=v.saturated)
    bits = lambda a: np.array(list(a), np.uint32).view(np.float32)
    out["raw"] = dict(
        n=raw.n,
        sums={name: (raw.sum[k].hi << 64) | raw.sum[k].lo for k, name in enumerate(DIAG_SUMS)},
        min=dict(zip(DIAG_EXTREMA, bits(raw.min_bits))), max=dict(zip(DIAG_EXTREMA, bits(raw.max_bits))),
        saturated=raw.saturated, hist_field=raw.hist_field,
        hist_range=tuple(bits([raw.hist_lo_bits, raw.hist_hi_bits])),
        hist=np.array(list(raw.hist), np.uint64), struct=raw)
    return out


class SphTracerStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64),
                ("waves_shared", C.c_uint64), ("waves_direct", C.c_uint64), ("groups", C.c_uint64),
                ("seconds", C.c_double)]


class SphDeriveStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64),
                ("runs_staged", C.c_uint64), ("runs_direct", C.c_uint64), ("seconds", C.c_double)]


class SphBodyOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("link", C.c_float)]


class SphBodyStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("links", C.c_uint64),
                ("unions", C.c_uint64), ("rounds", C.c_uint64), ("gave_up", C.c_uint64), ("seconds", C.c_double)]


class SphBodyMeasureOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("link", C.c_float), ("max_bodies", C.c_uint32), ("pad_", C.c_int32)]


class SphBodyMomentsRaw(C.Structure):
    _fields_ = [("label", C.c_uint32), ("count", C.c_uint32), ("saturated", C.c_uint64), ("sum", SphSum128 * 18)]


class SphBodyValues(C.Structure):
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("velocity", C.c_double * 3), ("momentum", C.c_double * 3),
                ("kinetic", C.c_double), ("kinetic_internal", C.c_double), ("mean_rho", C.c_double), ("mean_prs", C.c_double),
                ("covariance", C.c_double * 6), ("gyration", C.c_double), ("angular", C.c_double * 3),
                ("saturated", C.c_uint64)]


class SphBodyMeasureStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("seconds", C.c_double)]


def body_moments_dtype():
    """the numpy dtype of an SphBodyMomentsRaw row: label, count, saturated, and sum as (18, 2) uint64 -- [k, 0] the low
    and [k, 1] the high word of sum k (two's complement; BODY_SUMS names the sums)"""
    import numpy as np
    return np.dtype([("label", "<u4"), ("count", "<u4"), ("saturated", "<u8"), ("sum", "<u8", (18, 2))])


def body_values_dtype():
    """the numpy dtype of an SphBodyValues"""
    import numpy as np
    return np.dtype([(name, "<u8" if name == "saturated" else "<f8", () if not hasattr(t, "_length_") else (t._length_,))
                     for name, t in SphBodyValues._fields_])


def body_values(moments, settings):
    """sph_body_values over a structured array of raw rows (body_moments_dtype) -> a structured array of
    body_values_dtype, one entry per body.  Pure host code: no GPU, no handle."""
    import numpy as np
    rows = np.ascontiguousarray(moments, dtype=body_moments_dtype()).reshape(-1)
    out = np.zeros(len(rows), body_values_dtype())
    rc = load_library().sph_body_values(rows.ctypes.data_as(C.POINTER(SphBodyMomentsRaw)), len(rows), C.byref(settings),
                                        out.ctypes.data_as(C.POINTER(SphBodyValues)))
    if rc:
        raise SphError(f"sph_body_values failed ({rc})")
    return out


class SphBodyTrackOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("link", C.c_float), ("max_edges", C.c_uint32), ("flags", C.c_uint32)]


class SphBodyEdge(C.Structure):
    _fields_ = [("prev", C.c_uint32), ("cur", C.c_uint32), ("count", C.c_uint32), ("flags", C.c_uint32)]


class SphBodyTrack(C.Structure):
    _fields_ = [("track", C.c_uint64), ("parents", C.c_uint32), ("main_parent", C.c_uint32), ("main_overlap", C.c_uint32),
                ("flags", C.c_uint32)]


class SphBodyFate(C.Structure):
    _fields_ = [("track", C.c_uint64), ("label", C.c_uint32), ("count", C.c_uint32), ("children", C.c_uint32),
                ("main_child", C.c_uint32), ("main_overlap", C.c_uint32), ("flags", C.c_uint32)]


class SphBodyTrackSummary(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("previous_bodies", C.c_uint32), ("bodies", C.c_uint32),
                ("edges", C.c_uint32), ("continued", C.c_uint32), ("born", C.c_uint32), ("ended", C.c_uint32),
                ("merges", C.c_uint32), ("splits", C.c_uint32), ("next_track", C.c_uint64), ("sequence", C.c_uint64)]


class SphBodyTrackStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("partials", C.c_uint64),
                ("edges", C.c_uint64), ("seconds", C.c_double)]


TRACK_SUMMARY = ("previous_bodies", "bodies", "edges", "continued", "born", "ended", "merges", "splits", "next_track", "sequence")


def _struct_dtype(struct):
    import numpy as np
    kinds = {C.c_uint32: "<u4", C.c_uint64: "<u8"}
    return np.dtype([(name, kinds[t]) for name, t in struct._fields_])


def body_edge_dtype():
    """the numpy dtype of an SphBodyEdge: prev, cur (rows of the two tables), count, flags"""
    return _struct_dtype(SphBodyEdge)


def body_track_dtype():
    """the numpy dtype of an SphBodyTrack (one per current body): track, parents, main_parent, main_overlap, flags"""
    return _struct_dtype(SphBodyTrack)


def body_fate_dtype():
    """the numpy dtype of an SphBodyFate (one per previous body): track, label, count, children, main_child,
    main_overlap, flags"""
    return _struct_dtype(SphBodyFate)


class SphNeighbourOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("radius", C.c_float), ("flags", C.c_int32), ("pad_", C.c_int32),
                ("max_entries", C.c_uint64)]


class SphNeighbourStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("entries", C.c_uint64),
                ("longest", C.c_uint64), ("runs_staged", C.c_uint64), ("runs_direct", C.c_uint64), ("seconds", C.c_double)]


class SphPairOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("flags", C.c_int32), ("radius", C.c_float), ("bins", C.c_int32), ("pad_", C.c_int32)]


class SphPairBinRaw(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("sums", SphSum128 * 4), ("saturated", C.c_uint64)]


class SphPairValues(C.Structure):
    _fields_ = [("r_lo", C.c_double), ("r_hi", C.c_double), ("pairs", C.c_double), ("mean_r2", C.c_double), ("s2", C.c_double),
                ("s2_par", C.c_double), ("approach", C.c_double), ("g", C.c_double), ("saturated", C.c_uint64)]


class SphPairStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("pairs", C.c_uint64),
                ("runs_staged", C.c_uint64), ("runs_direct", C.c_uint64), ("seconds", C.c_double)]


class SphRay(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("t_min", C.c_float), ("d", C.c_float * 3), ("t_max", C.c_float)]


class SphCastOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("radius", C.c_float)]


class SphViewOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("eye", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3),
                ("tan_half_x", C.c_float), ("tan_half_y", C.c_float), ("near", C.c_float), ("far", C.c_float),
                ("radius", C.c_float), ("shade", C.c_int32), ("value_lo", C.c_float), ("value_hi", C.c_float),
                ("light", C.c_float * 3), ("edge_radius", C.c_float)]


class SphCastStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("pad_", C.c_int32), ("calls", C.c_int64), ("rays", C.c_uint64),
                ("layers", C.c_uint64), ("tests", C.c_uint64), ("seconds", C.c_double)]


def ray_dtype():
    """the numpy dtype of an SphRay: o (3 floats), t_min, d (3 floats), t_max"""
    import numpy as np
    return np.dtype([("o", "<f4", (3,)), ("t_min", "<f4"), ("d", "<f4", (3,)), ("t_max", "<f4")])


def pair_bin_dtype():
    """the numpy dtype of an SphPairBinRaw row: pairs, sums as (4, 2) uint64 -- [k, 0] the low and [k, 1] the high word of
    sum k (two's complement; PAIR_SUMS names the sums) --, saturated"""
    import numpy as np
    return np.dtype([("pairs", "<u8"), ("sums", "<u8", (4, 2)), ("saturated", "<u8")])


def pair_values_dtype():
    """the numpy dtype of an SphPairValues"""
    import numpy as np
    return np.dtype([(name, "<u8" if name == "saturated" else "<f8") for name, _ in SphPairValues._fields_])


def pair_edges(radius, h, bins=0):
    """sph_pair_edges: the (bins,) float32 squared outer edges of `bins` bins (0: 32) of equal width up to `radius`
    (0: h).  Pure host code: no GPU, no handle."""
    import numpy as np
    out = np.zeros(PAIR_MAX_BINS, np.float32)
    rc = load_library().sph_pair_edges(C.c_float(radius), C.c_float(h), int(bins), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise SphError(f"sph_pair_edges failed ({rc})")
    return out[:int(bins) if bins else 32].copy()


def pair_values(rows, edges2, settings, n):
    """sph_pair_values over a structured array of raw rows (pair_bin_dtype) and their squared edges -> a structured array
    of pair_values_dtype, one entry per bin, for n particles in the box of `settings`.  Pure host code."""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=pair_bin_dtype()).reshape(-1)
    edges2 = np.ascontiguousarray(edges2, dtype=np.float32).reshape(-1)
    if len(edges2) != len(rows):
        raise SphError("pair_values: as many edges as rows")
    out = np.zeros(len(rows), pair_values_dtype())
    rc = load_library().sph_pair_values(rows.ctypes.data_as(C.POINTER(SphPairBinRaw)), edges2.ctypes.data_as(C.POINTER(C.c_float)),
                                        len(rows), C.byref(settings), int(n), out.ctypes.data_as(C.POINTER(SphPairValues)))
    if rc:
        raise SphError(f"sph_pair_values failed ({rc})")
    return out


class SphKernelTimes(C.Structure):
    _fields_ = [("hash", C.c_double), ("sort", C.c_double), ("gather", C.c_double),
                ("density", C.c_double), ("force", C.c_double), ("readback", C.c_double),
                ("pair_tests", C.c_uint64), ("steps", C.c_int64), ("pair_hits", C.c_uint64)]


def library_path():
    # SPH_LIB_PATH: A/B experiments with differently-built libraries (same ABI)
    return os.environ.get("SPH_LIB_PATH") or os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_library():
    """Load libsph_hip.so; fail loudly if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise SphError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C cudafluidsimulator_amd/csrc`. There is no CPU fallback.")
    L = C.CDLL(path)
    fp = C.POINTER(C.c_float)
    u32p = C.POINTER(C.c_uint32)
    i32p = C.POINTER(C.c_int32)
    hp = C.c_void_p
    L.sph_default_settings.argtypes = [C.POINTER(SphSettings), C.c_int, C.c_int]
    L.sph_initial_positions.argtypes = [C.POINTER(SphSettings), fp]
    L.sph_create.argtypes = [C.POINTER(SphSettings), C.POINTER(SphOptions), C.POINTER(hp)]
    L.sph_destroy.argtypes = [hp]
    L.sph_destroy.restype = None
    L.sph_setup.argtypes = [hp]
    L.sph_upload_state.argtypes = [hp, fp, fp, C.c_int]
    L.sph_step.argtypes = [hp, C.POINTER(SphTimes)]
    L.sph_apply_click.argtypes = [hp, C.c_int, C.c_int]
    L.sph_positions_host.argtypes = [hp]
    L.sph_positions_host.restype = fp
    L.sph_download_state.argtypes = [hp, fp, fp, fp, fp]
    L.sph_download_force.argtypes = [hp, fp]
    L.sph_download_grid.argtypes = [hp, u32p, u32p, i32p]
    L.sph_sync.argtypes = [hp]
    L.sph_debug_counters.argtypes = [hp, C.POINTER(C.c_uint64)]
    L.sph_save_state.argtypes = [hp, C.c_char_p]
    L.sph_load_state.argtypes = [hp, C.c_char_p]
    L.sph_num_particles.argtypes = [hp]
    L.sph_num_table_cells.argtypes = [hp]
    L.sph_get_kernel_times.argtypes = [hp, C.POINTER(SphKernelTimes), C.c_int]
    L.sph_last_error.argtypes = [hp]
    L.sph_last_error.restype = C.c_char_p
    for name in ("sph_phase_grid", "sph_phase_density", "sph_phase_force",
                 "sph_phase_readback"):
        getattr(L, name).argtypes = [hp]
    L.sph_sort_check.argtypes = [C.c_int, u32p, C.c_int, C.c_int, u32p, u32p]
    L.sph_build_info.restype = C.c_char_p
    L.sph_set_stream.argtypes = [hp, C.c_void_p]
    L.sph_bind_buffers.argtypes = [hp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.sph_slab_sort.argtypes = [hp, C.c_int, C.c_int, C.c_int, u32p, C.c_int, i32p]
    L.sph_slab_copy_segments.argtypes = [hp, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         i32p, i32p]
    L.sph_slab_partition.argtypes = [hp, C.c_int, C.c_int, C.c_int, u32p, C.c_int, i32p, C.c_void_p]
    L.sph_slab_density.argtypes = [hp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sph_slab_force.argtypes = [hp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sph_render_frame.argtypes = [hp, C.POINTER(SphRenderOptions)]
    L.sph_frame_host.argtypes = [hp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sph_frame_host.restype = C.POINTER(C.c_uint8)
    L.sph_download_frame_buffers.argtypes = [hp, u32p, u32p, u32p]
    L.sph_get_render_time.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.sph_api_version.argtypes = []
    L.sph_render_field.argtypes = [hp, C.POINTER(SphFieldFrameOptions)]
    L.sph_download_field_buffer.argtypes = [hp, u32p]
    L.sph_field_range.argtypes = [hp, fp, fp]
    L.sph_render_column.argtypes = [hp, C.POINTER(SphColumnFrameOptions)]
    L.sph_download_column_buffer.argtypes = [hp, C.POINTER(C.c_uint64)]
    L.sph_column_range.argtypes = [hp, fp, fp]
    L.sph_render_liquid.argtypes = [hp, C.POINTER(SphLiquidFrameOptions)]
    L.sph_download_liquid_buffers.argtypes = [hp, u32p, u32p, fp, C.POINTER(C.c_uint64)]
    L.sph_sample_field.argtypes = [hp, C.POINTER(SphSampleLattice)]
    L.sph_sample_host.argtypes = [hp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sph_sample_host.restype = fp
    L.sph_get_sample_time.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.sph_extract_surface.argtypes = [hp, C.POINTER(SphSurfaceOptions)]
    L.sph_surface_host.argtypes = [hp, C.POINTER(fp), C.POINTER(C.c_int64), C.POINTER(u32p), C.POINTER(C.c_int64)]
    L.sph_get_surface_time.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.sph_diagnose.argtypes = [hp, C.POINTER(SphDiagnosticsOptions)]
    L.sph_diagnostics_host.argtypes = [hp, C.POINTER(SphDiagnosticsRaw)]
    L.sph_diagnostics_values.argtypes = [C.POINTER(SphDiagnosticsRaw), C.POINTER(SphSettings), C.POINTER(SphDiagnostics)]
    L.sph_diagnostics_add.argtypes = [C.POINTER(SphDiagnosticsRaw), C.POINTER(SphDiagnosticsRaw)]
    L.sph_get_diagnostics_time.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.sph_slab_diagnose.argtypes = [hp, C.c_int, C.c_int, C.c_int, C.POINTER(SphDiagnosticsOptions)]
    L.sph_tracers_set.argtypes = [hp, fp, C.c_int]
    L.sph_tracers_advect.argtypes = [hp, C.c_float]
    L.sph_tracers_host.argtypes = [hp, C.POINTER(fp), C.POINTER(fp), C.POINTER(C.c_int)]
    L.sph_get_tracer_stats.argtypes = [hp, C.POINTER(SphTracerStats), C.c_int]
    L.sph_derive.argtypes = [hp]
    L.sph_derived_host.argtypes = [hp, C.POINTER(fp), C.POINTER(fp), C.POINTER(u32p), C.POINTER(C.c_int)]
    L.sph_get_derive_stats.argtypes = [hp, C.POINTER(SphDeriveStats), C.c_int]
    L.sph_label_bodies.argtypes = [hp, C.POINTER(SphBodyOptions)]
    L.sph_bodies_host.argtypes = [hp, C.POINTER(u32p), C.POINTER(C.c_int), C.POINTER(u32p), C.POINTER(C.c_int),
                                  C.POINTER(C.c_uint32)]
    L.sph_get_body_stats.argtypes = [hp, C.POINTER(SphBodyStats), C.c_int]
    L.sph_measure_bodies.argtypes = [hp, C.POINTER(SphBodyMeasureOptions)]
    L.sph_body_moments_host.argtypes = [hp, C.POINTER(C.POINTER(SphBodyMomentsRaw)), C.POINTER(C.c_int), C.POINTER(u32p)]
    L.sph_body_values.argtypes = [C.POINTER(SphBodyMomentsRaw), C.c_int, C.POINTER(SphSettings), C.POINTER(SphBodyValues)]
    L.sph_get_body_measure_stats.argtypes = [hp, C.POINTER(SphBodyMeasureStats), C.c_int]
    L.sph_track_bodies.argtypes = [hp, C.POINTER(SphBodyTrackOptions)]
    L.sph_body_tracks_host.argtypes = [hp, C.POINTER(C.POINTER(SphBodyTrack)), C.POINTER(C.c_int), C.POINTER(C.POINTER(SphBodyFate)),
                                       C.POINTER(C.c_int), C.POINTER(C.POINTER(SphBodyEdge)), C.POINTER(C.c_int),
                                       C.POINTER(SphBodyTrackSummary)]
    L.sph_track_reset.argtypes = [hp]
    L.sph_get_body_track_stats.argtypes = [hp, C.POINTER(SphBodyTrackStats), C.c_int]
    L.sph_neighbour_lists.argtypes = [hp, C.POINTER(SphNeighbourOptions)]
    L.sph_neighbours_host.argtypes = [hp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(u32p), C.POINTER(C.c_int),
                                      C.POINTER(C.c_uint64)]
    L.sph_get_neighbour_stats.argtypes = [hp, C.POINTER(SphNeighbourStats), C.c_int]
    L.sph_pair_edges.argtypes = [C.c_float, C.c_float, C.c_int, fp]
    L.sph_pair_statistics.argtypes = [hp, C.POINTER(SphPairOptions)]
    L.sph_pair_statistics_host.argtypes = [hp, C.POINTER(C.POINTER(SphPairBinRaw)), C.POINTER(fp), C.POINTER(C.c_int)]
    L.sph_pair_values.argtypes = [C.POINTER(SphPairBinRaw), fp, C.c_int, C.POINTER(SphSettings), C.c_int64, C.POINTER(SphPairValues)]
    L.sph_get_pair_stats.argtypes = [hp, C.POINTER(SphPairStats), C.c_int]
    L.sph_cast_rays.argtypes = [hp, C.POINTER(SphRay), C.c_int, C.POINTER(SphCastOptions)]
    L.sph_cast_host.argtypes = [hp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int)]
    L.sph_render_view.argtypes = [hp, C.POINTER(SphViewOptions)]
    L.sph_download_view_buffer.argtypes = [hp, C.POINTER(C.c_uint64)]
    L.sph_get_cast_stats.argtypes = [hp, C.POINTER(SphCastStats), C.c_int]
    _lib = L
    return L
