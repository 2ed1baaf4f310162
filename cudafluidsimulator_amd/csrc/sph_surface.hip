// The surface mesh: sph_extract_surface and what reads its results (kernels: sample.hip for the field, surface.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

int surface_reserve_lattice(sph_handle *h, size_t points, size_t blocks) {
    if (points > h->surfPointCap || blocks > h->surfBlockCap || !h->surfTotalsDev) {
        int rc = pass_quiesce(h, h->surf);
        if (rc) return rc;
    }
    if (points > h->surfPointCap) {
        h->surfPointCap = 0;
        HIPCHK(h, h->surfField.alloc(points));
        HIPCHK(h, h->surfBits.alloc(points));
        HIPCHK(h, h->surfLocal.alloc(points));
        h->surfPointCap = points;
    }
    if (blocks > h->surfBlockCap) {
        h->surfBlockCap = 0;
        HIPCHK(h, h->surfBlockSum.alloc(blocks));
        HIPCHK(h, h->surfBlockOff.alloc(blocks));
        h->surfBlockCap = blocks;
    }
    if (!h->surfTotalsDev) {
        HIPCHK(h, h->surfTotalsDev.alloc(2));
        HIPCHK(h, h->surfTotalsHost.alloc(2));
    }
    return SPH_OK;
}

// (the compute stream is idle here: the host has just waited for the totals)
int surface_reserve_mesh(sph_handle *h, size_t verts, size_t tris) {
    if (verts <= h->surfVertCap && tris <= h->surfTriCap) return SPH_OK;
    HIPCHK(h, hipStreamSynchronize(h->copy)); // the last mesh may still be on its way out of the old buffers
    if (verts > h->surfVertCap) {
        h->surfVertCap = 0;
        HIPCHK(h, h->surfVertsDev.alloc(verts * 3));
        HIPCHK(h, h->surfVertsHost.alloc(verts * 3));
        h->surfVertCap = verts;
    }
    if (tris > h->surfTriCap) {
        h->surfTriCap = 0;
        HIPCHK(h, h->surfTrisDev.alloc(tris * 3));
        HIPCHK(h, h->surfTrisHost.alloc(tris * 3));
        h->surfTriCap = tris;
    }
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_extract_surface(sph_handle *h, const SphSurfaceOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the surface mesh", ": multi-GPU runs are not meshed");
    if (rc) return rc;
    const char *unset = "SphSurfaceOptions.struct_size is not set";
    if (!opt) return fail(h, SPH_EINVAL, unset); // (no defaults: a lattice and a level have to be given)
    SphSurfaceOptions o{};
    if ((rc = copy_options(h, opt, o, unset))) return rc;
    if (const char *bad = bad_lattice(o.nx, o.ny, o.nz, o.origin, o.spacing, 2)) return fail(h, SPH_EINVAL, bad);
    if (!std::isfinite(o.iso) || !(o.iso > 0.f)) return fail(h, SPH_EINVAL, "iso must be finite and > 0");
    const bool plain = plain_path("SPH_SURFACE_PLAIN");
    SurfaceArgs S{};
    S.nx = o.nx, S.ny = o.ny, S.nz = o.nz;
    S.ox = o.origin[0], S.oy = o.origin[1], S.oz = o.origin[2];
    S.sx = o.spacing[0], S.sy = o.spacing[1], S.sz = o.spacing[2];
    S.iso = o.iso;
    const size_t points = (size_t)o.nx * o.ny * o.nz;
    if ((rc = surface_reserve_lattice(h, points, (size_t)sph_surface_blocks(S)))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    if ((rc = outbound_fence(h, h->surf.out))) return rc; // the previous mesh's copy still reads the device buffers
    h->surf.valid = false;

    const SampleArgs A = lattice_args(h, o.nx, o.ny, o.nz, o.origin, o.spacing, SPH_FIELD_DENSITY);
    if ((rc = timed_launch(h, &h->surfSampleSeconds, [&] { sph_launch_sample(h->P, A, plain, h->surfField, h->compute); }))) return rc;
    SurfaceBuffers B{};
    B.field = h->surfField, B.bits = h->surfBits, B.local = h->surfLocal;
    B.blockSum = h->surfBlockSum, B.blockOff = h->surfBlockOff, B.totals = h->surfTotalsDev;
    if ((rc = timed_launch(h, &h->surf.seconds, [&] { sph_launch_surface_count(S, plain, B, h->compute); }))) return rc;
    // the one wait of this call: the two totals size the mesh
    if ((rc = fetch_small(h, h->surfTotalsHost.get(), h->surfTotalsDev.get(), 2 * sizeof(unsigned long long), h->surfCounted))) return rc;
    const size_t verts = (size_t)h->surfTotalsHost[0], tris = (size_t)h->surfTotalsHost[1];
    h->surf.calls += 1;
    (plain ? h->surfPlainCalls : h->surfWaveCalls) += 1;
    if (verts > 0 || tris > 0) {
        if ((rc = surface_reserve_mesh(h, verts, tris))) return rc;
        if ((rc = timed_launch(h, &h->surf.seconds, [&] { sph_launch_surface_emit(S, plain, B, h->surfVertsDev, h->surfTrisDev, h->compute); })))
            return rc;
        if ((rc = outbound_send(h, h->surf.out, {{h->surfVertsHost.get(), h->surfVertsDev.get(), verts * 3 * sizeof(float)},
                                                 {h->surfTrisHost.get(), h->surfTrisDev.get(), tris * 3 * sizeof(uint32_t)}})))
            return rc;
    }
    h->surfVerts = (long long)verts, h->surfTris = (long long)tris;
    h->surf.valid = true;
    return SPH_OK;
}

int sph_surface_host(sph_handle *h, const float **vertices_xyz, int64_t *num_vertices, const uint32_t **triangles, int64_t *num_triangles) {
    if (!h) return SPH_EINVAL;
    if (!h->surf.valid) return fail(h, SPH_ESTATE, "sph_extract_surface must come first");
    if (outbound_wait(h->surf.out) != hipSuccess) return fail(h, SPH_EHIP, "surface copy failed");
    if (vertices_xyz) *vertices_xyz = h->surfVerts ? h->surfVertsHost.get() : nullptr;
    if (num_vertices) *num_vertices = h->surfVerts;
    if (triangles) *triangles = h->surfTris ? h->surfTrisHost.get() : nullptr;
    if (num_triangles) *num_triangles = h->surfTris;
    return SPH_OK;
}

int sph_get_surface_time(sph_handle *h, double *sample_seconds, double *extract_seconds, int64_t *calls, int reset) {
    if (!h) return SPH_EINVAL;
    long long unused = 0;
    int rc = timed_total(h, &h->surfSampleSeconds, &unused, sample_seconds, nullptr, reset);
    if (rc) return rc;
    return timed_total(h, &h->surf.seconds, &h->surf.calls, extract_seconds, calls, reset);
}

} // extern "C"
