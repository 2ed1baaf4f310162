// The surface mesh: sph_extract_surface and what reads its results (kernels: sample.hip for the field, surface.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

// nothing queued reads or writes the surface's buffers any more
int surface_quiesce(sph_handle *h) {
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->surfOut.pending = false;
    h->surfValid = false;
    return SPH_OK;
}

int surface_reserve_lattice(sph_handle *h, size_t points, size_t blocks) {
    if (points > h->surfPointCap || blocks > h->surfBlockCap || !h->surfTotalsDev) {
        int rc = surface_quiesce(h);
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
        HIPCHK(h, h->surfCounted.create(hipEventDisableTiming));
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

const char *bad_surface(const SphSurfaceOptions &o) {
    for (int d : {o.nx, o.ny, o.nz})
        if (d < 2 || d > 4096) return "lattice dimensions must be 2..4096";
    if ((long long)o.nx * o.ny * o.nz > (1ll << 24)) return "lattice holds more than 1 << 24 points";
    for (float v : o.origin)
        if (!std::isfinite(v)) return "origin must be finite";
    for (float s : o.spacing)
        if (!std::isfinite(s) || !(s > 0.f)) return "spacing must be finite and > 0";
    if (!std::isfinite(o.iso) || !(o.iso > 0.f)) return "iso must be finite and > 0";
    return nullptr;
}

} // namespace

extern "C" {

int sph_extract_surface(sph_handle *h, const SphSurfaceOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU runs are not meshed");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    if (h->opt.sweep == SPH_SWEEP_LINKED) return fail(h, SPH_ESTATE, "the surface mesh needs a cell table: not available with SPH_SWEEP_LINKED");
    if (h->P.morton) return fail(h, SPH_ESTATE, "the surface mesh walks rows of cells as runs of the stream: not available with SPH_KEY_MORTON");
    if (h->phase != 0 && h->phase != 1) return fail(h, SPH_ESTATE, "a step split into phases is still open");
    const char *unset = "SphSurfaceOptions.struct_size is not set";
    if (!opt) return fail(h, SPH_EINVAL, unset); // (no defaults: a lattice and a level have to be given)
    SphSurfaceOptions o{};
    int rc = copy_options(h, opt, o, unset);
    if (rc) return rc;
    if (const char *bad = bad_surface(o)) return fail(h, SPH_EINVAL, bad);
    const bool plain = plain_path("SPH_SURFACE_PLAIN");
    SurfaceArgs S{};
    S.nx = o.nx, S.ny = o.ny, S.nz = o.nz;
    S.ox = o.origin[0], S.oy = o.origin[1], S.oz = o.origin[2];
    S.sx = o.spacing[0], S.sy = o.spacing[1], S.sz = o.spacing[2];
    S.iso = o.iso;
    const size_t points = (size_t)o.nx * o.ny * o.nz;
    if ((rc = surface_reserve_lattice(h, points, (size_t)sph_surface_blocks(S)))) return rc;
    // the grid of the state the handle holds NOW, as sph_sample_field finds or builds it
    if (h->phase == 0 && h->n > 0 && (rc = build_grid_ahead(h))) return rc;
    if ((rc = outbound_fence(h, h->surfOut))) return rc; // the previous mesh's copy still reads the device buffers
    h->surfValid = false;

    SampleArgs A{};
    A.nx = o.nx, A.ny = o.ny, A.nz = o.nz;
    A.ox = S.ox, A.oy = S.oy, A.oz = S.oz;
    A.sx = S.sx, A.sy = S.sy, A.sz = S.sz;
    A.field = SPH_FIELD_DENSITY;
    A.n = h->n;
    if (h->n > 0) {
        A.cellRange = h->cellRange;
        if (h->opt.sweep == SPH_SWEEP_LIST && h->pv8) { // the gather left no sorted vel4 in this mode
            A.pos = h->pv8;
            A.vel = h->pv8 + 1;
            A.stride = 2;
        } else {
            A.pos = h->pos4[h->sorted];
            A.vel = h->vel4[h->sorted];
            A.stride = 1;
        }
    }
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->surfSampleSeconds, &pe))) return rc;
    sph_launch_sample(h->P, A, plain, h->surfField, h->compute);
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());

    SurfaceBuffers B{};
    B.field = h->surfField, B.bits = h->surfBits, B.local = h->surfLocal;
    B.blockSum = h->surfBlockSum, B.blockOff = h->surfBlockOff, B.totals = h->surfTotalsDev;
    if ((rc = pair_begin(h, &h->surfExtractSeconds, &pe))) return rc;
    sph_launch_surface_count(S, plain, B, h->compute);
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    // the one wait of this call: the two totals size the mesh
    HIPCHK(h, hipMemcpyAsync(h->surfTotalsHost.get(), h->surfTotalsDev.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->compute));
    HIPCHK(h, hipEventRecord(h->surfCounted, h->compute));
    HIPCHK(h, hipEventSynchronize(h->surfCounted));
    const size_t verts = (size_t)h->surfTotalsHost[0], tris = (size_t)h->surfTotalsHost[1];
    h->surfCount += 1;
    (plain ? h->surfPlainCalls : h->surfWaveCalls) += 1;
    if (verts > 0 || tris > 0) {
        if ((rc = surface_reserve_mesh(h, verts, tris))) return rc;
        if ((rc = pair_begin(h, &h->surfExtractSeconds, &pe))) return rc;
        sph_launch_surface_emit(S, plain, B, h->surfVertsDev, h->surfTrisDev, h->compute);
        HIPCHK(h, hipEventRecord(pe->b, h->compute));
        HIPCHK(h, hipGetLastError());
        if ((rc = outbound_send(h, h->surfOut, {{h->surfVertsHost.get(), h->surfVertsDev.get(), verts * 3 * sizeof(float)},
                                                {h->surfTrisHost.get(), h->surfTrisDev.get(), tris * 3 * sizeof(uint32_t)}})))
            return rc;
    }
    h->surfVerts = (long long)verts, h->surfTris = (long long)tris;
    h->surfValid = true;
    return SPH_OK;
}

int sph_surface_host(sph_handle *h, const float **vertices_xyz, int64_t *num_vertices, const uint32_t **triangles, int64_t *num_triangles) {
    if (!h) return SPH_EINVAL;
    if (!h->surfValid) return fail(h, SPH_ESTATE, "sph_extract_surface must come first");
    if (outbound_wait(h->surfOut) != hipSuccess) return fail(h, SPH_EHIP, "surface copy failed");
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
    return timed_total(h, &h->surfExtractSeconds, &h->surfCount, extract_seconds, calls, reset);
}

} // extern "C"
