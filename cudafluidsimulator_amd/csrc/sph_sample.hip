// The field sample: sph_sample_field and what reads its results (kernels: sample.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace sph_host {

const char *bad_lattice(int nx, int ny, int nz, const float (&origin)[3], const float (&spacing)[3], int minDim) {
    for (int d : {nx, ny, nz})
        if (d < minDim || d > 4096) return minDim == 1 ? "lattice dimensions must be 1..4096" : "lattice dimensions must be 2..4096";
    if ((long long)nx * ny * nz > (1ll << 24)) return "lattice holds more than 1 << 24 points";
    for (float o : origin)
        if (!std::isfinite(o)) return "origin must be finite";
    for (float s : spacing)
        if (!std::isfinite(s) || !(s > 0.f)) return "spacing must be finite and > 0";
    return nullptr;
}

SampleArgs lattice_args(const sph_handle *h, int nx, int ny, int nz, const float (&origin)[3], const float (&spacing)[3], int field) {
    SampleArgs A{};
    A.nx = nx, A.ny = ny, A.nz = nz;
    A.ox = origin[0], A.oy = origin[1], A.oz = origin[2];
    A.sx = spacing[0], A.sy = spacing[1], A.sz = spacing[2];
    A.field = field;
    A.S = sorted_stream(h);
    return A;
}

} // namespace sph_host

namespace {

// (re)allocate the value buffers for `points` floats
int sample_reserve(sph_handle *h, size_t points) {
    if (points <= h->sampleCap) return SPH_OK;
    int rc = pass_quiesce(h, h->sample); // the old buffers may still be read by a queued copy
    if (rc) return rc;
    h->sampleCap = 0;
    HIPCHK(h, h->sampleDev.alloc(points));
    HIPCHK(h, h->sampleHost.alloc(points));
    h->sampleCap = points;
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_sample_field(sph_handle *h, const SphSampleLattice *lat) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the field sample", ": multi-GPU runs are not sampled");
    if (rc) return rc;
    const char *unset = "SphSampleLattice.struct_size is not set";
    if (!lat) return fail(h, SPH_EINVAL, unset); // (no defaults: a lattice has to be given)
    SphSampleLattice L{};
    if ((rc = copy_options(h, lat, L, unset))) return rc;
    if (const char *bad = bad_lattice(L.nx, L.ny, L.nz, L.origin, L.spacing, 1)) return fail(h, SPH_EINVAL, bad);
    if (bad_field(L.field)) return fail(h, SPH_EINVAL, "unknown field");
    const size_t points = (size_t)L.nx * L.ny * L.nz;
    if ((rc = sample_reserve(h, points))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    const bool plain = plain_path("SPH_SAMPLE_PLAIN");
    if ((rc = outbound_fence(h, h->sample.out))) return rc; // the previous sample's copy still reads the device buffer
    const SampleArgs A = lattice_args(h, L.nx, L.ny, L.nz, L.origin, L.spacing, L.field);
    if ((rc = timed_launch(h, &h->sample.seconds, [&] { sph_launch_sample(h->P, A, plain, h->sampleDev, h->compute); }))) return rc;
    h->sample.calls += 1;
    (plain ? h->samplePlainCalls : h->sampleTileCalls) += 1;
    h->sample.valid = false; // (until the copy is queued: the pinned buffer still holds the previous sample)
    if ((rc = outbound_send(h, h->sample.out, {{h->sampleHost.get(), h->sampleDev.get(), points * sizeof(float)}}))) return rc;
    h->sampleDim[0] = L.nx, h->sampleDim[1] = L.ny, h->sampleDim[2] = L.nz;
    h->sample.valid = true;
    return SPH_OK;
}

const float *sph_sample_host(sph_handle *h, int *nx, int *ny, int *nz) {
    if (!h) return nullptr;
    if (!h->sample.valid) {
        h->err = "sph_sample_field must come first";
        return nullptr;
    }
    if (outbound_wait(h->sample.out) != hipSuccess) {
        h->err = "sample copy failed";
        return nullptr;
    }
    if (nx) *nx = h->sampleDim[0];
    if (ny) *ny = h->sampleDim[1];
    if (nz) *nz = h->sampleDim[2];
    return h->sampleHost;
}

int sph_get_sample_time(sph_handle *h, double *seconds, int64_t *samples, int reset) {
    if (!h) return SPH_EINVAL;
    return timed_total(h, &h->sample.seconds, &h->sample.calls, seconds, samples, reset);
}

} // extern "C"
