// The field sample: sph_sample_field and what reads its results (kernels: sample.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

// (re)allocate the value buffers for `points` floats
int sample_reserve(sph_handle *h, size_t points) {
    if (points <= h->sampleCap) return SPH_OK;
    // the old buffers may still be read by a queued copy
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->sampleOut.pending = false;
    h->sampleValid = false;
    h->sampleCap = 0;
    HIPCHK(h, h->sampleDev.alloc(points));
    HIPCHK(h, h->sampleHost.alloc(points));
    h->sampleCap = points;
    return SPH_OK;
}

const char *bad_lattice(const SphSampleLattice &L) {
    for (int d : {L.nx, L.ny, L.nz})
        if (d < 1 || d > 4096) return "lattice dimensions must be 1..4096";
    if ((long long)L.nx * L.ny * L.nz > (1ll << 24)) return "lattice holds more than 1 << 24 points";
    for (float o : L.origin)
        if (!std::isfinite(o)) return "origin must be finite";
    for (float s : L.spacing)
        if (!std::isfinite(s) || !(s > 0.f)) return "spacing must be finite and > 0";
    if (bad_field(L.field)) return "unknown field";
    return nullptr;
}

} // namespace

extern "C" {

int sph_sample_field(sph_handle *h, const SphSampleLattice *lat) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU runs are not sampled");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    if (h->opt.sweep == SPH_SWEEP_LINKED) return fail(h, SPH_ESTATE, "the field sample needs a cell table: not available with SPH_SWEEP_LINKED");
    if (h->P.morton) return fail(h, SPH_ESTATE, "the field sample walks rows of cells as runs of the stream: not available with SPH_KEY_MORTON");
    if (h->phase != 0 && h->phase != 1) return fail(h, SPH_ESTATE, "a step split into phases is still open");
    const char *unset = "SphSampleLattice.struct_size is not set";
    if (!lat) return fail(h, SPH_EINVAL, unset); // (no defaults: a lattice has to be given)
    SphSampleLattice L{};
    int rc = copy_options(h, lat, L, unset);
    if (rc) return rc;
    if (const char *bad = bad_lattice(L)) return fail(h, SPH_EINVAL, bad);
    const size_t points = (size_t)L.nx * L.ny * L.nz;
    if ((rc = sample_reserve(h, points))) return rc;
    // A grid of the state the handle holds NOW.  Phase 1: it exists (sph_phase_grid, or built ahead by a timed
    // step).  Phase 0: the table of the last step is the pre-integration one; the next step's grid is built
    // here, ahead, and that step consumes it.
    if (h->phase == 0 && h->n > 0 && (rc = build_grid_ahead(h))) return rc;
    const bool plain = plain_path("SPH_SAMPLE_PLAIN");
    if ((rc = outbound_fence(h, h->sampleOut))) return rc; // the previous sample's copy still reads the device buffer
    SampleArgs A{};
    A.nx = L.nx, A.ny = L.ny, A.nz = L.nz;
    A.ox = L.origin[0], A.oy = L.origin[1], A.oz = L.origin[2];
    A.sx = L.spacing[0], A.sy = L.spacing[1], A.sz = L.spacing[2];
    A.field = L.field;
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
    if ((rc = pair_begin(h, &h->sampleSeconds, &pe))) return rc;
    sph_launch_sample(h->P, A, plain, h->sampleDev, h->compute);
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    h->sampleCount += 1;
    (plain ? h->samplePlainCalls : h->sampleTileCalls) += 1;
    h->sampleValid = false; // (until the copy is queued: the pinned buffer still holds the previous sample)
    if ((rc = outbound_send(h, h->sampleOut, {{h->sampleHost.get(), h->sampleDev.get(), points * sizeof(float)}}))) return rc;
    h->sampleDim[0] = L.nx, h->sampleDim[1] = L.ny, h->sampleDim[2] = L.nz;
    h->sampleValid = true;
    return SPH_OK;
}

const float *sph_sample_host(sph_handle *h, int *nx, int *ny, int *nz) {
    if (!h) return nullptr;
    if (!h->sampleValid) {
        h->err = "sph_sample_field must come first";
        return nullptr;
    }
    if (outbound_wait(h->sampleOut) != hipSuccess) {
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
    return timed_total(h, &h->sampleSeconds, &h->sampleCount, seconds, samples, reset);
}

} // extern "C"
