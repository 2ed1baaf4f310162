// Derived per-particle fields: sph_derive and what reads its results (kernels: derived.hip).
#include "sph_handle.h"

using namespace sph_host;

namespace {

// (re)allocate the result buffers for n particles
int derive_reserve(sph_handle *h, size_t n) {
    if (n <= h->deriveCap) return SPH_OK;
    // the old buffers may still be written by a queued sweep or read by a queued copy
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->deriveOut.pending = false;
    h->deriveValid = false;
    h->deriveCap = 0;
    HIPCHK(h, h->deriveVortDiv.alloc(n));
    HIPCHK(h, h->deriveGradRho.alloc(n));
    HIPCHK(h, h->deriveNeighbours.alloc(n));
    HIPCHK(h, h->deriveVortDivHost.alloc(n));
    HIPCHK(h, h->deriveGradRhoHost.alloc(n));
    HIPCHK(h, h->deriveNeighboursHost.alloc(n));
    h->deriveCap = n;
    return SPH_OK;
}

int derive_counters(sph_handle *h) {
    if (h->deriveCounters) return SPH_OK;
    HIPCHK(h, h->deriveCounters.alloc(kDeriveCounters));
    HIPCHK(h, h->deriveCountersHost.alloc(kDeriveCounters));
    HIPCHK(h, hipMemsetAsync(h->deriveCounters, 0, kDeriveCounters * sizeof(unsigned long long), h->compute));
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_derive(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU runs derive no fields");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    if (h->opt.sweep == SPH_SWEEP_LINKED) return fail(h, SPH_ESTATE, "the derived fields need a cell table: not available with SPH_SWEEP_LINKED");
    if (h->P.morton) return fail(h, SPH_ESTATE, "the derived fields walk rows of cells as runs of the stream: not available with SPH_KEY_MORTON");
    if (h->phase != 0 && h->phase != 1) return fail(h, SPH_ESTATE, "a step split into phases is still open");
    const int n = h->n;
    int rc;
    if (n == 0) { // nothing to sweep, nothing to copy
        if ((rc = outbound_fence(h, h->deriveOut))) return rc;
        h->deriveN = 0;
        h->deriveValid = true;
        return SPH_OK;
    }
    if ((rc = derive_reserve(h, (size_t)n))) return rc;
    // a grid of the state the handle holds NOW, found or built ahead exactly as sph_tracers_advect does
    if (h->phase == 0 && (rc = build_grid_ahead(h))) return rc;
    const bool plain = plain_path("SPH_DERIVE_PLAIN");
    if (!plain && (rc = derive_counters(h))) return rc;
    if ((rc = outbound_fence(h, h->deriveOut))) return rc; // the previous derive's copies still read the device buffers
    DeriveArgs A{};
    A.n = n;
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
    A.vortDiv = h->deriveVortDiv;
    A.gradRho = h->deriveGradRho;
    A.neighbours = h->deriveNeighbours;
    A.counters = h->deriveCounters;
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->deriveSeconds, &pe))) return rc;
    sph_launch_derive(h->P, A, plain, h->compute);
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    h->deriveCalls += 1;
    h->deriveValid = false; // (until the copies are queued: the pinned buffers still hold the previous results)
    if ((rc = outbound_send(h, h->deriveOut, {{h->deriveVortDivHost.get(), h->deriveVortDiv.get(), (size_t)n * sizeof(float4)},
                                              {h->deriveGradRhoHost.get(), h->deriveGradRho.get(), (size_t)n * sizeof(float4)},
                                              {h->deriveNeighboursHost.get(), h->deriveNeighbours.get(), (size_t)n * sizeof(uint32_t)}})))
        return rc;
    h->deriveN = n;
    h->deriveValid = true;
    return SPH_OK;
}

int sph_derived_host(sph_handle *h, const float **vort_div, const float **grad_rho, const uint32_t **neighbours, int *n) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->deriveValid) return fail(h, SPH_ESTATE, "sph_derive must come first");
    HIPCHK(h, outbound_wait(h->deriveOut));
    const bool any = h->deriveN > 0;
    if (vort_div) *vort_div = any ? &h->deriveVortDivHost.get()->x : nullptr;
    if (grad_rho) *grad_rho = any ? &h->deriveGradRhoHost.get()->x : nullptr;
    if (neighbours) *neighbours = any ? h->deriveNeighboursHost.get() : nullptr;
    if (n) *n = h->deriveN;
    return SPH_OK;
}

int sph_get_derive_stats(sph_handle *h, SphDeriveStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphDeriveStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->deriveSeconds, &h->deriveCalls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if (h->deriveCounters) {
        HIPCHK(h, hipMemcpyAsync(h->deriveCountersHost, h->deriveCounters, kDeriveCounters * sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, h->compute));
        if (reset) HIPCHK(h, hipMemsetAsync(h->deriveCounters, 0, kDeriveCounters * sizeof(unsigned long long), h->compute));
        HIPCHK(h, hipStreamSynchronize(h->compute));
        S.runs_staged = h->deriveCountersHost[0];
        S.runs_direct = h->deriveCountersHost[1];
    }
    *out = S;
    return SPH_OK;
}

} // extern "C"
