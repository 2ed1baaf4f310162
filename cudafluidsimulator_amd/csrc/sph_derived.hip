// Derived per-particle fields: sph_derive and what reads its results (kernels: derived.hip).
#include "sph_handle.h"

using namespace sph_host;

namespace {

// (re)allocate the result buffers for n particles
int derive_reserve(sph_handle *h, size_t n) {
    if (n <= h->deriveCap) return SPH_OK;
    int rc = pass_quiesce(h, h->derive); // the old buffers may still be written by a queued sweep or read by a queued copy
    if (rc) return rc;
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

} // namespace

extern "C" {

int sph_derive(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the derived fields' sweep", ": multi-GPU runs derive no fields");
    if (rc) return rc;
    const int n = h->n;
    if (n == 0) { // nothing to sweep, nothing to copy
        if ((rc = outbound_fence(h, h->derive.out))) return rc;
        h->deriveN = 0;
        h->derive.valid = true;
        return SPH_OK;
    }
    if ((rc = derive_reserve(h, (size_t)n))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    const bool plain = plain_path("SPH_DERIVE_PLAIN");
    if (!plain && (rc = h->deriveCounters.ensure(h))) return rc;
    if ((rc = outbound_fence(h, h->derive.out))) return rc; // the previous derive's copies still read the device buffers
    DeriveArgs A{};
    A.S = sorted_stream(h);
    A.vortDiv = h->deriveVortDiv;
    A.gradRho = h->deriveGradRho;
    A.neighbours = h->deriveNeighbours;
    A.counters = h->deriveCounters.dev;
    if ((rc = timed_launch(h, &h->derive.seconds, [&] { sph_launch_derive(h->P, A, plain, h->compute); }))) return rc;
    h->derive.calls += 1;
    h->derive.valid = false; // (until the copies are queued: the pinned buffers still hold the previous results)
    if ((rc = outbound_send(h, h->derive.out, {{h->deriveVortDivHost.get(), h->deriveVortDiv.get(), (size_t)n * sizeof(float4)},
                                              {h->deriveGradRhoHost.get(), h->deriveGradRho.get(), (size_t)n * sizeof(float4)},
                                              {h->deriveNeighboursHost.get(), h->deriveNeighbours.get(), (size_t)n * sizeof(uint32_t)}})))
        return rc;
    h->deriveN = n;
    h->derive.valid = true;
    return SPH_OK;
}

int sph_derived_host(sph_handle *h, const float **vort_div, const float **grad_rho, const uint32_t **neighbours, int *n) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->derive.valid) return fail(h, SPH_ESTATE, "sph_derive must come first");
    HIPCHK(h, outbound_wait(h->derive.out));
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
    int rc = timed_total(h, &h->derive.seconds, &h->derive.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if ((rc = h->deriveCounters.read(h, reset))) return rc;
    if (const unsigned long long *c = h->deriveCounters.host) S.runs_staged = c[0], S.runs_direct = c[1];
    *out = S;
    return SPH_OK;
}

} // extern "C"
