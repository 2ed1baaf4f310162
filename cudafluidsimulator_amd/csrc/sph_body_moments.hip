// Per-body moments: sph_measure_bodies and what reads its results (kernels: body_moments.hip; the labelling:
// label_bodies in sph_bodies.hip; the derived values: sph_body_values.cpp).
#include "sph_handle.h"

using namespace sph_host;

namespace {

constexpr size_t kRowBytes = (size_t)kBodyMomentStride * sizeof(unsigned long long);
static_assert(kRowBytes == sizeof(SphBodyMomentsRaw), "the pinned rows are handed out as SphBodyMomentsRaw");

// the bins, with the first call; the rows, (re)allocated for `bodies` of them
int moment_reserve(sph_handle *h, size_t bodies) {
    if (!h->momentHist) {
        HIPCHK(h, h->momentHist.alloc(SPH_BODY_SIZE_BINS));
        HIPCHK(h, h->momentHistHost.alloc(SPH_BODY_SIZE_BINS));
    }
    if (bodies <= h->momentCap) return SPH_OK;
    int rc = pass_quiesce(h, h->moment);
    if (rc) return rc;
    h->momentCap = 0;
    HIPCHK(h, h->momentRows.alloc(bodies * kBodyMomentStride));
    HIPCHK(h, h->momentRowsHost.alloc(bodies * kBodyMomentStride));
    h->momentCap = bodies;
    return SPH_OK;
}

} // namespace

namespace sph_host {

int measure_labelled(sph_handle *h, uint32_t max_bodies, const char *who) {
    int rc;
    const int n = h->bodyN;
    const size_t bodies = (size_t)h->bodyCount;
    if (max_bodies && bodies > (size_t)max_bodies) {
        h->moment.valid = false;
        return fail(h, SPH_ENOMEM, std::string(who) + ": the state has " + std::to_string(bodies) + " bodies, more than max_bodies = " +
                                       std::to_string(max_bodies) + "; no moments");
    }
    if ((rc = moment_reserve(h, bodies))) return rc;
    if ((rc = outbound_fence(h, h->moment.out))) return rc; // the previous call's copies still read the device buffers
    h->moment.valid = false;
    BodyMomentArgs A{};
    A.S = sorted_stream(h);
    A.rowLabel = h->bodyRowLabel, A.rank = h->bodyRank, A.table = h->bodyTable;
    A.numBodies = (int)bodies;
    A.rows = h->momentRows, A.sizeHist = h->momentHist;
    const bool plain = plain_path("SPH_BODIES_PLAIN");
    if ((rc = timed_launch(h, &h->moment.seconds, [&] { sph_launch_body_moments(A, plain, h->compute); }))) return rc;
    if (bodies > 0)
        rc = outbound_send(h, h->moment.out, {{h->momentRowsHost.get(), h->momentRows.get(), bodies * kRowBytes},
                                              {h->momentHistHost.get(), h->momentHist.get(), SPH_BODY_SIZE_BINS * sizeof(uint32_t)}});
    else
        rc = outbound_send(h, h->moment.out, {{h->momentHistHost.get(), h->momentHist.get(), SPH_BODY_SIZE_BINS * sizeof(uint32_t)}});
    if (rc) return rc;
    if (n > 0) h->moment.calls += 1;
    h->momentCount = (int)bodies;
    h->moment.valid = true;
    return SPH_OK;
}

} // namespace sph_host

extern "C" {

int sph_measure_bodies(sph_handle *h, const SphBodyMeasureOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the bodies' labelling", ": multi-GPU runs label no bodies");
    if (rc) return rc;
    SphBodyMeasureOptions o{};
    if ((rc = copy_options(h, opt, o, "SphBodyMeasureOptions.struct_size is not set"))) return rc;
    if (o.pad_ != 0) return fail(h, SPH_EINVAL, "SphBodyMeasureOptions.pad_ must be 0");
    if ((rc = label_bodies(h, o.link, "sph_measure_bodies"))) return rc;
    // the labelling stands from here on, whatever becomes of the moments
    return measure_labelled(h, o.max_bodies, "sph_measure_bodies");
}

int sph_body_moments_host(sph_handle *h, const SphBodyMomentsRaw **rows, int *num_bodies, const uint32_t **size_hist) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->moment.valid) return fail(h, SPH_ESTATE, "sph_measure_bodies must come first");
    HIPCHK(h, outbound_wait(h->moment.out));
    if (rows) *rows = h->momentCount > 0 ? reinterpret_cast<const SphBodyMomentsRaw *>(h->momentRowsHost.get()) : nullptr;
    if (num_bodies) *num_bodies = h->momentCount;
    if (size_hist) *size_hist = h->momentHistHost.get();
    return SPH_OK;
}

int sph_get_body_measure_stats(sph_handle *h, SphBodyMeasureStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphBodyMeasureStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->moment.seconds, &h->moment.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    *out = S;
    return SPH_OK;
}

} // extern "C"
