// Pair statistics: sph_pair_statistics and what reads its results (kernels: pairs.hip; the pure host functions:
// sph_pair_values.cpp).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

constexpr int kDefaultBins = 32;

// the fixed-size buffers, by the first call; the partial rows for `rows` workgroups of `bins` bins
int pair_reserve(sph_handle *h, int rows, int bins) {
    if (!h->pairRows) {
        HIPCHK(h, h->pairEdges.alloc(SPH_PAIR_MAX_BINS));
        HIPCHK(h, h->pairEdgesHost.alloc(SPH_PAIR_MAX_BINS));
        HIPCHK(h, h->pairRows.alloc(SPH_PAIR_MAX_BINS));
        HIPCHK(h, h->pairRowsHost.alloc(SPH_PAIR_MAX_BINS));
        HIPCHK(h, h->pairTile.alloc(1));
        HIPCHK(h, hipDeviceGetAttribute(&h->pairCUs, hipDeviceAttributeMultiprocessorCount, h->device));
    }
    const size_t words = (size_t)rows * kPairWords * (size_t)bins;
    if (words <= h->pairPartialCap) return SPH_OK;
    int rc = pass_quiesce(h, h->pair); // a queued join may still read the old rows
    if (rc) return rc;
    h->pairPartialCap = 0;
    HIPCHK(h, h->pairPartials.alloc(words));
    h->pairPartialCap = words;
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_pair_statistics(sph_handle *h, const SphPairOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the pair statistics' sweep", ": multi-GPU runs gather no pair statistics (pairs cross slab boundaries)");
    if (rc) return rc;
    SphPairOptions o{};
    if ((rc = copy_options(h, opt, o, "SphPairOptions.struct_size is not set"))) return rc;
    if (o.flags != 0) return fail(h, SPH_EINVAL, "SphPairOptions.flags: no flag is defined");
    if (o.pad_ != 0) return fail(h, SPH_EINVAL, "SphPairOptions.pad_ must be 0");
    if (o.bins < 0 || o.bins > SPH_PAIR_MAX_BINS) return fail(h, SPH_EINVAL, "bins must be 0 (= 32) or 1 .. 128");
    if (!std::isfinite(o.radius) || o.radius < 0.f || o.radius > h->P.h)
        return fail(h, SPH_EINVAL, "radius must be 0 (= h) or finite with 0 < radius <= h");
    const float radius = o.radius == 0.f ? h->P.h : o.radius;
    const int bins = o.bins ? o.bins : kDefaultBins;
    const int n = h->n;
    const bool plain = plain_path("SPH_PAIRS_PLAIN");
    if (!plain && n > kPairMaxN)
        return fail(h, SPH_EINVAL, "sph_pair_statistics: " + std::to_string(n) + " particles, more than the " + std::to_string(kPairMaxN) +
                                       " up to which no accumulator of the default path can wrap");
    PairEdges E{};
    if (sph_pair_edges(radius, h->P.h, bins, E.e) != SPH_OK) return fail(h, SPH_EINVAL, "sph_pair_edges refused the radius");
    if (!h->pairRows && (rc = pair_reserve(h, 0, bins))) return rc; // (the CU count sizes the launch)
    const int wanted = call_knob("SPH_PAIRS_WORKGROUPS");
    const int rows = sph_pair_rows(n, h->pairCUs, plain, wanted > 0 && wanted <= (1 << 16) ? wanted : 0);
    const int shedBits = call_knob("SPH_PAIRS_SHED_BITS");
    if ((rc = pair_reserve(h, rows, bins))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    if ((rc = h->pairCounters.ensure(h))) return rc;
    if ((rc = outbound_fence(h, h->pair.out))) return rc; // the previous call's copies still read the device buffers
    h->pair.valid = false;
    PairArgs A{};
    A.S = sorted_stream(h);
    A.r2 = radius * radius;
    A.perRadius = (float)bins / radius;
    A.bins = bins;
    A.edges2 = h->pairEdges;
    A.partials = h->pairPartials;
    A.rows = rows;
    A.tile = h->pairTile;
    A.shed = 1ll << (shedBits >= 33 && shedBits <= 62 ? shedBits : 62);
    A.out = h->pairRows;
    A.counters = h->pairCounters.dev;
    sph_launch_pair_table(E, A, h->compute);
    HIPCHK(h, hipGetLastError());
    if (n > 0) {
        if ((rc = timed_launch(h, &h->pair.seconds, [&] { sph_launch_pair_statistics(h->P, A, plain, h->compute); }))) return rc;
        h->pair.calls += 1;
    }
    if ((rc = outbound_send(h, h->pair.out, {{h->pairRowsHost.get(), h->pairRows.get(), (size_t)bins * sizeof(SphPairBinRaw)},
                                             {h->pairEdgesHost.get(), h->pairEdges.get(), (size_t)bins * sizeof(float)}})))
        return rc;
    h->pairBins = bins;
    h->pair.valid = true;
    return SPH_OK;
}

int sph_pair_statistics_host(sph_handle *h, const SphPairBinRaw **rows, const float **edges2, int *bins) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->pair.valid) return fail(h, SPH_ESTATE, "sph_pair_statistics must come first");
    HIPCHK(h, outbound_wait(h->pair.out));
    if (rows) *rows = h->pairRowsHost.get();
    if (edges2) *edges2 = h->pairEdgesHost.get();
    if (bins) *bins = h->pairBins;
    return SPH_OK;
}

int sph_get_pair_stats(sph_handle *h, SphPairStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphPairStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->pair.seconds, &h->pair.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if ((rc = h->pairCounters.read(h, reset))) return rc;
    if (const unsigned long long *c = h->pairCounters.host) S.runs_staged = c[0], S.runs_direct = c[1], S.pairs = c[2];
    *out = S;
    return SPH_OK;
}

} // extern "C"
