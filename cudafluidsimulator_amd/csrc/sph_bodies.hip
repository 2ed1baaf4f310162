// Bodies: sph_label_bodies and what reads its results (kernels: bodies.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

// (re)allocate the per-row and per-id buffers for n particles
int body_reserve(sph_handle *h, size_t n) {
    if (!h->bodyCounters) {
        HIPCHK(h, h->bodyCounters.alloc(1));
        HIPCHK(h, h->bodyCountersHost.alloc(1));
        HIPCHK(h, h->bodyFinalHost.alloc(1));
    }
    if (n <= h->bodyCap) return SPH_OK;
    int rc = pass_quiesce(h, h->body);
    if (rc) return rc;
    h->bodyCap = 0;
    for (auto *b : {&h->bodyParent, &h->bodyRoot, &h->bodyRootId, &h->bodyRowLabel, &h->bodyFlag, &h->bodyRank, &h->bodyLabels})
        HIPCHK(h, b->alloc(n));
    HIPCHK(h, h->bodyBlockSum.alloc((size_t)sph_body_scan_blocks((int)n)));
    HIPCHK(h, h->bodyLabelsHost.alloc(n));
    h->bodyCap = n;
    return SPH_OK;
}

// (the compute stream is idle here: the host has just waited for the number of bodies)
int body_reserve_table(sph_handle *h, size_t bodies) {
    if (bodies <= h->bodyTableCap) return SPH_OK;
    HIPCHK(h, hipStreamSynchronize(h->copy)); // the last table may still be on its way out of the old buffer
    h->body.out.pending = false;
    h->bodyTableCap = 0;
    HIPCHK(h, h->bodyTable.alloc(bodies * 8));
    HIPCHK(h, h->bodyTableHost.alloc(bodies * 8));
    h->bodyTableCap = bodies;
    return SPH_OK;
}

// the counter block to pinned memory, and the one wait of the call (the check path: one per round)
int body_fetch_counters(sph_handle *h) {
    return fetch_small(h, h->bodyCountersHost.get(), h->bodyCounters.get(), sizeof(BodyCounters), h->bodyCounted);
}

} // namespace

namespace sph_host {

int label_bodies(sph_handle *h, float linkOption, const char *who) {
    int rc;
    if (!std::isfinite(linkOption) || linkOption < 0.f || linkOption > h->P.h) return fail(h, SPH_EINVAL, "link must be 0 (= h) or finite with 0 < link <= h");
    const float link = linkOption == 0.f ? h->P.h : linkOption;
    const int n = h->n;
    if (n == 0) { // nothing to sweep, nothing to copy
        if ((rc = outbound_fence(h, h->body.out))) return rc;
        h->bodyN = h->bodyCount = 0;
        h->body.valid = true;
        return SPH_OK;
    }
    if ((rc = body_reserve(h, (size_t)n))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    if ((rc = outbound_fence(h, h->body.out))) return rc; // the previous call's copies still read the device buffers
    h->body.valid = false; // (until the copies are queued: the pinned buffers still hold the previous results)
    const bool plain = plain_path("SPH_BODIES_PLAIN");
    BodyArgs A{};
    A.S = sorted_stream(h);
    A.r2 = link * link;
    A.parent = h->bodyParent, A.root = h->bodyRoot, A.rootId = h->bodyRootId, A.rowLabel = h->bodyRowLabel;
    A.flag = h->bodyFlag, A.rank = h->bodyRank, A.blockSum = h->bodyBlockSum;
    A.labels = h->bodyLabels;
    A.counters = h->bodyCounters;
    unsigned long long rounds = 0;
    rc = timed_launch(h, &h->body.seconds, [&]() -> int {
        if (!plain) {
            sph_launch_bodies_unite(h->P, A, h->compute);
            return SPH_OK;
        }
        // at most n rounds: a label moves at least one link closer to every row of its body in each
        sph_launch_bodies_plain_begin(A, h->compute);
        for (bool changed = true; changed && rounds < (unsigned long long)n; ++rounds) {
            sph_launch_bodies_plain_round(h->P, A, rounds == 0, h->compute);
            HIPCHK(h, hipGetLastError());
            if (int rc2 = body_fetch_counters(h)) return rc2;
            changed = h->bodyCountersHost->changed != 0;
        }
        sph_launch_bodies_plain_end(A, h->compute);
        return SPH_OK;
    });
    if (rc) return rc;
    if ((rc = body_fetch_counters(h))) return rc;
    const BodyCounters C = *h->bodyCountersHost.get();
    h->body.calls += 1;
    h->bodyRounds += rounds;
    h->bodyGaveUp += C.gaveUp;
    if (C.gaveUp) return fail(h, SPH_EHIP, std::string(who) + ": a bounded loop of the union-find ran out of trips; no results");
    const size_t bodies = C.numBodies;
    if (bodies == 0 || bodies > (size_t)n) return fail(h, SPH_EHIP, std::string(who) + ": the particle ids are not a permutation of [0, n)");
    h->bodyLinks += C.links;
    h->bodyUnions += plain ? (unsigned long long)n - bodies : C.unions;
    if ((rc = body_reserve_table(h, bodies))) return rc;
    A.table = h->bodyTable;
    if ((rc = timed_launch(h, &h->body.seconds, [&] { sph_launch_bodies_table(A, (int)bodies, h->compute); }))) return rc;
    if ((rc = outbound_send(h, h->body.out, {{h->bodyLabelsHost.get(), h->bodyLabels.get(), (size_t)n * sizeof(uint32_t)},
                                            {h->bodyTableHost.get(), h->bodyTable.get(), bodies * 8 * sizeof(uint32_t)},
                                            {h->bodyFinalHost.get(), h->bodyCounters.get(), sizeof(BodyCounters)}})))
        return rc;
    h->bodyN = n;
    h->bodyCount = (int)bodies;
    h->body.valid = true;
    return SPH_OK;
}

} // namespace sph_host

extern "C" {

int sph_label_bodies(sph_handle *h, const SphBodyOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the bodies' labelling", ": multi-GPU runs label no bodies");
    if (rc) return rc;
    SphBodyOptions o{};
    if ((rc = copy_options(h, opt, o, "SphBodyOptions.struct_size is not set"))) return rc;
    return label_bodies(h, o.link, "sph_label_bodies");
}

int sph_bodies_host(sph_handle *h, const uint32_t **labels, int *n, const uint32_t **table, int *num_bodies, uint32_t *largest) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->body.valid) return fail(h, SPH_ESTATE, "sph_label_bodies must come first");
    HIPCHK(h, outbound_wait(h->body.out));
    const bool any = h->bodyN > 0;
    if (labels) *labels = any ? h->bodyLabelsHost.get() : nullptr;
    if (n) *n = h->bodyN;
    if (table) *table = any ? h->bodyTableHost.get() : nullptr;
    if (num_bodies) *num_bodies = h->bodyCount;
    if (largest) *largest = any ? ~(uint32_t)(h->bodyFinalHost->largest & 0xFFFFFFFFull) : 0u;
    return SPH_OK;
}

int sph_get_body_stats(sph_handle *h, SphBodyStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphBodyStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->body.seconds, &h->body.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    S.links = h->bodyLinks, S.unions = h->bodyUnions, S.rounds = h->bodyRounds, S.gave_up = h->bodyGaveUp;
    if (reset) h->bodyLinks = h->bodyUnions = h->bodyRounds = h->bodyGaveUp = 0;
    *out = S;
    return SPH_OK;
}

} // extern "C"
