// Neighbour lists: sph_neighbour_lists and what reads its results (kernels: neighbours.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

constexpr uint64_t kDefaultMaxEntries = 1ull << 28; // 1 GiB of ids

// (re)allocate the per-particle buffers for n particles
int neighbour_reserve(sph_handle *h, size_t n) {
    if (!h->nbrTotals) {
        HIPCHK(h, h->nbrTotals.alloc(2));
        HIPCHK(h, h->nbrTotalsHost.alloc(2));
    }
    if (n <= h->nbrCap) return SPH_OK;
    int rc = pass_quiesce(h, h->nbr); // the old buffers may still be read by a queued copy
    if (rc) return rc;
    h->nbrCap = 0;
    HIPCHK(h, h->nbrCounts.alloc(n));
    HIPCHK(h, h->nbrOffsets.alloc(n + 1));
    HIPCHK(h, h->nbrBlockSum.alloc((size_t)sph_neighbour_scan_blocks((int)n)));
    HIPCHK(h, h->nbrOffsetsHost.alloc(n + 1));
    h->nbrCap = n;
    return SPH_OK;
}

// ... and the lists, once their total is known: an eighth more than asked for, so that a run whose lists grow a
// little from call to call does not reallocate in every one
int neighbour_reserve_entries(sph_handle *h, uint64_t entries) {
    if (entries <= h->nbrEntryCap) return SPH_OK;
    int rc = pass_quiesce(h, h->nbr);
    if (rc) return rc;
    h->nbrEntryCap = 0;
    const uint64_t cap = entries + entries / 8;
    HIPCHK(h, h->nbrLists.alloc((size_t)cap));
    HIPCHK(h, h->nbrListsHost.alloc((size_t)cap));
    h->nbrEntryCap = cap;
    return SPH_OK;
}

// SPH_NEIGHBOURS_TIME_PHASE (sph_handle.h): 0 = every phase is timed, else only this one (1 count, 2 scan, 3 emit, 4 sort)
template <class F>
int phase_launch(sph_handle *h, int phase, int only, F &&launch) {
    if (only == 0 || only == phase) return timed_launch(h, &h->nbr.seconds, launch);
    launch();
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_neighbour_lists(sph_handle *h, const SphNeighbourOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the neighbour lists' sweep", ": multi-GPU runs list no neighbours (lists cross slab boundaries)");
    if (rc) return rc;
    SphNeighbourOptions o{};
    if ((rc = copy_options(h, opt, o, "SphNeighbourOptions.struct_size is not set"))) return rc;
    if (o.flags & ~SPH_NEIGHBOURS_WALK_ORDER) return fail(h, SPH_EINVAL, "SphNeighbourOptions.flags: an unknown flag");
    if (o.pad_ != 0) return fail(h, SPH_EINVAL, "SphNeighbourOptions.pad_ must be 0");
    if (!std::isfinite(o.radius) || o.radius < 0.f || o.radius > h->P.h)
        return fail(h, SPH_EINVAL, "radius must be 0 (= h) or finite with 0 < radius <= h");
    const float radius = o.radius == 0.f ? h->P.h : o.radius;
    const uint64_t maxEntries = o.max_entries ? o.max_entries : kDefaultMaxEntries;
    const int n = h->n;
    if (n == 0) { // nothing to sweep, nothing to copy
        if ((rc = outbound_fence(h, h->nbr.out))) return rc;
        h->nbrN = 0;
        h->nbrEntries = h->nbrLongest = 0;
        h->nbr.valid = true;
        return SPH_OK;
    }
    if ((rc = neighbour_reserve(h, (size_t)n))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    const bool plain = plain_path("SPH_NEIGHBOURS_PLAIN");
    const int only = call_knob("SPH_NEIGHBOURS_TIME_PHASE");
    if (!plain && (rc = h->nbrCounters.ensure(h))) return rc;
    if ((rc = outbound_fence(h, h->nbr.out))) return rc; // the previous call's copies still read the device buffers
    h->nbr.valid = false; // (until the copies are queued; a refused result leaves none)
    NeighbourArgs A{};
    A.S = sorted_stream(h);
    A.r2 = radius * radius;
    A.counts = h->nbrCounts, A.offsets = h->nbrOffsets, A.blockSum = h->nbrBlockSum;
    A.totals = h->nbrTotals;
    A.counters = h->nbrCounters.dev;
    if ((rc = phase_launch(h, 1, only, [&] { sph_launch_neighbour_count(h->P, A, plain, h->compute); }))) return rc;
    if ((rc = phase_launch(h, 2, only, [&] { sph_launch_neighbour_scan(A, h->compute); }))) return rc;
    // the one wait of the call: the total sizes the lists
    if ((rc = fetch_small(h, h->nbrTotalsHost.get(), h->nbrTotals.get(), 2 * sizeof(unsigned long long), h->nbrCounted))) return rc;
    const uint64_t entries = h->nbrTotalsHost.get()[0];
    h->nbr.calls += 1;
    h->nbrEntriesSum += entries;
    h->nbrLongest = h->nbrTotalsHost.get()[1];
    if (entries > maxEntries)
        return fail(h, SPH_ENOMEM, "sph_neighbour_lists: the lists hold " + std::to_string(entries) + " entries, more than max_entries = " +
                                       std::to_string(maxEntries) + "; no results");
    if (entries > 0) {
        if ((rc = neighbour_reserve_entries(h, entries))) return rc;
        A.neighbours = h->nbrLists;
        if ((rc = phase_launch(h, 3, only, [&] { sph_launch_neighbour_emit(h->P, A, plain, h->compute); }))) return rc;
        if (!(o.flags & SPH_NEIGHBOURS_WALK_ORDER) &&
            (rc = phase_launch(h, 4, only, [&] { sph_launch_neighbour_sort(A, plain, h->compute); })))
            return rc;
        rc = outbound_send(h, h->nbr.out, {{h->nbrOffsetsHost.get(), h->nbrOffsets.get(), ((size_t)n + 1) * sizeof(uint64_t)},
                                          {h->nbrListsHost.get(), h->nbrLists.get(), (size_t)entries * sizeof(uint32_t)}});
    } else {
        rc = outbound_send(h, h->nbr.out, {{h->nbrOffsetsHost.get(), h->nbrOffsets.get(), ((size_t)n + 1) * sizeof(uint64_t)}});
    }
    if (rc) return rc;
    h->nbrN = n;
    h->nbrEntries = entries;
    h->nbr.valid = true;
    return SPH_OK;
}

int sph_neighbours_host(sph_handle *h, const uint64_t **offsets, const uint32_t **neighbours, int *n, uint64_t *entries) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->nbr.valid) return fail(h, SPH_ESTATE, "sph_neighbour_lists must come first");
    HIPCHK(h, outbound_wait(h->nbr.out));
    if (offsets) *offsets = h->nbrN > 0 ? h->nbrOffsetsHost.get() : &h->nbrNoOffsets;
    if (neighbours) *neighbours = h->nbrEntries > 0 ? h->nbrListsHost.get() : nullptr;
    if (n) *n = h->nbrN;
    if (entries) *entries = h->nbrEntries;
    return SPH_OK;
}

int sph_get_neighbour_stats(sph_handle *h, SphNeighbourStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphNeighbourStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->nbr.seconds, &h->nbr.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if ((rc = h->nbrCounters.read(h, reset))) return rc;
    if (const unsigned long long *c = h->nbrCounters.host) S.runs_staged = c[0], S.runs_direct = c[1];
    S.entries = h->nbrEntriesSum, S.longest = h->nbrLongest;
    if (reset) h->nbrEntriesSum = h->nbrLongest = 0;
    *out = S;
    return SPH_OK;
}

} // extern "C"
