// Body tracks: sph_track_bodies and what reads its results (kernels: body_tracks.hip; the labelling: label_bodies in
// sph_bodies.hip; the moments: measure_labelled in sph_body_moments.hip).
#include "sph_handle.h"

using namespace sph_host;

namespace {

// the counter blocks and next_track, with the first call; the buffers over particle ids, (re)allocated for n of them
int track_reserve(sph_handle *h, size_t n) {
    if (!h->trackCounters) {
        HIPCHK(h, h->trackCounters.alloc(1));
        HIPCHK(h, h->trackCountersHost.alloc(1));
        HIPCHK(h, h->trackFinalHost.alloc(1));
        HIPCHK(h, h->trackNext.alloc(1));
        HIPCHK(h, hipMemsetAsync(h->trackNext, 0, sizeof(unsigned long long), h->compute));
        *h->trackFinalHost.get() = TrackCounters{};
    }
    if (n <= h->trackCap) return SPH_OK;
    int rc = pass_quiesce(h, h->track);
    if (rc) return rc;
    h->trackCap = 0;
    h->trackHasRef = false; // (n is fixed per handle: the first call comes here, with no reference yet)
    h->trackWs = SortWorkspace{};
    for (auto *b : {&h->trackRow[0], &h->trackRow[1], &h->trackPPrev, &h->trackPCur, &h->trackPCount, &h->trackHead, &h->trackEdgeOf,
                    &h->trackParents, &h->trackChildren, &h->trackKeys[0], &h->trackKeys[1], &h->trackVals[0], &h->trackVals[1]})
        HIPCHK(h, b->alloc(n));
    for (auto *b : {&h->trackId[0], &h->trackId[1], &h->trackBestParent, &h->trackBestChild}) HIPCHK(h, b->alloc(n));
    for (auto &b : h->trackBody) HIPCHK(h, b.alloc(n));
    HIPCHK(h, h->trackBlockSum.alloc((size_t)sph_track_scan_blocks((int)n)));
    const size_t nb = sph_sort_workspace_blocks((int)n);
    HIPCHK(h, h->trackBlockHist.alloc(1024 * nb));
    HIPCHK(h, h->trackDigitTotal.alloc(1024));
    SortWorkspace ws{};
    for (int b = 0; b < 2; ++b) ws.keys[b] = h->trackKeys[b], ws.vals[b] = h->trackVals[b];
    ws.blockHist = h->trackBlockHist;
    ws.digitTotal = h->trackDigitTotal;
    ws.capacity = (int)n;
    ws.maxBlocks = (int)nb;
    h->trackWs = ws;
    h->trackCap = n;
    return SPH_OK;
}

// a result's rows on the device and in pinned memory (the compute stream is idle here: the host has just waited for a
// counter; the last result may still be on its way out of the old buffer)
template <class T>
int track_reserve_rows(sph_handle *h, sph_host::DeviceBuf<T> &dev, sph_host::PinnedBuf<T> &host, size_t &cap, size_t rows) {
    if (rows <= cap) return SPH_OK;
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->track.out.pending = false;
    cap = 0;
    HIPCHK(h, dev.alloc(rows));
    HIPCHK(h, host.alloc(rows));
    cap = rows;
    return SPH_OK;
}

int track_fetch_counters(sph_handle *h) {
    return fetch_small(h, h->trackCountersHost.get(), h->trackCounters.get(), sizeof(TrackCounters), h->trackCounted);
}

// no reference, no results; next_track and sequence from 0 again
int track_forget(sph_handle *h) {
    h->trackHasRef = false;
    h->trackRefBodies = 0;
    h->trackSequence = 0;
    h->track.valid = false;
    if (h->trackNext) HIPCHK(h, hipMemsetAsync(h->trackNext, 0, sizeof(unsigned long long), h->compute));
    return SPH_OK;
}

// the call behind its state checks and its options' copy
int track_bodies(sph_handle *h, const SphBodyTrackOptions &o) {
    int rc;
    if ((rc = label_bodies(h, o.link, "sph_track_bodies"))) return rc;
    // the labelling stands from here on, whatever becomes of the tracks
    const int n = h->bodyN;
    const int bodies = h->bodyCount;
    if ((rc = track_reserve(h, (size_t)n))) return rc;
    if ((rc = outbound_fence(h, h->track.out))) return rc; // the previous call's copies still read the device buffers
    h->track.valid = false;
    if (n == 0) { // no bodies, no edges; nothing is queued
        *h->trackFinalHost.get() = TrackCounters{};
        h->trackBodies = h->trackPrevious = h->trackEdgeCount = 0;
        h->trackHasRef = true, h->trackRefBodies = 0;
        h->trackSequence += 1;
        h->track.valid = true;
        return (o.flags & SPH_TRACK_WITH_MOMENTS) ? measure_labelled(h, 0, "sph_track_bodies") : SPH_OK;
    }
    const bool plain = plain_path("SPH_BODIES_PLAIN");
    const int previous = h->trackHasRef ? h->trackRefBodies : 0;
    const int ref = h->trackRef, next = ref ^ 1;
    if ((rc = track_reserve_rows(h, h->trackTracks, h->trackTracksHost, h->trackTracksCap, (size_t)bodies))) return rc;
    if ((rc = track_reserve_rows(h, h->trackFates, h->trackFatesHost, h->trackFatesCap, (size_t)previous))) return rc;
    TrackArgs A{};
    A.S = sorted_stream(h);
    A.rowLabel = h->bodyRowLabel, A.rank = h->bodyRank, A.labels = h->bodyLabels, A.table = h->bodyTable;
    A.numBodies = bodies, A.numPrev = previous;
    A.prow = h->trackRow[ref], A.prevBody = h->trackBody[ref], A.prevTrack = h->trackId[ref];
    A.crow = h->trackRow[next], A.curBody = h->trackBody[next], A.curTrack = h->trackId[next];
    A.nextTrack = h->trackNext;
    A.pPrev = h->trackPPrev, A.pCur = h->trackPCur, A.pCount = h->trackPCount;
    A.head = h->trackHead, A.edgeOf = h->trackEdgeOf, A.blockSum = h->trackBlockSum;
    A.ws = h->trackWs;
    A.parents = h->trackParents, A.children = h->trackChildren;
    A.bestParent = h->trackBestParent, A.bestChild = h->trackBestChild;
    A.tracks = h->trackTracks, A.fates = h->trackFates;
    A.counters = h->trackCounters;
    if ((rc = timed_launch(h, &h->track.seconds, [&] { sph_launch_track_partials(A, plain, h->compute); }))) return rc;
    h->track.calls += 1;
    int partials = 0, edges = 0;
    if (previous > 0) {
        partials = n; // the check path's
        if (!plain) { // the first wait: the number of partial edges sizes the sort
            if ((rc = track_fetch_counters(h))) return rc;
            const uint32_t m = h->trackCountersHost->partials;
            if (m == 0 || m > (uint32_t)n) return fail(h, SPH_EHIP, "sph_track_bodies: the particle ids are not a permutation of [0, n)");
            partials = (int)m;
        }
        h->trackPartialsSum += (unsigned long long)partials;
        int order = 0;
        if ((rc = timed_launch(h, &h->track.seconds, [&] { order = sph_launch_track_sort(A, partials, h->compute); }))) return rc;
        // the second wait: the number of edges sizes the copies and is what max_edges caps
        if ((rc = track_fetch_counters(h))) return rc;
        const uint32_t e = h->trackCountersHost->edges;
        if (e == 0 || e > (uint32_t)partials) return fail(h, SPH_EHIP, "sph_track_bodies: the heads' scan left no edge count");
        edges = (int)e;
        h->trackEdgesSum += (unsigned long long)edges;
        if (o.max_edges && e > o.max_edges) { // the reference, next_track and sequence stay what they were
            if (o.flags & SPH_TRACK_WITH_MOMENTS) h->moment.valid = false;
            return fail(h, SPH_ENOMEM, "sph_track_bodies: the two labellings share " + std::to_string(e) + " edges, more than max_edges = " +
                                           std::to_string(o.max_edges) + "; no tracks");
        }
        if ((rc = track_reserve_rows(h, h->trackEdges, h->trackEdgesHost, h->trackEdgesCap, (size_t)edges))) return rc;
        A.edges = h->trackEdges;
        if ((rc = timed_launch(h, &h->track.seconds, [&] { sph_launch_track_edges(A, partials, edges, order, plain, h->compute); }))) return rc;
    }
    if ((rc = timed_launch(h, &h->track.seconds, [&] { sph_launch_track_assign(A, edges, h->compute); }))) return rc;
    const OutboundCopy tracks{h->trackTracksHost.get(), h->trackTracks.get(), (size_t)bodies * sizeof(SphBodyTrack)};
    const OutboundCopy last{h->trackFinalHost.get(), h->trackCounters.get(), sizeof(TrackCounters)};
    if (previous > 0)
        rc = outbound_send(h, h->track.out, {tracks, last,
                                             {h->trackFatesHost.get(), h->trackFates.get(), (size_t)previous * sizeof(SphBodyFate)},
                                             {h->trackEdgesHost.get(), h->trackEdges.get(), (size_t)edges * sizeof(SphBodyEdge)}});
    else
        rc = outbound_send(h, h->track.out, {tracks, last});
    if (rc) return rc;
    // this labelling is the reference from here on
    h->trackRef = next;
    h->trackHasRef = true, h->trackRefBodies = bodies;
    h->trackSequence += 1;
    h->trackBodies = bodies, h->trackPrevious = previous, h->trackEdgeCount = edges;
    h->track.valid = true;
    return (o.flags & SPH_TRACK_WITH_MOMENTS) ? measure_labelled(h, 0, "sph_track_bodies") : SPH_OK;
}

} // namespace

extern "C" {

int sph_track_bodies(sph_handle *h, const SphBodyTrackOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the bodies' labelling", ": multi-GPU runs label no bodies");
    if (rc) return rc;
    SphBodyTrackOptions o{};
    if ((rc = copy_options(h, opt, o, "SphBodyTrackOptions.struct_size is not set"))) return rc;
    if (o.flags & ~(uint32_t)SPH_TRACK_WITH_MOMENTS) return fail(h, SPH_EINVAL, "SphBodyTrackOptions.flags: unknown bits");
    rc = track_bodies(h, o);
    if (rc == SPH_EHIP) (void)track_forget(h); // (the message stays the failed call's)
    return rc;
}

int sph_body_tracks_host(sph_handle *h, const SphBodyTrack **tracks, int *num_bodies, const SphBodyFate **previous, int *num_previous,
                         const SphBodyEdge **edges, int *num_edges, SphBodyTrackSummary *summary) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->track.valid) return fail(h, SPH_ESTATE, "sph_track_bodies must come first");
    HIPCHK(h, outbound_wait(h->track.out));
    if (tracks) *tracks = h->trackBodies > 0 ? h->trackTracksHost.get() : nullptr;
    if (num_bodies) *num_bodies = h->trackBodies;
    if (previous) *previous = h->trackPrevious > 0 ? h->trackFatesHost.get() : nullptr;
    if (num_previous) *num_previous = h->trackPrevious;
    if (edges) *edges = h->trackEdgeCount > 0 ? h->trackEdgesHost.get() : nullptr;
    if (num_edges) *num_edges = h->trackEdgeCount;
    if (summary) {
        const TrackCounters &C = *h->trackFinalHost.get();
        SphBodyTrackSummary S{};
        S.struct_size = (int32_t)sizeof S;
        S.previous_bodies = (uint32_t)h->trackPrevious, S.bodies = (uint32_t)h->trackBodies, S.edges = (uint32_t)h->trackEdgeCount;
        S.continued = C.continued, S.born = C.born, S.ended = C.ended, S.merges = C.merges, S.splits = C.splits;
        S.next_track = C.nextTrack;
        S.sequence = h->trackSequence;
        *summary = S;
    }
    return SPH_OK;
}

int sph_track_reset(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    return track_forget(h);
}

int sph_get_body_track_stats(sph_handle *h, SphBodyTrackStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphBodyTrackStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->track.seconds, &h->track.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    S.partials = h->trackPartialsSum, S.edges = h->trackEdgesSum;
    if (reset) h->trackPartialsSum = h->trackEdgesSum = 0;
    *out = S;
    return SPH_OK;
}

} // extern "C"
