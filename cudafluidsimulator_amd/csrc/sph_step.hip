// The single domain's step: the four phases, sph_step with the next step's grid built ahead, the click, and
// the event rings that time them.
//
// Step pipeline (replaces Simulator::simulate / simulateAndTime,
// simulator.cu:462-546):
//   compute stream: clear cell table -> hash -> 3-pass radix sort -> gather +
//                   cell ranges -> density -> force+integrate (+ scatter of
//                   positions into original-id order)
//   copy stream:    D2H of the id-ordered positions into pinned host memory,
//                   double-buffered on the device so step k+1 computes while
//                   step k's positions cross PCIe (the reference blocks on this
//                   copy every step, simulator.cu:479-480,532-533).
#include "sph_handle.h"

#include <chrono>
#include <cstdio>

using namespace sph_host;

namespace sph_host {

// The reference's out-of-grid diagnostic (getGridCell, simulator.cu:60-73), printed by the host after a
// synchronisation instead of by device printf: the first sort pass logs such positions and clamps their
// cell into the table (the reference indexes out of bounds there).
void report_oob(sph_handle *h) {
    if (!h || !h->oobHost) return;
    const uint32_t cnt = h->oobHost->count;
    if (cnt == h->oobSeen) return;
    const int D = h->P.D;
    const uint32_t shown = cnt < SPH_OOB_RECORDS ? cnt : SPH_OOB_RECORDS;
    for (uint32_t k = h->oobSeen < shown ? h->oobSeen : shown; k < shown; ++k) {
        const auto &r = h->oobHost->rec[k];
        const char axis[3] = {'x', 'y', 'z'};
        for (int a = 0; a < 3; ++a)
            if (r.cell[a] < 0 || r.cell[a] >= D)
                printf("OOB particle: %c = %d\n(%f, %f, %f)\n", axis[a], r.cell[a], r.pos[0], r.pos[1], r.pos[2]);
    }
    if (cnt > shown) printf("OOB particle: %u positions outside the grid so far (the first %u listed)\n", cnt, shown);
    fflush(stdout);
    h->oobSeen = cnt;
}

int key_bits(const sph_handle *h) {
    int bits = 1;
    while ((1ll << bits) < (long long)h->P.numCells) ++bits;
    return bits;
}

// xcd_tile() chunk: an eighth of one z-layer's worth of 256-particle tiles.
int tile_chunk(const sph_handle *h, int count, int layers) {
    if (h->knobs.tileChunk >= 0) return h->knobs.tileChunk;
    if (layers <= 0) return 0;
    const long long tiles = ((long long)count + 255) / 256;
    return (int)(tiles / (8ll * layers)); // 0 (contiguous eighths) when a layer is under 8 tiles
}

SweepArgs make_sweep_args(sph_handle *h) {
    SweepArgs A{};
    const int s = h->sorted;
    A.pos4 = h->pos4[s];
    A.vel4 = h->vel4[s];
    A.cellRange = h->cellRange;
    A.keys = h->ws.keys[h->sortedKeyBuf];
    A.pos_out = h->pos4[s ^ 1];
    A.vel_out = h->vel4[s ^ 1];
    A.host_order_pos = nullptr;
    A.force_out = h->force4;
    A.pairCounter = nullptr;
    A.i_begin = 0;
    A.i_end = h->n;
    A.i_origin = 0;
    A.i_begin2 = A.i_end2 = 0;
    A.nblk1 = 0;
    A.patchHalo = 0;
    A.n_all = h->n;
    A.tileChunk = tile_chunk(h, h->n, h->zLayers);
    A.tileRotate = h->knobs.xcdRotate > 0 ? h->knobs.xcdRotate : 0;
    A.maskPool = h->maskPool;
    A.maskOff = h->maskOff;
    A.noneList = h->noneList;
    A.hitCount = h->hitCount;
    A.maskCursor = h->maskCursor;
    A.maskCapacity = h->maskCapacity;
    A.pv8 = h->pv8;
    // (slabs: the wave origin is rounded down to a multiple of 64, the gather launch clears the array,
    // so halo rows -- whose densities arrive after the density sweep -- stay "not quiet")
    A.quiet = h->knobs.zeroPairFilter ? h->quiet.get() : nullptr;
    A.calm = h->calm;
    A.quietAll = A.quiet ? reinterpret_cast<uint32_t *>(h->quietVref + 1) : nullptr;
    A.quietHalo = nullptr; // (slab launches next to a halo layer set it: slab_halo_quiet)
    A.rhoToVel4 = h->external ? 1 : 0;
    A.listHead = reinterpret_cast<const int *>(h->cellRange);
    A.listNext = reinterpret_cast<const int *>(h->ws.vals[0]);
    return A;
}

StreamView sorted_stream(const sph_handle *h) {
    StreamView S{};
    S.n = h->n;
    if (h->n <= 0) return S;
    S.cellRange = h->cellRange;
    if (h->opt.sweep == SPH_SWEEP_LIST && h->pv8) { // the gather left no sorted vel4 in this mode
        S.pos = h->pv8;
        S.vel = h->pv8 + 1;
        S.stride = 2;
    } else {
        S.pos = h->pos4[h->sorted];
        S.vel = h->vel4[h->sorted];
        S.stride = 1;
    }
    return S;
}

// what rides on the gather launch of a grid build: the hit-stream cursors are cleared there
GatherExtras gather_extras(sph_handle *h) {
    GatherExtras X;
    if (h->maskCursor) {
        X.cursor = h->maskCursor;
        X.cursorWords = (int)(kCursorBytes / sizeof(unsigned long long));
        h->cursorClean = true;
    }
    if (h->quiet && h->knobs.zeroPairFilter) {
        X.vref = h->quietVref;
        X.calm = h->calm;
        X.quietAll = reinterpret_cast<uint32_t *>(h->quietVref + 1);
        if (h->external) { // single domain: the density sweep rewrites every word each step
            X.quietClear = h->quiet;
            X.quietWords = (int)(2 * (((size_t)h->cap + 63) / 64) + 2);
        }
    }
    return X;
}

// Fold one finished step's events into the accumulated kernel times.
int resolve_events(sph_handle *h, StepEvents &se) {
    if (!se.used || se.counted) return SPH_OK;
    HIPCHK(h, hipEventSynchronize(se.e[5]));
    float ms[5];
    for (int k = 0; k < 5; ++k) HIPCHK(h, hipEventElapsedTime(&ms[k], se.e[k], se.e[k + 1]));
    h->kt.hash += ms[0] * 1e-3;
    h->kt.sort += ms[1] * 1e-3;
    h->kt.gather += ms[2] * 1e-3;
    h->kt.density += ms[3] * 1e-3;
    h->kt.force += ms[4] * 1e-3;
    if (se.hasCopy) {
        float cms;
        HIPCHK(h, hipEventSynchronize(se.c[1]));
        HIPCHK(h, hipEventElapsedTime(&cms, se.c[0], se.c[1]));
        h->kt.readback += cms * 1e-3;
    }
    h->kt.steps += 1;
    se.counted = true;
    se.used = false;
    if (h->knobs.stepTrace && h->trBase && se.hasCopy) { // GPU-side timeline (ms since the first traced step began)
        float t0 = 0, t3 = 0, t5 = 0, c0 = 0, c1 = 0;
        if (hipEventElapsedTime(&t0, h->trBase, se.e[0]) == hipSuccess && hipEventElapsedTime(&t3, h->trBase, se.e[3]) == hipSuccess &&
            hipEventElapsedTime(&t5, h->trBase, se.e[5]) == hipSuccess && hipEventElapsedTime(&c0, h->trBase, se.c[0]) == hipSuccess &&
            hipEventElapsedTime(&c1, h->trBase, se.c[1]) == hipSuccess)
            fprintf(stderr, "sph timeline: grid %.3f..%.3f sweeps ..%.3f | copy %.3f..%.3f\n", t0, t3, t5, c0, c1);
        (void)hipGetLastError();
    }
    return SPH_OK;
}

int begin_step_events(sph_handle *h) {
    StepEvents &se = h->ring[h->ringHead];
    if (se.used) {
        int rc = resolve_events(h, se);
        if (rc) return rc;
    }
    se.used = true;
    se.counted = false;
    se.hasCopy = false;
    h->curEv = &se;
    h->ringHead = (h->ringHead + 1) % kEventRing;
    return SPH_OK;
}

// Queue the grid build of the state the handle holds now, for the step that comes next (sph_handle::gridAhead):
// that step finds phase 1 and goes on with this build's events.
int build_grid_ahead(sph_handle *h) {
    int rc;
    if ((rc = begin_step_events(h))) return rc;
    StepEvents *nextEv = h->curEv;
    if ((rc = sph_phase_grid(h))) return rc;
    h->curEv = nullptr;
    h->aheadEv = nextEv;
    h->gridAhead = true;
    return SPH_OK;
}

int resolve_pair(sph_handle *h, PairEvent &pe) {
    if (!pe.used) return SPH_OK;
    float ms = 0.f;
    HIPCHK(h, hipEventSynchronize(pe.b));
    HIPCHK(h, hipEventElapsedTime(&ms, pe.a, pe.b));
    *pe.target += ms * 1e-3;
    pe.used = false;
    return SPH_OK;
}

// begin a timed section whose GPU time is added to *target when resolved
int pair_begin(sph_handle *h, double *target, PairEvent **out, hipStream_t stream) {
    PairEvent &pe = h->pairs[h->pairHead];
    int rc = resolve_pair(h, pe);
    if (rc) return rc;
    h->pairHead = (h->pairHead + 1) % kPairRing;
    pe.target = target;
    pe.used = true;
    HIPCHK(h, hipEventRecord(pe.a, stream ? stream : h->compute));
    *out = &pe;
    return SPH_OK;
}

int timed_total(sph_handle *h, double *seconds, long long *count, double *secondsOut, int64_t *countOut, int reset) {
    SPH_ON_DEVICE(h);
    for (auto &pe : h->pairs)
        if (pe.used && pe.target == seconds) {
            int rc = resolve_pair(h, pe);
            if (rc) return rc;
        }
    if (secondsOut) *secondsOut = *seconds;
    if (countOut) *countOut = *count;
    if (reset) {
        *seconds = 0;
        *count = 0;
    }
    return SPH_OK;
}

int outbound_fence(sph_handle *h, Outbound &o) {
    if (o.pending) HIPCHK(h, hipStreamWaitEvent(h->compute, o.copied, 0));
    o.pending = false;
    return SPH_OK;
}

int outbound_send(sph_handle *h, Outbound &o, std::initializer_list<OutboundCopy> copies) {
    HIPCHK(h, o.done.create(hipEventDisableTiming));
    HIPCHK(h, o.copied.create(hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(o.done, h->compute));
    HIPCHK(h, hipStreamWaitEvent(h->copy, o.done, 0));
    for (const OutboundCopy &c : copies) HIPCHK(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->copy));
    HIPCHK(h, hipEventRecord(o.copied, h->copy));
    o.pending = true;
    return SPH_OK;
}

hipError_t outbound_wait(const Outbound &o) { return o.pending ? hipEventSynchronize(o.copied) : hipSuccess; }

int analysis_begin(sph_handle *h, const char *what, const char *slab_hint) {
    if (h->external) return reject_slab_mode(h, slab_hint);
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    const std::string w = what;
    if (h->opt.sweep == SPH_SWEEP_LINKED) return fail(h, SPH_ESTATE, w + " needs a cell table: not available with SPH_SWEEP_LINKED");
    if (h->P.morton) return fail(h, SPH_ESTATE, w + " walks rows of cells as runs of the stream: not available with SPH_KEY_MORTON");
    if (h->phase != 0 && h->phase != 1) return fail(h, SPH_ESTATE, "a step split into phases is still open");
    return SPH_OK;
}

int analysis_grid(sph_handle *h) { return h->phase == 0 && h->n > 0 ? build_grid_ahead(h) : SPH_OK; }

int pass_quiesce(sph_handle *h, Pass &p) {
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    p.out.pending = false;
    p.valid = false;
    return SPH_OK;
}

int fetch_small(sph_handle *h, void *dst, const void *src, size_t bytes, Event &landed) {
    HIPCHK(h, landed.create(hipEventDisableTiming));
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->compute));
    HIPCHK(h, hipEventRecord(landed, h->compute));
    HIPCHK(h, hipEventSynchronize(landed));
    return SPH_OK;
}

int CounterBlock::ensure(sph_handle *h) {
    if (dev) return SPH_OK;
    HIPCHK(h, dev.alloc(count));
    HIPCHK(h, host.alloc(count));
    HIPCHK(h, hipMemsetAsync(dev, 0, count * sizeof(unsigned long long), h->compute));
    return SPH_OK;
}

int CounterBlock::read(sph_handle *h, int reset) {
    if (!dev) return SPH_OK;
    HIPCHK(h, hipMemcpyAsync(host, dev, count * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->compute));
    if (reset) HIPCHK(h, hipMemsetAsync(dev, 0, count * sizeof(unsigned long long), h->compute));
    HIPCHK(h, hipStreamSynchronize(h->compute));
    return SPH_OK;
}

// the density sweep of the single domain and of a slab: counters on request, clean hit-stream cursors
int launch_density(sph_handle *h, SweepArgs &A, hipStream_t stream) {
    if (h->opt.flags & SPH_FLAG_COUNT_PAIRS) A.pairCounter = h->pairCounter;
    if (h->maskCursor && !h->cursorClean) HIPCHK(h, hipMemsetAsync(h->maskCursor, 0, kCursorBytes, stream));
    h->cursorClean = false;
    sph_launch_density(h->P, A, h->opt.math_mode, h->opt.sweep, stream);
    return SPH_OK;
}

// forget a grid that was built ahead for a state that is no longer the current one
void drop_grid_ahead(sph_handle *h) {
    if (!h->gridAhead) return;
    h->gridAhead = false;
    if (h->aheadEv) h->aheadEv->used = false; // (its density / force events were never recorded)
    h->aheadEv = nullptr;
    h->gridValid = false;
    h->phase = 0;
}

// host-side bookkeeping after the particle streams in buffer 0 were replaced
void state_replaced(sph_handle *h) {
    drop_grid_ahead(h);
    (void)sdma_wait(h, 0);
    (void)sdma_wait(h, 1);
    h->rbDeferredSlot = -1;
    h->clickValid = false;
    h->cur = 0;
    h->ready = true;
    h->gridValid = false;
    h->phase = 0;
    h->sorted = -1;
    h->stepIndex = 0;
    h->copyPending[0] = h->copyPending[1] = false;
}

} // namespace sph_host

extern "C" {

int sph_phase_grid(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h);
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    if (h->gridAhead) { // built by the previous timed step for exactly this state
        h->gridAhead = false;
        // (a caller that does not go on with the build's events -- the phase API -- drops them: the
        // density / force events of this entry would never be recorded)
        if (h->aheadEv && h->curEv != h->aheadEv) h->aheadEv->used = false;
        h->aheadEv = nullptr;
        return SPH_OK;  // (phase is 1 already)
    }
    if (h->phase != 0 && h->phase != 3) return fail(h, SPH_ESTATE, "grid phase out of order");
    hipStream_t s = h->compute;
    StepEvents *ev = h->curEv;
    const int c = h->cur, n = h->n;
    if (ev) HIPCHK(h, hipEventRecord(ev->e[0], s));
    if (h->opt.sweep == SPH_SWEEP_LINKED) {
        // the reference's grid: list heads reset (kernelResetGrid :321-326), then one
        // atomic push per particle (kernelBuildGrid :133-147).  No sort, no gather:
        // the streams stay where they are, in particle-id order.
        int *head = reinterpret_cast<int *>(h->cellRange);
        int *next = reinterpret_cast<int *>(h->ws.vals[0]);
        HIPCHK(h, hipMemsetAsync(head, 0xFF, (size_t)h->P.numCells * sizeof(int), s));
        if (ev) HIPCHK(h, hipEventRecord(ev->e[1], s));
        if (ev) HIPCHK(h, hipEventRecord(ev->e[2], s));
        sph_launch_link_build(h->P, h->pos4[c], head, next, n, s);
        if (ev) HIPCHK(h, hipEventRecord(ev->e[3], s));
        HIPCHK(h, hipGetLastError());
        h->sorted = c;
        h->gridValid = false; // no cell-range table in this mode
        h->phase = 1;
        return SPH_OK;
    }
    // kernelResetGrid (simulator.cu:321-326,492-495) and the cell hash are both part of the
    // first sort pass: no launch of their own
    if (ev) HIPCHK(h, hipEventRecord(ev->e[1], s));
    // The table of the last completed step stays intact: a click after a grid built ahead walks it.  Normally that
    // is the previous build's table and the build takes the other one; after a build that was dropped (click after
    // a grid built ahead) it IS the other one, and the dropped build's table is written again.
    h->cellCur ^= 1;
    if (h->clickValid && h->cellTable[h->cellCur] == h->clickTable) h->cellCur ^= 1;
    h->cellRange = h->cellTable[h->cellCur];
    h->ws.velSample = (h->quiet && h->knobs.zeroPairFilter) ? h->vel4[c] : nullptr; // the zero-pair filter's reference velocity
    h->ws.vrefOut = h->quietVref;
    int res = sph_sort_cells(h->ws, h->P, h->pos4[c], n, key_bits(h), s, h->cellRange, h->P.numCells);
    if (ev) HIPCHK(h, hipEventRecord(ev->e[2], s));
    // the list sweeps take velocities from the interleaved records: no sorted vel4 copy
    float4 *velSorted = (h->opt.sweep == SPH_SWEEP_LIST && h->pv8) ? nullptr : h->vel4[c ^ 1];
    sph_launch_gather(h->pos4[c], h->vel4[c], h->ws.vals[res], h->ws.keys[res],
                      h->pos4[c ^ 1], velSorted, h->pv8, h->cellRange, n, s, gather_extras(h));
    if (ev) HIPCHK(h, hipEventRecord(ev->e[3], s));
    HIPCHK(h, hipGetLastError());
    h->sorted = c ^ 1;
    h->sortedKeyBuf = res;
    h->gridValid = true;
    h->phase = 1;
    return SPH_OK;
}

int sph_phase_density(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->phase != 1) return fail(h, SPH_ESTATE, "density phase needs the grid phase first");
    SweepArgs A = make_sweep_args(h);
    if (int rc = launch_density(h, A, h->compute)) return rc;
    if (h->curEv) HIPCHK(h, hipEventRecord(h->curEv->e[4], h->compute));
    HIPCHK(h, hipGetLastError());
    h->phase = 2;
    return SPH_OK;
}

int sph_phase_force(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->phase != 2) return fail(h, SPH_ESTATE, "force phase needs the density phase first");
    SweepArgs A = make_sweep_args(h);
    const int slot = (int)(h->stepIndex & 1);
    if (!(h->opt.flags & SPH_FLAG_NO_READBACK)) {
        // devPos[slot] was last read by the copy of step k-2
        if (h->copyPending[slot]) {
            HIPCHK(h, hipStreamWaitEvent(h->compute, h->copyDone[slot], 0));
            h->copyPending[slot] = false;
        }
        if (h->rbPending[slot]) { // an SDMA copy (timed step k-2) has no stream to wait on: the host waits
            int rc = sdma_wait(h, slot);
            if (rc) return rc;
        }
        A.host_order_pos = h->devPos[slot];
    }
    sph_launch_force(h->P, A, h->opt.math_mode, h->opt.sweep, h->compute);
    if (h->curEv) HIPCHK(h, hipEventRecord(h->curEv->e[5], h->compute));
    HIPCHK(h, hipGetLastError());
    h->cur = h->sorted ^ 1; // new state, still in this step's sorted order
    h->phase = 3;
    h->hostPosIsInit = false;
    h->clickTable = h->cellRange;
    h->clickValid = h->opt.sweep != SPH_SWEEP_LINKED;
    return SPH_OK;
}

int sph_phase_readback(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->phase != 3) return fail(h, SPH_ESTATE, "readback needs the force phase first");
    if (h->opt.flags & SPH_FLAG_NO_READBACK) {
        h->stepIndex++;
        h->phase = 0;
        return SPH_OK;
    }
    const int slot = (int)(h->stepIndex & 1);
    if (h->mappedPos) { // the force sweep already wrote the host buffer
        h->stepIndex++;
        h->phase = 0;
        return SPH_OK;
    }
    if (h->sdmaOk && h->stepTimed && h->n > 0) {
        h->rbDeferredSlot = slot; // sph_step issues the copy once it has seen this step's force sweep finish
        h->stepIndex++;
        h->phase = 0;
        return SPH_OK;
    }
    for (int b = 0; b < 2; ++b) { // (SDMA copies of earlier timed steps write the same host buffer)
        int rc = sdma_wait(h, b);
        if (rc) return rc;
    }
    HIPCHK(h, hipEventRecord(h->computeDone[slot], h->compute));
    HIPCHK(h, hipStreamWaitEvent(h->copy, h->computeDone[slot], 0));
    if (h->curEv) HIPCHK(h, hipEventRecord(h->curEv->c[0], h->copy));
    // (measured, round 3: the copy in 4 / 16 / 64 pieces takes 0.93 / 1.04 / 1.50 ms instead of 0.90)
    if (h->n > 0)
        HIPCHK(h, hipMemcpyAsync(h->hostPos, h->devPos[slot], (size_t)h->n * 3 * sizeof(float),
                                 hipMemcpyDeviceToHost, h->copy));
    if (h->curEv) {
        HIPCHK(h, hipEventRecord(h->curEv->c[1], h->copy));
        h->curEv->hasCopy = true;
    }
    HIPCHK(h, hipEventRecord(h->copyDone[slot], h->copy));
    h->copyPending[slot] = true;
    h->stepIndex++;
    h->phase = 0;
    return SPH_OK;
}

int sph_step(sph_handle *h, SphTimes *times) {
    if (!h) return SPH_EINVAL;
    const auto trIn = std::chrono::steady_clock::now();
    if (h->knobs.stepTrace && h->trSteps > 0) h->trBetween += std::chrono::duration<double>(trIn - h->trLastReturn).count();
    if (h->external) return reject_slab_mode(h);
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    if (h->phase != 0 && h->phase != 3 && !(h->gridAhead && h->phase == 1))
        return fail(h, SPH_ESTATE, "a step split into phases is still open");
    int rc;
    // slot of the PREVIOUS step's position copy (if any)
    const int prevSlot = (int)((h->stepIndex + 1) & 1);
    const bool prevCopy = h->stepIndex > 0 && (h->copyPending[prevSlot] || h->rbPending[prevSlot]);
    StepEvents *ev = nullptr;
    h->stepTimed = times != nullptr; // (the read-back phase picks the copy path by it)
    h->rbDeferredSlot = -1;
    auto trT = std::chrono::steady_clock::now();
    auto trLap = [&](int k) {
        if (!h->knobs.stepTrace) return;
        const auto now = std::chrono::steady_clock::now();
        h->trPh[k] += std::chrono::duration<double>(now - trT).count();
        trT = now;
    };
    if (h->knobs.stepTrace && !h->trBase && !h->gridAhead) {
        if (h->trBase.create() == hipSuccess) (void)hipEventRecord(h->trBase, h->compute);
    }
    if (h->gridAhead) { // the previous timed step queued this step's grid build (and recorded its events)
        ev = h->aheadEv;
        h->curEv = ev;
    } else {
        if ((rc = begin_step_events(h))) return rc;
        ev = h->curEv;
    }
    trLap(0);
    if ((rc = sph_phase_grid(h))) return rc; // (a grid built ahead is consumed here)
    trLap(1);
    if ((rc = sph_phase_density(h))) return rc;
    trLap(2);
    if ((rc = sph_phase_force(h))) return rc;
    trLap(3);
    if ((rc = sph_phase_readback(h))) return rc; // ends the step
    h->stepTimed = false;
    trLap(4);
    h->curEv = nullptr;
    if (times) {
        const auto trA = std::chrono::steady_clock::now();
        if (h->aheadEnabled && h->opt.sweep != SPH_SWEEP_LINKED && h->n > 0) {
            // queue the next step's grid build before waiting for this one (see sph_handle::gridAhead)
            if ((rc = build_grid_ahead(h))) return rc;
            HIPCHK(h, hipEventSynchronize(ev->e[5])); // this step's force sweep (not the grid queued behind it)
        } else {
            HIPCHK(h, hipStreamSynchronize(h->compute));
        }
        const auto trB = std::chrono::steady_clock::now();
        if (h->knobs.stepTrace) {
            h->trEnqueue += std::chrono::duration<double>(trA - trIn).count();
            h->trSync += std::chrono::duration<double>(trB - trA).count();
        }
        if (h->rbDeferredSlot >= 0) { // the force sweep is through: this step's positions leave through an SDMA engine
            const int s2 = h->rbDeferredSlot;
            h->rbDeferredSlot = -1;
            if ((rc = sdma_issue(h, s2))) return rc;
        }
        report_oob(h);
        float gridMs = 0.f, sphMs = 0.f;
        HIPCHK(h, hipEventElapsedTime(&gridMs, ev->e[0], ev->e[3]));
        HIPCHK(h, hipEventElapsedTime(&sphMs, ev->e[3], ev->e[5]));
        times->buildGrid += gridMs * 1e-3;
        times->sphUpdate += sphMs * 1e-3;
        // "Data transfer" = the part of the previous step's D2H that this
        // step's compute did not hide (the reference blocks on every copy,
        // simulator.cu:532-533; here step k's copy overlaps step k+1).
        if (prevCopy) {
            auto t0 = std::chrono::steady_clock::now();
            if (h->copyPending[prevSlot]) HIPCHK(h, hipEventSynchronize(h->copyDone[prevSlot]));
            if ((rc = sdma_wait(h, prevSlot))) return rc;
            times->memcpy +=
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        times->iters += 1;
        if (h->knobs.stepTrace) {
            h->trLastReturn = std::chrono::steady_clock::now();
            h->trPost += std::chrono::duration<double>(h->trLastReturn - trB).count();
            h->trSteps++;
        }
    }
    return SPH_OK;
}

int sph_apply_click(sph_handle *h, int mx, int my) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h);
    if (h->opt.sweep == SPH_SWEEP_LINKED)
        return fail(h, SPH_ESTATE, "the click impulse is not available with SPH_SWEEP_LINKED");
    if (!h->clickValid || (h->phase != 0 && !h->gridAhead) || h->stepIndex == 0)
        return fail(h, SPH_ESTATE, "click needs a completed step (it reuses that step's grid)");
    drop_grid_ahead(h); // a grid built ahead gathered the velocities this impulse is about to change
    sph_launch_click(h->P, h->clickTable, h->vel4[h->cur], mx, my, h->compute);
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

const float *sph_positions_host(sph_handle *h) {
    if (!h) return nullptr;
    if (hipStreamSynchronize(h->compute) != hipSuccess ||
        hipStreamSynchronize(h->copy) != hipSuccess) {
        h->err = "stream synchronize failed";
        return nullptr;
    }
    if (sdma_wait(h, 0) || sdma_wait(h, 1)) return nullptr;
    if (h->hostPosIsInit && h->initPos4 && h->hostPos && h->n > 0) {
        // the initial streams are in id order: x, y, z of every 16-byte row
        if (hipMemcpy2D(h->hostPos, 3 * sizeof(float), h->initPos4, sizeof(float4), 3 * sizeof(float), (size_t)h->n,
                        hipMemcpyDeviceToHost) != hipSuccess) {
            h->err = "copy of the initial positions failed";
            return nullptr;
        }
    }
    h->hostPosIsInit = false;
    report_oob(h);
    return h->hostPos;
}

} // extern "C"
