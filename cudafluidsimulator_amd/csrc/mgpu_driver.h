// In-process multi-GPU driver (include/sph_mgpu.h): z-slabs of whole cell layers, one per
// MI355X, a one-cell halo exchanged with RCCL send/recv over xGMI every step.  Host logic
// only -- the kernels are libsph_hip.so's, driven through the slab entry points of
// include/sph_c_api.h; there is no reference counterpart (the reference's step,
// simulator.cu:462-546, is single-GPU).
//
// This header: the driver object and what its units share -- mgpu_plan.h (every size derived from
// headers), mgpu_transport.cpp (a round of messages), mgpu_state.cpp (the object, its buffers, the
// cutting of slabs), mgpu_step.cpp (the step).
//
// Why z: it is the slowest digit of the flattened cell key (simulator.cu:78-82), so a slab
// is a contiguous range of the key-sorted particle streams and so are its boundary
// layers; gravity acts along y (simulator.cu:270-271) and does not drain slabs.
//
// Order of the combined array before its stable sort -- [halo from below | my migrants
// down | migrants from below | mine | migrants from above | my migrants up | halo from
// above] -- reproduces, inside every cell, the order a stable sort of the previous GLOBAL
// sequence (slabs concatenated by rank) would give, so N slabs equal the single domain bit
// for bit.  The same argument covers re-cutting the slabs (stable filter of that sequence).
//
// Host synchronisations per step: ONE (after exchange A, to read the partition bounds and
// the neighbours' headers); every later size is derived from those headers, and the
// derivation is checked against the sort's own bounds one step later.
#pragma once

#include "mgpu_plan.h"
#include "sph_mgpu.h"
#include "sph_owned.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mgpu_host {

using sph_owned::DeviceBuf;
using sph_owned::Event;
using sph_owned::PinnedBuf;

struct F4 { float x, y, z, w; };

// The slab's pinned host words: what the step's one synchronisation reads, and the outgoing status word.
struct Pinned {
    Hdr mine;     // own header (partition bounds)
    Hdr rx[2];    // the neighbours' headers: [0] from below, [1] from above
    int sort[4];  // bounds of the combined sort
    int pad[3];
    int status;
};
static_assert(sizeof(Pinned) == 128 && offsetof(Pinned, rx) == 32 && offsetof(Pinned, sort) == 96 &&
                  offsetof(Pinned, status) == 124, "own Hdr (8 ints) | rx Hdr x2 (16) | sort bounds (4) | pad | status");

// What alloc_slab makes and free_slab resets wholesale: assigning SlabResources{} releases every buffer and event
// (the handle and the streams: free_slab itself).
struct SlabResources {
    int zlo = 0, zhi = 0;
    bool has_dn = false, has_up = false;
    sph_handle *h = nullptr;
    hipStream_t s = nullptr;      // compute (owned by h unless shared)
    hipStream_t comm = nullptr;   // exchange B overlaps the interior force sweep
    hipStream_t bnd = nullptr;    // the boundary layers' force sweep (joins the interior's launch)
    hipStream_t copy = nullptr;   // position read-back
    Event evDensity, evB, evBnd, evForce, evCopy; // (without timing)
    Event evT[3];                 // step start, grid done, force done (the timed ones)
    Event evTx[2];                // STREAMS transport: [compute, exchange] stream reached its sends (without timing)
    Event evRx[2];                //                    ... its receives have landed
    DeviceBuf<F4> pos[2], vel[2];
    DeviceBuf<F4> rx_pos[2], rx_vel[2]; // [0] from below, [1] from above
    DeviceBuf<F4> ex_pos[2], ex_vel[2]; // overflow messages (rare: ensure_extra)
    int ex_cap[2] = {0, 0};
    DeviceBuf<Hdr> hdr_tx;
    DeviceBuf<Hdr> hdr_rx;        // [2]
    DeviceBuf<int> sortb;         // bounds of the combined sort (5 ints)
    PinnedBuf<Pinned> pinned;
    PinnedBuf<F4> hostRows;       // owned pos4 rows of the last step
    int hostRowsCount = 0;
    bool rowsStale = true;        // hostRows does not hold the owned rows (fresh upload, re-cut): refill on demand
    bool copyPending = false;
    int cur = 0, off = 0, n_own = 0;
    // per step
    int sbuf = 0;
    Assembly a{};                 // n_comb, i0, e_lo, s_hi, i1 of this step
    Hdr mine{}, nb_dn{}, nb_up{};
    bool expectValid = false;
    int expect[4] = {0, 0, 0, 0};
    int status = 0;
};

// A local slab: its identity, which outlives a re-allocation, on top of its resources.
struct Slab : SlabResources {
    int rank = 0, device = 0;
    ncclComm_t comm_nccl = nullptr;
};

// The face between ranks r and r+1; lo / hi is null where that rank lives in another driver object.
struct Face { int r; Slab *lo, *hi; };

// One message of a round.
struct Msg {
    int src_rank, dst_rank;
    const void *src; // valid if the sender is local
    void *dst;       // valid if the receiver is local
    size_t bytes;
};

// Optional host threads, one per local slab (SPH_MGPU_THREADS=1): the ~25 launches of a slab step
// cost the ONE host thread ~0.13 ms per slab, so an in-process run of eight GPUs is bound by the
// host at this problem size (profiles/r02_experiments.md).  The per-slab parts of a step (partition;
// assemble + sort + density; force + read-back) touch one slab each and run on the slab's worker;
// everything that spans slabs (message rounds, the host synchronisation, re-cuts) stays on the
// calling thread, between two joins.  Off by default: one host thread, as the reference has.
struct Workers {
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable wake, done;
    const std::function<int(int)> *job = nullptr; // slab index -> status
    long long generation = 0;
    int pending = 0;
    bool stop = false;
    std::vector<int> rc;
};

} // namespace mgpu_host

struct sph_mgpu {
    SphSettings settings{};
    SphMgpuOptions opt{};
    int n = 0, D = 0, DD = 0;
    int cap = 0, F = 0;
    std::vector<mgpu_host::Slab> slabs; // local slabs, ascending rank (sized once, by sph_mgpu_create)
    std::vector<mgpu_host::Face> faces; // the faces with at least one local end, ascending
    std::vector<int> cuts;         // world+1 layer cuts
    bool shared_stream = false;    // loopback / self transport: every slab on one stream
    hipStream_t shared = nullptr;
    std::vector<float> hostPos;    // n x 3, id order
    bool hostPosValid = false;
    bool ready = false;
    long long step = 0;
    SphMgpuStats stats{};
    std::string err;
    // step state carried between the phases of one step
    std::chrono::steady_clock::time_point t_begin;
    bool overflow = false;
    int phase = 0;                 // phases of the current step already done (0..3)
    bool clickQueued = false;      // sph_mgpu_queue_click: applied by the step that completes next
    // One process per GPU: a rank whose checks fail must not simply stop -- its neighbours would wait in
    // their next grouped receive for ever (the status word only travels with the NEXT exchange A).
    // A "poisoned" driver finishes the message rounds of the running step with the sizes the headers
    // dictate (payload: whatever the buffers hold), posts ONE more exchange A whose header carries
    // status = 1 -- the farewell -- and only then returns the error; a neighbour that reads status = 1
    // does the same towards ITS other neighbours, one rank per step.  Compute is skipped.
    bool poisoned = false;
    int poisonCode = 0;
    int clickX = 0, clickY = 0;
    std::mutex errMu;              // fail() from worker threads
    mgpu_host::Workers *workers = nullptr; // SPH_MGPU_THREADS=1
};

namespace mgpu_host {

// ---- mgpu_state.cpp ----
int fail(sph_mgpu *m, int code, const std::string &msg); // m == nullptr: the error of a failed create
// A check failed.  Every rank in this process: report at once.  Otherwise remember the first failure,
// keep the step's message rounds going (see sph_mgpu::poisoned) and report at the end of the step.
int poison(sph_mgpu *m, int code, const std::string &msg);
// Run fn(slab) for every local slab: in rank order on the calling thread, or on the slabs'
// worker threads (all joined before this returns).  First non-zero status wins.
int for_each_slab(sph_mgpu *m, const std::function<int(Slab &)> &fn);
int recut(sph_mgpu *m);

// ---- mgpu_transport.cpp ----
int init_comms(sph_mgpu *m, const void *unique_id128); // (a failure is reported as the error of the create)
void destroy_comms(sph_mgpu *m);
// Deliver a round of messages.  RCCL: one group of sends and receives on each slab's compute or
// exchange stream; loopback: device-to-device copies on the (shared) stream.
int deliver(sph_mgpu *m, const std::vector<Msg> &msgs, bool on_comm_stream);
int resolve_mail(sph_mgpu *m); // mailbox transport: complete the receives posted in the previous phase

inline Slab *local(sph_mgpu *m, int rank) {
    for (auto &sl : m->slabs)
        if (sl.rank == rank) return &sl;
    return nullptr;
}

// some rank of the run lives in another driver object (process): failures must be announced
inline bool distributed(const sph_mgpu *m) { return (int)m->slabs.size() < m->opt.world; }

#define HIPM(m, call)                                                                 \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess)                                                        \
            return fail((m), SPH_EHIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define NCCLM(m, call)                                                                \
    do {                                                                              \
        ncclResult_t r__ = (call);                                                    \
        if (r__ != ncclSuccess)                                                       \
            return fail((m), SPH_EHIP, std::string(#call) + ": " + ncclGetErrorString(r__)); \
    } while (0)
#define SPHM(m, sl, call)                                                             \
    do {                                                                              \
        int r__ = (call);                                                             \
        if (r__ != SPH_OK)                                                            \
            return fail((m), r__, std::string(#call) + ": " + sph_last_error((sl).h)); \
    } while (0)
#define PASS(call) do { int r__ = (call); if (r__ != SPH_OK) return r__; } while (0)
#define POISON(m, code, msg) PASS(poison((m), (code), (msg)))

} // namespace mgpu_host
