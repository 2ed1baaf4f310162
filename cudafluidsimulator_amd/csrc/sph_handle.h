// The handle behind include/sph_c_api.h and the few helpers its host translation units share (the sph_*.hip units of
// the Makefile's SRCS).
// Host code only.
// Ownership: every device buffer, pinned block and event below is a DeviceBuf / PinnedBuf / Event (sph_owned.h) and goes
// with the handle; a raw pointer member is a view of one of them (or of the caller's memory) and says so.
#pragma once

#include "sph_c_api.h"
#include "sph_device.h"
#include "sph_owned.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>

namespace sph_host {

using sph_owned::DeviceBuf;
using sph_owned::Event;
using sph_owned::PinnedBuf;

// The library's SPH_* environment knobs: this comment is the list.  None changes a result; all are for A/B runs,
// studies and diagnosis.  "create": read once, by read_knobs() at the top of sph_create, into sph_handle::knobs.
// "call": read by every call, through plain_path() / call_knob().  Numbers are parsed with atoi (an empty value is 0).
//   name                  default  read    what it does
//   SPH_SLIM_DIV          (auto)   create  0: the pair body uses the full IEEE divide / square-root expansions even
//                                          with the reference's constants (same bits); any other value: no effect
//   SPH_PIPELINE          (auto)   create  0 / non-zero: a timed step does not / does queue the next step's grid build
//                                          before it waits; default: on below 1.5 M particles
//   SPH_MASK_POOL_WORDS   (auto)   create  size of the list sweep's hit-stream pool in 32-bit words (strtoull, / 4 =
//                                          quads; then the 32-bit clamp); default: sized from n and the free memory
//   SPH_ZERO_PAIR_FILTER  1        create  0: the list sweep's zero-pair filter is off
//   SPH_PREWARM_COPIES    16       create  small device-to-host copies sph_create issues to warm the runtime's copy path
//   SPH_TILE_CHUNK        -1       create  xcd_tile()'s chunk: -1 auto, 0 contiguous eighths, > 0 tiles per chunk
//   SPH_XCD_ROTATE        -1       create  xcd_tile()'s rotation period in groups (z-layers), 0 = off; -1: off for the
//                                          single domain, every layer for a slab (slab_rotate)
//   SPH_STEP_TRACE        0        create  non-zero: sph_destroy prints where the host spent its timed steps, every timed
//                                          step its GPU timeline, sph_create the SDMA engine it picked
//   SPH_READBACK_SDMA     1        create  0: timed steps read back through the HIP runtime's copy, not an SDMA engine
//   SPH_RENDER_PLAIN      0        call    non-zero: sph_render_frame / _field / _column take the check path
//   SPH_SAMPLE_PLAIN      0        call    non-zero: sph_sample_field takes the one-thread-per-point check path
//   SPH_DIAG_PLAIN        0        call    non-zero: sph_diagnose / sph_slab_diagnose take the check path
//   SPH_SURFACE_PLAIN     0        call    non-zero: sph_extract_surface takes the check path, for its sample and its extraction
//   SPH_TRACER_PLAIN      0        call    non-zero: sph_tracers_advect takes the one-thread-per-tracer check path
//   SPH_DERIVE_PLAIN      0        call    non-zero: sph_derive takes the one-thread-per-row check path
//   SPH_BODIES_PLAIN      0        call    non-zero: sph_label_bodies takes the check path (min-label propagation in rounds),
//                                          and sph_measure_bodies with it, for its labelling and for its moments (one atomic per word),
//                                          and sph_track_bodies, for all three (every particle id a partial edge)
//   SPH_NEIGHBOURS_PLAIN  0        call    non-zero: sph_neighbour_lists takes the check path (one thread per row, one per list)
//   SPH_NEIGHBOURS_TIME_PHASE 0    call    1 count, 2 scan, 3 emit, 4 sort: SphNeighbourStats.seconds sums that phase alone
//                                          (scripts/studies/neighbours.py); 0: all four
//   SPH_PAIRS_PLAIN       0        call    non-zero: sph_pair_statistics takes the check path (one thread per row, the bin by a
//                                          linear scan, every word a global atomic)
//   SPH_PAIRS_WORKGROUPS  0        call    1 .. 65536: the default path of sph_pair_statistics launches that many workgroups
//                                          (at most one per tile) instead of 16 per compute unit; same words
//   SPH_PAIRS_SHED_BITS   62       call    33 .. 62: a high word of that path's table sheds into its top word at 2^bits
//                                          instead of 2^62 (pairs.hip); same words
//   SPH_CAST_PLAIN        0        call    non-zero: sph_cast_rays / sph_render_view take the check path (one thread per ray, every
//                                          row of the stream); admitted while rays x particles <= 2^32
//   SPH_MGPU_THREADS      0        (libsph_mgpu.so, its own object: sph_mgpu_create in mgpu_state.cpp) non-zero: one
//                                          host thread per local slab
// (The SPH_* variables the command-line front end reads -- SPH_SWEEP, SPH_GPUS, SPH_TRANSPORT, SPH_RECUT_EVERY,
// SPH_FREE_*, SPH_PRINT_SHA256 -- are its arguments by another road, not library knobs.)
struct Knobs {
    int slimDiv = 1;        // only 0 acts
    int pipeline = -1;      // -1: by n
    bool maskPoolSet = false;
    unsigned long long maskPoolQuads = 0;
    bool zeroPairFilter = true;
    int prewarmCopies = 16;
    int tileChunk = -1;
    int xcdRotate = -1;
    bool stepTrace = false;
    bool readbackSdma = true;
};
inline int call_knob(const char *name) { // a "call" knob's number (unset: 0)
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
}
inline bool plain_path(const char *name) { return call_knob(name) != 0; }

constexpr int kEventRing = 64;
constexpr int kCounterWords = 16 + 256 * 16; // 16 spare words, then 256 shards x 16: [0] pair tests,
                                             // [1..13] reserved (always zero), [14] bodies, [15] hits
constexpr size_t kCursorBytes = (size_t)SL_POOL_SHARDS * SL_CURSOR_STRIDE * sizeof(unsigned long long);

struct PairEvent { // one timed section of the slab path
    Event a, b;
    double *target = nullptr; // view: the handle's accumulator the section is added to
    bool used = false;
};
constexpr int kPairRing = 48;

// A result on its way to pinned memory over the copy stream, behind what `compute` had queued when it left
// (outbound_* below): the frame, the field sample, the surface mesh.
struct Outbound {
    Event done, copied; // on compute: the result is complete; on copy: it has arrived
    bool pending = false;  // a copy is queued: `copied` tells when the device buffer is free again
};
struct OutboundCopy {
    void *dst;
    const void *src;
    size_t bytes;
};

// What every pass that queues work and hands back a result keeps: the result on its way out, whether the pinned
// buffers hold (or will hold) one, and the GPU time and number of its calls (timed_total reads them).
struct Pass {
    Outbound out;
    bool valid = false;
    double seconds = 0; // from HIP events (PairEvent ring)
    long long calls = 0;
};

// What the last render drew (sph_frame.hip): decides which buffers hold a result and who may read them
enum class FrameKind { Flat, Field, Column, Liquid, View };

// The visualiser's frame (sph_frame.hip; kernels: render.hip).  The first render of an image size allocates the
// per-pixel depth bits, hit count and static box-edge layer and the RGB8 frame, on the device and in pinned memory.
// The first field or column frame of that size adds `packed` -- the field frame's (depth bits << 32 | value bits)
// minimum per pixel, the column frame's 64-bit sum -- and the two words of the colour scale's range, which leave for
// pinned memory with the frame; the first column frame the word of the largest column and the table of the
// pixel-centre rays; the first liquid frame two planes of smoothed depth and one of normals.
struct FrameState {
    RenderParams rp{}; // size / point radius / shade of the last render (width 0: none yet)
    DeviceBuf<uint32_t> depth, count, edge, rgb;
    PinnedBuf<uint8_t> host;
    Pass pass; // out: the frame (and range) on its way to host / rangeHost; valid: a frame of the size in rp is held
    DeviceBuf<unsigned long long> packed;
    DeviceBuf<uint32_t> range;
    PinnedBuf<uint32_t> rangeHost;
    DeviceBuf<unsigned long long> maxWord;
    DeviceBuf<float> rays;
    DeviceBuf<uint32_t> smooth[2];          // the liquid frame's ping-pong planes (first liquid frame of an image size)
    DeviceBuf<float4> normals;              // ... and its normals
    const uint32_t *smoothed = nullptr;     // the plane that holds the last liquid frame's final smoothed depth
    FrameKind kind = FrameKind::Flat; // of the last render
};

// A few 64-bit counters a pass's kernels add to, on the device, with the pinned block they are read through.
struct CounterBlock {
    explicit CounterBlock(int words) : count(words) {}
    DeviceBuf<unsigned long long> dev;
    PinnedBuf<unsigned long long> host;
    const int count;
    int ensure(sph_handle *h);          // allocated and cleared by the first call that needs them
    int read(sph_handle *h, int reset); // host[0, count) = the counters now (never allocated: nothing, host stays null); reset: cleared after
};

struct StepEvents {
    Event e[6]; // start, hash, sort, gather, density, force
    Event c[2]; // copy start / end
    bool used = false, hasCopy = false, counted = false;
};

} // namespace sph_host

struct sph_handle {
    // ---- sph_api.hip: settings, the particle streams and the grid's buffers, state flags ----
    SphSettings settings{};
    SphOptions opt{};
    sph_host::Knobs knobs{}; // the SPH_* environment, as sph_create found it
    DevParams P{};
    int n = 0, cap = 0, device = 0;
    hipStream_t compute = nullptr, copy = nullptr; // created by sph_create; sph_destroy destroys them last, after every buffer and event
    sph_host::DeviceBuf<float4> posBuf[2], velBuf[2]; // the particle streams of a handle that owns its state
    float4 *pos4[2] = {nullptr, nullptr}; // views: posBuf / velBuf, or the caller's buffers (sph_bind_buffers)
    float4 *vel4[2] = {nullptr, nullptr};
    int cur = 0;     // buffers holding the current state
    int sorted = -1; // buffers holding the sorted streams of the last grid build
    sph_host::DeviceBuf<uint32_t> sortKeys[2], sortVals[2], sortBlockHist, sortDigitTotal;
    SortWorkspace ws{}; // views of the six above and of oobHost (the struct is sort.hip's argument)
    int sortedKeyBuf = 0;
    int2 *cellRange = nullptr;       // view: the cell table of the LAST grid build (= cellTable[cellCur])
    sph_host::DeviceBuf<int2> cellTable[2]; // two tables: a grid built ahead (below) must not clobber the last step's
    int cellCur = 0;
    sph_host::DeviceBuf<float> devPosBuf[2];
    float *devPos[2] = {nullptr, nullptr}; // views: devPosBuf, or (SPH_FLAG_MAPPED_POSITIONS) the device address of hostPos
    sph_host::PinnedBuf<float> hostPos; // n*3
    bool hostPosIsInit = false; // setup() restored the initial state on the device: getPosition() fetches it on demand
    // Pinned staging for state uploads (two halves, ping-pong).  A hipMemcpy from pageable
    // memory makes the runtime pin and later unpin the caller's pages; the unpin is deferred
    // and stalls the GPU's queues for 6-28 ms some time AFTER the call returned -- inside the
    // first steps of the run that follows (measured).
    sph_host::PinnedBuf<float4> stage[2];
    sph_host::Event stageFree[2];
    bool mappedPos = false;   // SPH_FLAG_MAPPED_POSITIONS: devPos[] view hostPos (host-mapped)
    sph_host::DeviceBuf<float4> force4;
    sph_host::DeviceBuf<unsigned long long> pairCounter;
    sph_host::PinnedBuf<unsigned long long> pairHost;
    SphKernelTimes kt{};
    sph_host::DeviceBuf<float4> pv8;
    sph_host::DeviceBuf<uint32_t> maskPool, maskOff; // SPH_SWEEP_LIST
    sph_host::DeviceBuf<uint32_t> noneList; // SPH_SWEEP_LIST: waves without a stream this step (pool exhausted)
    sph_host::DeviceBuf<uint32_t> hitCount; // SPH_SWEEP_LIST: recorded hits per sorted row
    sph_host::DeviceBuf<uint32_t> quiet;    // SPH_SWEEP_LIST: one bit per sorted row, the force sweep's zero-pair filter
    sph_host::DeviceBuf<float4> quietVref; // ... its reference velocity (picked by the first sort pass) ...
    sph_host::DeviceBuf<unsigned long long> calm; // ... and one bit per sorted row "moves with it" (written by the gather launch)
    sph_host::DeviceBuf<float4> initPos4; // setup()'s initial positions (+ids), kept on the device for the next setup()
    sph_host::PinnedBuf<SphOobLog> oobHost; // host-mapped: positions outside the grid met by the cell hash
    uint32_t oobSeen = 0;            // how many of them were already reported
    int initZLayers = 0;
    uint64_t hitsRecorded = 0;       // SPH_FLAG_COUNT_PAIRS: hits in the stream, before the filter
    sph_host::DeviceBuf<unsigned long long> maskCursor;
    unsigned long long maskCapacity = 0; // quads (16 B)
    int zLayers = 0;        // occupied z-layers of the (owned) particles: sizes xcd_tile()'s chunks
    bool ready = false;     // state uploaded
    bool gridValid = false; // sorted streams + cell table match `sorted`
    int phase = 0;          // 0 idle, 1 grid done, 2 density done, 3 force done
    std::string err;

    // ---- sph_step.hip: the step pipeline, its events and the host-side trace ----
    // Step pipelining (timed steps): simulateAndTime() has to wait for its step, and between that wait and the
    // first launch of the next call the GPU idled ~0.12 ms per step (host: two event queries, the return to the
    // caller -- Python in bench.py --, the next call's first launches).  A timed step therefore queues the NEXT
    // step's grid build (which only needs the state this step leaves behind) BEFORE it waits, and waits for its
    // own force event instead of the whole stream; the next step finds its grid built.  Anything that changes
    // or replaces the state in between (click, upload, load) simply drops the grid built ahead.
    bool gridAhead = false;
    int2 *clickTable = nullptr;      // view: cell table of the last COMPLETED step (what sph_apply_click walks)
    bool clickValid = false;
    bool aheadEnabled = true;        // default: below 1.5 M particles; SPH_PIPELINE=0/1 forces it (same results)
    sph_host::StepEvents *aheadEv = nullptr; // view into ring[]
    sph_host::Event computeDone[2], copyDone[2];
    bool copyPending[2] = {false, false};
    bool stepTimed = false;          // sph_step(times != NULL) is running (the read-back phase picks the copy path by it)
    int rbDeferredSlot = -1;         // the read-back phase left this slot's copy to sph_step
    bool cursorClean = false; // the gather launch of this grid build cleared the hit-stream cursors
    long long stepIndex = 0;
    sph_host::StepEvents ring[sph_host::kEventRing];
    int ringHead = 0;
    sph_host::StepEvents *curEv = nullptr; // view into ring[]
    sph_host::PairEvent pairs[sph_host::kPairRing];
    int pairHead = 0;
    // SPH_STEP_TRACE=1 (knobs.stepTrace, diagnostic): where the HOST spends a timed step, printed by sph_destroy
    double trEnqueue = 0, trSync = 0, trPost = 0, trBetween = 0, trPh[5] = {0, 0, 0, 0, 0};
    long long trSteps = 0;
    std::chrono::steady_clock::time_point trLastReturn{};
    sph_host::Event trBase;           // first traced step's start: GPU-side timeline of every later step

    // ---- sph_readback.hip ----
    // Read-back of a TIMED step through an SDMA engine (hsa_amd_memory_async_copy) instead of the HIP runtime's
    // copy, which on this platform is a blit KERNEL: beside it the first histogram pass takes 84 instead of
    // 27 us, the density sweep +30 us, the force sweep +50 us.  The engine moves the
    // same 56 GB/s and occupies no CU.  HIP offers no way to order an HSA copy behind a kernel, so the copy
    // is issued by the host right after it has seen the step's force sweep finish -- which a timed step
    // waits for anyway; untimed steps (simulate()) keep the stream-ordered HIP copy.  SPH_READBACK_SDMA=0: off.
    bool sdmaOk = false;
    uint64_t hsaGpu = 0, hsaCpu = 0; // hsa_agent_t::handle
    uint64_t rbSig[2] = {0, 0};      // hsa_signal_t::handle
    bool rbPending[2] = {false, false};
    uint32_t sdmaEngine = 0;         // hsa_amd_sdma_engine_id_t picked by sdma_init (0: the HSA runtime's own choice)
    double hsaTickSeconds = 0;

    // ---- sph_slab.hip ----
    int slabOwnedBegin = 0, slabOwnedEnd = 0; // rows of the last sph_slab_density (the rest of [0, n_all) is halo)
    bool external = false;  // pos4/vel4 are caller-owned (sph_bind_buffers)
    hipStream_t ownCompute = nullptr; // the created `compute` while a caller's stream stands in (sph_set_stream)
    sph_host::DeviceBuf<int> boundsDev;
    sph_host::PinnedBuf<int> boundsHost;
    sph_host::DeviceBuf<int> partTiles; // slab partition: class counts per 1024-particle tile

    // ---- sph_frame.hip ----
    sph_host::FrameState frame;

    // ---- sph_sample.hip ----
    // The field sample (sample.hip): one float per lattice point on the device and in pinned memory, both grown
    // on demand by sph_sample_field.
    sph_host::DeviceBuf<float> sampleDev;
    sph_host::PinnedBuf<float> sampleHost;
    size_t sampleCap = 0;            // floats either buffer holds
    int sampleDim[3] = {0, 0, 0};    // nx, ny, nz of the last sample
    sph_host::Pass sample;           // out: the values on their way to sampleHost; seconds: the sampling kernel
    long long sampleTileCalls = 0, samplePlainCalls = 0; // which kernel ran (SPH_STEP_TRACE=1: printed by sph_destroy)

    // ---- sph_surface.hip ----
    // The surface mesh (surface.hip): per lattice point the density sample, the corner byte and the block-relative
    // offsets; per counting block its sums and offsets; the two totals; the mesh on the device and in pinned memory.
    // All grown on demand by sph_extract_surface.
    sph_host::DeviceBuf<float> surfField;
    sph_host::DeviceBuf<uint8_t> surfBits;
    sph_host::DeviceBuf<uint32_t> surfLocal;
    sph_host::DeviceBuf<uint2> surfBlockSum, surfBlockOff;
    sph_host::DeviceBuf<unsigned long long> surfTotalsDev;
    sph_host::PinnedBuf<unsigned long long> surfTotalsHost;
    sph_host::Event surfCounted;     // the totals have landed
    size_t surfPointCap = 0, surfBlockCap = 0; // points / blocks the buffers above hold
    sph_host::DeviceBuf<float> surfVertsDev;
    sph_host::DeviceBuf<uint32_t> surfTrisDev;
    sph_host::PinnedBuf<float> surfVertsHost;
    sph_host::PinnedBuf<uint32_t> surfTrisHost;
    size_t surfVertCap = 0, surfTriCap = 0; // vertices / triangles either buffer holds
    long long surfVerts = 0, surfTris = 0;  // of the last extraction
    sph_host::Pass surf;             // out: the mesh on its way to surfVertsHost / surfTrisHost; seconds: count + scan + emit
    double surfSampleSeconds = 0;    // ... and the sampling kernel
    long long surfWaveCalls = 0, surfPlainCalls = 0; // which path ran (SPH_STEP_TRACE=1: printed by sph_destroy)

    // ---- sph_diag.hip ----
    // Run diagnostics (diag.hip): the small result block on the device and in pinned memory, allocated by the
    // first sph_diagnose / sph_slab_diagnose.
    sph_host::DeviceBuf<DiagBlock> diagDev;
    sph_host::PinnedBuf<DiagBlock> diagHost;
    sph_host::Pass diag;             // out: the block on its way to diagHost; seconds: clear + reduce + histogram
    int diagN = 0;                   // rows of the last call
    SphDiagnosticsOptions diagOpt{}; // ... its options
    bool diagAuto = false;           // ... and whether its histogram took the reduced range

    // ---- sph_tracers.hip ----
    // Passive tracers (tracers.hip): (x, y, z, den) and (ux, uy, uz, 0) per tracer in the caller's order, on the
    // device and in pinned memory, grown on demand by sph_tracers_set; the tracers' own sort workspace and the walk
    // kernel's three counters, allocated by the first advect that needs them.
    sph_host::DeviceBuf<float4> tracerPosDen, tracerVel;
    sph_host::PinnedBuf<float4> tracerPosDenHost, tracerVelHost;
    size_t tracerCap = 0;            // tracers either pair of buffers holds
    int tracerCount = 0;             // m of the last sph_tracers_set
    sph_host::DeviceBuf<uint32_t> tracerKeys[2], tracerVals[2], tracerBlockHist, tracerDigitTotal;
    SortWorkspace tracerWs{};        // views of the six above (capacity 0: not allocated yet)
    sph_host::CounterBlock tracerCounters{kTracerCounters}; // waves_shared, waves_direct, groups
    sph_host::Pass tracer;           // out: the results on their way to tracerPosDenHost / tracerVelHost (valid: unused, the
                                     // tracers are the caller's); seconds: key + sort + walk

    // ---- sph_derived.hip ----
    // Derived per-particle fields (derived.hip): (wx, wy, wz, div), (gx, gy, gz, rho) and the neighbour count per
    // particle in id order, on the device and in pinned memory, grown on demand by sph_derive; the default path's
    // two counters, allocated by the first derive that needs them.
    sph_host::DeviceBuf<float4> deriveVortDiv, deriveGradRho;
    sph_host::DeviceBuf<uint32_t> deriveNeighbours;
    sph_host::PinnedBuf<float4> deriveVortDivHost, deriveGradRhoHost;
    sph_host::PinnedBuf<uint32_t> deriveNeighboursHost;
    size_t deriveCap = 0;            // particles each of the six buffers holds
    int deriveN = 0;                 // rows of the last sph_derive
    sph_host::CounterBlock deriveCounters{kDeriveCounters}; // runs_staged, runs_direct
    sph_host::Pass derive;           // out: the results on their way to the three pinned buffers; seconds: the sweep

    // ---- sph_bodies.hip ----
    // Bodies (bodies.hip): the working arrays over rows and particle ids, the labels in id order and the table on the
    // device and in pinned memory, all grown on demand by sph_label_bodies; the counter block on the device, its
    // pinned copy the call waits for (the number of bodies) and the one that leaves with the results (the largest).
    sph_host::DeviceBuf<uint32_t> bodyParent, bodyRoot, bodyRootId, bodyRowLabel, bodyFlag, bodyRank, bodyBlockSum;
    sph_host::DeviceBuf<uint32_t> bodyLabels, bodyTable;
    sph_host::PinnedBuf<uint32_t> bodyLabelsHost, bodyTableHost;
    sph_host::DeviceBuf<BodyCounters> bodyCounters;
    sph_host::PinnedBuf<BodyCounters> bodyCountersHost, bodyFinalHost;
    sph_host::Event bodyCounted;     // the counter block has landed
    size_t bodyCap = 0, bodyTableCap = 0; // particles / table rows the buffers hold
    int bodyN = 0, bodyCount = 0;    // rows and bodies of the last sph_label_bodies
    sph_host::Pass body;             // out: the results on their way to the pinned buffers; seconds: every kernel of the call
    unsigned long long bodyLinks = 0, bodyUnions = 0, bodyRounds = 0, bodyGaveUp = 0; // sums over calls

    // ---- sph_body_moments.hip ----
    // Per-body moments (body_moments.hip): one row of kBodyMomentStride words per body and the 32 size bins, on the
    // device and in pinned memory; the rows grow on demand by sph_measure_bodies, the bins come with its first call.
    sph_host::DeviceBuf<unsigned long long> momentRows;
    sph_host::PinnedBuf<unsigned long long> momentRowsHost;
    sph_host::DeviceBuf<uint32_t> momentHist;
    sph_host::PinnedBuf<uint32_t> momentHistHost;
    size_t momentCap = 0;            // bodies either row buffer holds
    int momentCount = 0;             // bodies of the last sph_measure_bodies
    sph_host::Pass moment;           // out: rows and bins on their way to the pinned buffers; seconds: the moment launches alone

    // ---- sph_body_tracks.hip ----
    // Body tracks (body_tracks.hip).  The reference, on the device: the table row of every particle id's body, (label,
    // count) and the track of every body, each twice -- [trackRef] is the reference, the other side is written by the
    // call and becomes the reference when the call has succeeded --, and next_track.  The working arrays over n (a
    // labelling may have n bodies), the pass's own sort workspace, the results on the device and in pinned memory
    // (grown on demand, each on its own), the counter block, its pinned copy the call waits for and the one that
    // leaves with the results.
    sph_host::DeviceBuf<uint32_t> trackRow[2];
    sph_host::DeviceBuf<uint2> trackBody[2];
    sph_host::DeviceBuf<unsigned long long> trackId[2];
    sph_host::DeviceBuf<unsigned long long> trackNext;
    int trackRef = 0;
    bool trackHasRef = false;        // a successful call since create / reset
    int trackRefBodies = 0;          // bodies of the reference
    uint64_t trackSequence = 0;      // successful calls since create / reset
    sph_host::DeviceBuf<uint32_t> trackPPrev, trackPCur, trackPCount, trackHead, trackEdgeOf, trackBlockSum, trackParents, trackChildren;
    sph_host::DeviceBuf<unsigned long long> trackBestParent, trackBestChild;
    sph_host::DeviceBuf<uint32_t> trackKeys[2], trackVals[2], trackBlockHist, trackDigitTotal;
    SortWorkspace trackWs{};         // views of the six above
    size_t trackCap = 0;             // particles the buffers above hold
    sph_host::DeviceBuf<SphBodyTrack> trackTracks;
    sph_host::PinnedBuf<SphBodyTrack> trackTracksHost;
    sph_host::DeviceBuf<SphBodyFate> trackFates;
    sph_host::PinnedBuf<SphBodyFate> trackFatesHost;
    sph_host::DeviceBuf<SphBodyEdge> trackEdges;
    sph_host::PinnedBuf<SphBodyEdge> trackEdgesHost;
    size_t trackTracksCap = 0, trackFatesCap = 0, trackEdgesCap = 0; // rows either buffer of a result holds
    sph_host::DeviceBuf<TrackCounters> trackCounters;
    sph_host::PinnedBuf<TrackCounters> trackCountersHost, trackFinalHost;
    sph_host::Event trackCounted;    // the counter block has landed
    int trackBodies = 0, trackPrevious = 0, trackEdgeCount = 0; // of the last sph_track_bodies
    sph_host::Pass track;            // out: the results on their way to the pinned buffers; seconds: the track launches alone
    unsigned long long trackPartialsSum = 0, trackEdgesSum = 0; // sums over calls

    // ---- sph_neighbours.hip ----
    // Neighbour lists (neighbours.hip): the length of every list and the CSR offsets in id order, the scan's block sums,
    // the lists themselves, the two words the call waits for (the total, the longest list), and the pinned copies of
    // offsets and lists; the per-particle buffers and the lists grow on demand, each on its own.
    sph_host::DeviceBuf<uint32_t> nbrCounts, nbrLists;
    sph_host::DeviceBuf<uint64_t> nbrOffsets;
    sph_host::DeviceBuf<unsigned long long> nbrBlockSum, nbrTotals;
    sph_host::PinnedBuf<uint64_t> nbrOffsetsHost;
    sph_host::PinnedBuf<uint32_t> nbrListsHost;
    sph_host::PinnedBuf<unsigned long long> nbrTotalsHost;
    sph_host::Event nbrCounted;      // the two words have landed
    size_t nbrCap = 0;               // particles the per-particle buffers hold
    uint64_t nbrEntryCap = 0;        // entries either list buffer holds
    int nbrN = 0;                    // rows of the last sph_neighbour_lists
    uint64_t nbrEntries = 0, nbrLongest = 0; // ... its total and its longest list
    uint64_t nbrEntriesSum = 0;      // sum over calls
    uint64_t nbrNoOffsets = 0;       // the offsets of a result without particles: {0}
    sph_host::CounterBlock nbrCounters{kNeighbourCounters}; // runs_staged, runs_direct
    sph_host::Pass nbr;              // out: offsets and lists on their way to the pinned buffers; seconds: count + scan + emit + sort

    // ---- sph_pairs.hip ----
    // Pair statistics (pairs.hip): the table of squared edges and the joined rows on the device and in pinned memory
    // (SPH_PAIR_MAX_BINS of each, allocated by the first call), the partial rows (grown on demand) and the default
    // path's tile counter; the three counters.
    sph_host::DeviceBuf<float> pairEdges;
    sph_host::PinnedBuf<float> pairEdgesHost;
    sph_host::DeviceBuf<SphPairBinRaw> pairRows;
    sph_host::PinnedBuf<SphPairBinRaw> pairRowsHost;
    sph_host::DeviceBuf<unsigned long long> pairPartials;
    sph_host::DeviceBuf<unsigned int> pairTile;
    size_t pairPartialCap = 0;       // words pairPartials holds
    int pairBins = 0;                // bins of the last sph_pair_statistics
    int pairCUs = 0;                 // compute units of the device (0: not asked yet)
    sph_host::CounterBlock pairCounters{kPairCounters}; // runs_staged, runs_direct, pairs
    sph_host::Pass pair;             // out: rows and edges on their way to the pinned buffers; seconds: clear + walk + join

    // ---- sph_rays.hip ----
    // Ray casting (rays.hip): the rays and their words on the device and the words in pinned memory, grown on demand by
    // sph_cast_rays; the default path's pair of words per wave (a cast's or a view's, grown on demand) and the two
    // counters they are added up in.
    sph_host::DeviceBuf<SphRay> castRays;
    sph_host::DeviceBuf<unsigned long long> castWords;
    sph_host::PinnedBuf<unsigned long long> castWordsHost;
    sph_host::DeviceBuf<unsigned long long> castPartials;
    size_t castCap = 0, castWaveCap = 0; // rays the three buffers hold / waves castPartials holds
    int castM = 0;                   // rays of the last sph_cast_rays
    sph_host::CounterBlock castCounters{kCastCounters}; // layers, tests (default path)
    sph_host::Pass cast;             // out: the words on their way to castWordsHost; seconds, calls: the casts' kernels
    long long castViews = 0;         // views that ran the cast kernel
    unsigned long long castRaysSum = 0, castPlainTests = 0; // rays of casts and views; rays x particles of the check path's
};

#define HIPCHK(h, call)                                                               \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess) {                                                      \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);            \
            return SPH_EHIP;                                                          \
        }                                                                             \
    } while (0)

// Every entry point that queues work makes the handle's device current first: a host
// thread that drives several GPUs (include/sph_mgpu.h) or switched devices since
// sph_create would otherwise launch on the wrong one.
#define SPH_ON_DEVICE(h)                                                              \
    do {                                                                              \
        int d__ = -1;                                                                 \
        if (hipGetDevice(&d__) != hipSuccess || d__ != (h)->device)                    \
            HIPCHK(h, hipSetDevice((h)->device));                                     \
    } while (0)

namespace sph_host {

// sph_api.hip
int fail(sph_handle *h, int code, const std::string &msg);
// SPH_ESTATE for a single-domain entry point on a slab handle; `hint` ends the message ("" or ": use ...")
int reject_slab_mode(sph_handle *h, const char *hint = ": use the sph_slab_* entry points");
// sph_step.hip
void report_oob(sph_handle *h);
int key_bits(const sph_handle *h);
void state_replaced(sph_handle *h);
SweepArgs make_sweep_args(sph_handle *h);
GatherExtras gather_extras(sph_handle *h);
int tile_chunk(const sph_handle *h, int count, int layers);
int launch_density(sph_handle *h, SweepArgs &A, hipStream_t stream);
int pair_begin(sph_handle *h, double *target, PairEvent **out, hipStream_t stream = nullptr);
int resolve_pair(sph_handle *h, PairEvent &pe);
// seconds and count of the sections timed into *seconds (render, sample), the open ones resolved first; reset: both to zero after
int timed_total(sph_handle *h, double *seconds, long long *count, double *secondsOut, int64_t *countOut, int reset);
// a result leaving on the copy stream: `compute` waits until the last copy has read the device buffer (before it is
// rewritten); the copies are queued behind everything `compute` holds now; the host waits for the last copy
int outbound_fence(sph_handle *h, Outbound &o);
int outbound_send(sph_handle *h, Outbound &o, std::initializer_list<OutboundCopy> copies);
hipError_t outbound_wait(const Outbound &o);
// What the passes over the grid's sorted stream share (the field sample, the surface mesh, the tracers, the derived
// fields, the bodies and their moments, the neighbour lists).  analysis_begin: the state checks, in this order -- a slab handle (`slab_hint` ends that message),
// no state yet, SPH_SWEEP_LINKED, SPH_KEY_MORTON, a phase-split step still open; `what` names the pass in the messages.
// analysis_grid: a grid of the state the handle holds NOW.  Phase 1: it exists (sph_phase_grid, or built ahead by a
// timed step).  Phase 0: the table of the last step is the pre-integration one; the next step's grid is built here,
// ahead, and that step consumes it.  Nothing to build without particles.  A pass checks its own options between the two.
int analysis_begin(sph_handle *h, const char *what, const char *slab_hint);
int analysis_grid(sph_handle *h);
// ... and the stream of that grid, as the passes' kernels read it (all null, n = 0, without particles)
StreamView sorted_stream(const sph_handle *h);
// nothing queued reads or writes the pass's buffers any more: they may be reallocated; the pass holds no result
int pass_quiesce(sph_handle *h, Pass &p);
// a few words the call itself has to wait for (a total that sizes the next launch): copied behind what `compute` holds
// now, waited for through `landed`
int fetch_small(sph_handle *h, void *dst, const void *src, size_t bytes, Event &landed);
int begin_step_events(sph_handle *h);
int build_grid_ahead(sph_handle *h);
int resolve_events(sph_handle *h, StepEvents &se);
void drop_grid_ahead(sph_handle *h);
// a timed section around launch() (void, or an int that ends the call when it is not SPH_OK): its GPU time is added
// to *seconds when resolved; launch errors are reported
template <class F>
int timed_launch(sph_handle *h, double *seconds, F &&launch) {
    PairEvent *pe = nullptr;
    int rc = pair_begin(h, seconds, &pe);
    if (rc) return rc;
    if constexpr (std::is_void_v<decltype(launch())>) launch();
    else if ((rc = launch())) return rc;
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}
// sph_sample.hip: what the field sample and the surface's sample share -- the lattice's checks (a message or null;
// the smallest dimension allowed differs) and its kernel arguments over the stream of the current grid
const char *bad_lattice(int nx, int ny, int nz, const float (&origin)[3], const float (&spacing)[3], int minDim);
SampleArgs lattice_args(const sph_handle *h, int nx, int ny, int nz, const float (&origin)[3], const float (&spacing)[3], int field);
// sph_bodies.hip: all of sph_label_bodies behind its state checks and its options' copy -- the link's check, the
// labelling of the state the handle holds now on either path, the table, the copies, the SphBodyStats accounting.
// `who` names the entry point in the messages.  sph_measure_bodies (sph_body_moments.hip) labels through it too.
int label_bodies(sph_handle *h, float link, const char *who);
// sph_body_moments.hip: what follows the labelling in sph_measure_bodies -- the cap (0: none), the buffers, the moment
// launches over the labelling the handle holds, the copies, the SphBodyMeasureStats accounting.  sph_track_bodies
// (sph_body_tracks.hip) measures through it too.
int measure_labelled(sph_handle *h, uint32_t max_bodies, const char *who);
// sph_rays.hip: what sph_cast_rays and sph_render_view (sph_frame.hip) share -- the spheres' radius of an option (a
// message or null); whether SPH_CAST_PLAIN asks for the check path, which admits `rays` of them or ends the call with
// SPH_EINVAL; the stream, the spheres and the default path's wave words and counters (grown and allocated here) into A,
// whose rays / cam / m are set; the accounting behind a launch
const char *bad_cast_radius(const sph_handle *h, float radius);
int cast_path(sph_handle *h, size_t rays, bool &plain);
int cast_prepare(sph_handle *h, CastArgs &A, float radius, bool plain);
void cast_account(sph_handle *h, const CastArgs &A, bool plain);
// sph_readback.hip
void sdma_init(sph_handle *h);
int sdma_wait(sph_handle *h, int slot);
int sdma_issue(sph_handle *h, int slot);
void sdma_destroy(sph_handle *h);

// rows -> device through the handle's pinned staging halves; `fill(k, dst, count)` packs rows
// [k, k+count) into dst.  Returns when every row is on the device.
constexpr size_t kStageRows = (size_t)1 << 19; // 8 MB per half
template <class Fill>
int staged_upload(sph_handle *h, float4 *dev, size_t n, Fill fill) {
    for (int b = 0; b < 2; ++b) {
        if (!h->stage[b]) HIPCHK(h, h->stage[b].alloc(kStageRows));
        HIPCHK(h, h->stageFree[b].create(hipEventDisableTiming));
    }
    int b = 0;
    for (size_t k = 0; k < n; k += kStageRows, b ^= 1) {
        const size_t cnt = n - k < kStageRows ? n - k : kStageRows;
        HIPCHK(h, hipEventSynchronize(h->stageFree[b])); // (a never-recorded event is complete)
        fill(k, h->stage[b], cnt);
        HIPCHK(h, hipMemcpyAsync(dev + k, h->stage[b], cnt * sizeof(float4), hipMemcpyHostToDevice, h->compute));
        HIPCHK(h, hipEventRecord(h->stageFree[b], h->compute));
    }
    HIPCHK(h, hipStreamSynchronize(h->compute));
    return SPH_OK;
}

// a caller's option struct into `o` (zero: defaults): as many bytes as its struct_size says, at most all of `o`
template <class Opt>
int copy_options(sph_handle *h, const Opt *opt, Opt &o, const char *unset) {
    if (!opt) return SPH_OK;
    if (opt->struct_size <= 0) return fail(h, SPH_EINVAL, unset);
    const size_t sz = (size_t)opt->struct_size;
    memcpy(&o, opt, sz < sizeof o ? sz : sizeof o);
    return SPH_OK;
}

inline bool bad_field(int f) { return f != SPH_FIELD_SPEED && f != SPH_FIELD_DENSITY && f != SPH_FIELD_PRESSURE; }

} // namespace sph_host
