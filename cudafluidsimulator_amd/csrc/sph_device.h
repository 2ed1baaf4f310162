// Internal declarations shared by the HIP translation units of libsph_hip.so.
// gfx950 (MI355X / CDNA4) only: wavefront = 64 lanes is hard-coded throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sph_c_api.h"

#define SPH_WAVE 64

// Physics constants of the reference (simulator.h:6-12, simulator.cu:13-14).
#define SPH_MASS 0.02f
#define SPH_GAS_CONSTANT 1.f
#define SPH_REST_DENSITY 1000.f
#define SPH_VISCOSITY 1.f
#define SPH_GRAVITY -9.8f
#define SPH_ELASTICITY 0.5f
#define SPH_EPS_F (1e-4f)
#define SPH_PUSH_STRENGTH (5.f)
#define SPH_BOX_MAX_X (600)
#define SPH_BOX_MIN_X (200)
#define SPH_BOX_MAX_Y (450)
#define SPH_BOX_MIN_Y (150)

// Run constants, passed to every kernel by value (they land in SGPRs; this
// replaces the reference's `__constant__ Settings deviceSettings`,
// simulator.cu:19,459).
struct DevParams {
    float h;       // smoothing radius = cell size
    float h2;      // h*h, rounded once in fp32 (simulator.cu:89,105)
    float vcoef;   // v_kernel_coeff
    float dcoef;   // d_kernel_coeff
    float boxDim;
    float boxHi;   // boxDim - h in fp32 (simulator.cu:283)
    float dt;      // timestep
    float cut2;    // largest dist2 for which ANY force term can be non-zero
    int D;         // cells per dimension (numCellsPerDim as int)
    int numCells;  // entries of the cell table: D^3 (flattened keys) or 8^ceil(log2 D) (Morton)
    int morton;    // key function: 0 = flattened cell index (simulator.cu:78-82), 1 = Morton
    int slimDiv;   // 1: h and the kernel coefficients are the reference's (main.cpp:57-63): the pair body may use
                   // the divide / square-root chains without range fix-ups (sweep_common.h); 0: full IEEE expansions
};

// The neighbour grid's key function.  Flattened = the reference's x + y D + z D^2; Morton =
// bits of x, y, z interleaved (x lowest), the ordering the reference's README.md:5 names
// for its `z_index_sort` branch (not in the checkout).  SPH_KEY_MORTON exists for the A/B
// of the two orderings and is served by the direct sweep only.
__device__ __forceinline__ uint32_t sph_spread3(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t sph_cell_key(const DevParams &P, int cx, int cy, int cz) {
    if (P.morton) return sph_spread3((uint32_t)cx) | (sph_spread3((uint32_t)cy) << 1) | (sph_spread3((uint32_t)cz) << 2);
    return (uint32_t)(cx + cy * P.D + cz * P.D * P.D);
}

// Reductions over the 64 lanes of a wave (xor butterfly: every lane ends up with the result)
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
    return v;
}
// (64-bit words travel as their 32-bit halves)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// The ordering key of an fp32 bit pattern and its inverse: unsigned keys ascend as the floats do (-0 < +0; a NaN sorts
// where its bits put it), so integer minima and maxima of keys are the floats' (DESIGN.md sections 10c, 10g)
__device__ __forceinline__ uint32_t order_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t order_bits(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// blocks of `per` items that hold n of them
inline int blocks_of(int n, int per) { return (n + per - 1) / per; }

// Particle state lives in two float4 streams, both in cell-sorted order:
//   pos4[i] = (x, y, z, bits(original particle id))
//   vel4[i] = (vx, vy, vz, rho_i)      rho filled by the density sweep
// 32 B per particle instead of the reference's 56-B AoS with a list pointer
// (simulator.h:33-51); a neighbour test touches 16 B.

// Out-of-grid positions met by the cell hash (the reference printf's "OOB particle" from the kernel,
// simulator.cu:60-73): host-mapped, written by the first sort pass, printed by the host.
#define SPH_OOB_RECORDS 8
struct SphOobLog {
    uint32_t count;
    struct { int cell[3]; float pos[3]; } rec[SPH_OOB_RECORDS];
};

// ---- radix sort (sort.hip) ----
struct SortWorkspace {
    uint32_t *keys[2];
    uint32_t *vals[2];
    uint32_t *blockHist;  // [digits <= 1024][numBlocks], digit-major
    uint32_t *digitTotal; // [digits]
    int capacity;         // elements
    int maxBlocks;
    SphOobLog *oob;       // device view of the handle's out-of-grid log (may be null)
    // zero-pair filter (optional): the first pass of a grid build samples 64 rows of velSample[0..n) and leaves the
    // most common velocity in *vrefOut -- the gather launch of the same build marks the rows that move with it
    const float4 *velSample;
    float4 *vrefOut;
};
size_t sph_sort_workspace_blocks(int n);
// Stable LSD sort of (keys[0], vals[0]) on `bits` key bits; returns the index
// (0/1) of the buffer pair that holds the result.
int sph_sort_pairs(const SortWorkspace &ws, int n, int bits, hipStream_t s);
// Same, for the grid build: the keys are the flattened cell indices of pos4[0..n), computed
// inside the first histogram pass (no separate hash kernel, no iota of values in memory);
// that pass also zeroes cellRange[0..numCells) (kernelResetGrid) for k_gather_cells.
int sph_sort_cells(const SortWorkspace &ws, const DevParams &P, const float4 *pos4, int n, int bits,
                   hipStream_t s, int2 *cellRange, int numCells);

// ---- grid build (grid.hip) ----
// bounds[k] = #keys < thr[k] over sorted keys (one binary search per lane)
struct Thresholds { uint32_t v[8]; };
// work that rides on the gather launch instead of a launch of its own (all optional)
struct GatherExtras {
    unsigned long long *cursor = nullptr; // hit-stream allocation cursors to clear ...
    int cursorWords = 0;                  // ... this many 8-byte words
    int *bounds = nullptr;                // slab path: bounds[t] = #keys < thr.v[t], bounds[nthr] = n
    const float4 *vref = nullptr;         // zero-pair filter: the reference velocity (picked by the first sort pass) ...
    unsigned long long *calm = nullptr;   // ... and one bit per sorted row "moves with it", a 64-bit word per 64 rows
    uint32_t *quietAll = nullptr;         // the "every (owned) row is quiet" word and, next to it, the "every halo row is
                                          // quiet" word (slabs) are set to 1 here
    uint32_t *quietClear = nullptr;       // slab path: the filter's bit array is cleared here (halo rows stay "not quiet") ...
    int quietWords = 0;                   // ... this many 32-bit words
    Thresholds thr{};
    int nthr = 0;
};
void sph_launch_gather(const float4 *pos_in, const float4 *vel_in,
                       const uint32_t *perm, const uint32_t *sorted_keys,
                       float4 *pos_out, float4 *vel_out, float4 *pv8, int2 *cellRange, int n,
                       hipStream_t s, const GatherExtras &X = GatherExtras());
void sph_launch_lower_bounds(const uint32_t *sorted_keys, int n, Thresholds thr, int nthr,
                             int *bounds_dev, hipStream_t s);
// stable partition of [0, n) by key class in two launches (tileCount: sph_partition_tiles(n) x 9 ints)
void sph_launch_partition(const DevParams &P, const float4 *pos_in, const float4 *vel_in, float4 *pos_out,
                          float4 *vel_out, Thresholds thr, int nthr, int n, int *tileCount, int *bounds_dev,
                          hipStream_t s);
size_t sph_partition_tiles(int n);
struct SegmentTable {
    const float4 *spos[8];
    const float4 *svel[8];
    int dst[8];
    int prefix[9]; // rows before segment k; prefix[n] = total
    int n;
};
void sph_launch_copy_segments(const SegmentTable &T, float4 *dpos, float4 *dvel, hipStream_t s);
void sph_launch_click(const DevParams &P, const int2 *cellRange, float4 *vel4,
                      int mx, int my, hipStream_t s, int zlo = 0, int zhi = 1 << 30);

// Hit-stream pool of the list sweep: cut into sub-pools with one allocation cursor each
// (one cursor per 256 bytes), see k_density_mask_lds.
#define SL_POOL_SHARDS 64
#define SL_CURSOR_STRIDE 32 // unsigned long long per cursor slot

// ---- sweeps (sweeps.hip) ----
struct SweepArgs {
    const float4 *pos4;       // sorted positions (+id)
    float4 *vel4;             // sorted velocities (+rho): density writes .w
    const int2 *cellRange;    // {start,end} per flattened cell
    const uint32_t *keys;     // sorted flattened cell keys
    float4 *pos_out;          // force+integrate outputs (same sorted index)
    float4 *vel_out;
    float *host_order_pos;    // n x 3 floats by original id (may be null)
    float4 *force_out;        // optional (SPH_FLAG_STORE_FORCE)
    unsigned long long *pairCounter; // optional (SPH_FLAG_COUNT_PAIRS)
    unsigned long long *stampCounter; // unused: no kernel reads it (kept so that the fields after it keep their offsets)
    int i_begin, i_end;       // owned range (whole array for one domain)
    int i_origin;             // list sweep: particle 0 of wave 0 of the hit stream (the density
                              // sweep's i_begin); a force launch may cover a sub-range of it
    int i_begin2, i_end2;     // list sweep force launch: an optional SECOND row range in the same
                              // launch (a slab's two boundary layers: one grid, one tail); empty = {0,0}
    int nblk1;                // ... blocks of the launch that belong to the first range
    int n_all;
    int patchHalo;            // list sweep force launch: copy the halo rows' vel4 into pv8 first
    int tileChunk;            // xcd_tile(): 256-particle tiles per chunk (1/8 z-layer), 0 = eighths
    int tileRotate;           // xcd_tile(): the chunk -> XCD assignment moves on by one every so many groups (0 = fixed)
    // SPH_SWEEP_LIST: hit bit streams handed from the density to the force sweep
    uint32_t *maskPool;               // pool of quads: two (first candidate, 32-bit mask) pairs each
    uint32_t *maskOff;                // per 64-particle wave: {first quad or ~0u, quads per lane}
    uint32_t *hitCount;               // per sorted row: hits the density sweep recorded (the force sweep deals rows to lanes by it)
    unsigned long long *maskCursor;   // quads handed out this step, per sub-pool: [SL_POOL_SHARDS][SL_CURSOR_STRIDE];
                                      // word 1 (cleared with them): waves that found their sub-pool exhausted ...
    uint32_t *noneList;               // ... and their numbers, in arrival order (k_force_fallback walks this list)
    unsigned long long maskCapacity;  // pool size in quads
    float4 *pv8;                      // interleaved (pos4, vel4) copy of the sorted streams
    uint32_t *quiet;                  // zero-pair filter (may be null = off): bit j of this array is set when sorted row j
                                      // has no pressure and moves with the reference velocity *quietVref; a hit between
                                      // two such rows adds exactly +-0 to the force and is dropped unread
    const unsigned long long *calm;   // bit j: sorted row j moves with the reference velocity (written by the gather launch)
    uint32_t *quietAll;               // 1 while EVERY row of this step's density sweep (slabs: every owned row) is quiet -- set by the
                                      // gather launch, cleared by the density sweep's first non-quiet row; the force
                                      // sweep then has no pair to evaluate and does not read its hit stream at all
    const uint32_t *quietHalo;        // slabs, launches that hold rows next to a halo layer (else null): 1 while every
                                      // HALO row of this step is quiet too (k_halo_quiet, after exchange B)
    int rhoToVel4;                    // list sweep: also store rho in vel4.w (slab halo exchange B)
    // SPH_SWEEP_LINKED: per-cell linked lists over the UNSORTED streams
    const int *listHead;              // [numCells] first particle of the cell or -1
    const int *listNext;              // [n] next particle of the same cell or -1
};
void sph_launch_halo_quiet(const float4 *pv8, int lo_end, int hi_begin, int n_all, const float4 *vref,
                           const uint32_t *ownedQuiet, uint32_t *haloQuiet, hipStream_t s);
// ---- linked-list backend (sweeps_linked.hip) ----
void sph_launch_link_build(const DevParams &P, const float4 *pos4, int *head, int *next, int n,
                           hipStream_t s);
void sph_launch_density_linked(const DevParams &P, const SweepArgs &A, hipStream_t s);
void sph_launch_force_linked(const DevParams &P, const SweepArgs &A, hipStream_t s);
void sph_launch_density_list(const DevParams &P, const SweepArgs &A, int mathMode, hipStream_t s);
void sph_launch_force_list(const DevParams &P, const SweepArgs &A, int mathMode, hipStream_t s);
void sph_launch_patch_halo(const SweepArgs &A, hipStream_t s);
void sph_launch_density(const DevParams &P, const SweepArgs &A, int mathMode,
                        int sweep, hipStream_t s);
void sph_launch_force(const DevParams &P, const SweepArgs &A, int mathMode,
                      int sweep, hipStream_t s);

// ---- the visualiser's frame (render.hip; the image is defined in DESIGN.md section 10) ----
struct RenderParams {
    int width, height;
    float Wf, Hf; // width and height as floats
    int radius;   // (point_size - 1) / 2
    int shade;    // SPH_SHADE_*
};
// the static layer: 12 box edges x 4096 samples, minimum depth bits per pixel (clears `edge` first)
void sph_launch_render_edges(const RenderParams &R, uint32_t *edge, hipStream_t s);
// The frame's device buffers, as the four launchers below take them: filled by frame_view() (sph_frame.hip) and by
// nobody else; null while no frame that needs the buffer was asked for
struct FrameView {
    uint32_t *depth, *count;     // per pixel, of the flat and field frames
    const uint32_t *edge;        // the static layer
    uint32_t *rgb;               // 3 bytes per pixel, padded to a multiple of 4 pixels
    unsigned long long *packed;  // per pixel: the field frame's (depth bits << 32 | value bits), the column frame's sum
    uint32_t *range;             // the bits of lo and hi of the colour scale
    unsigned long long *maxWord; // the largest column word
    const float *rays;           // sph_launch_column_rays' table
    uint32_t *smooth[2];         // the liquid frame's ping-pong planes of smoothed depth bits
    float4 *normals;             // ... and its normals
};
// The pixel-centre rays of a width x height image: ax of column c at [c], ay of row r at
// [width + r] (built once per image size, like the edge layer).
void sph_launch_column_rays(const RenderParams &R, float *rays, hipStream_t s);
// Each: clear + splat of pos4[0, n) + compose into V.rgb; plain = the one-atomic-per-hit check path.  Field frame:
// autoRange: min / max of the field (SPH_FIELD_*) over vel4[0, n) into V.range, else the bits of lo / hi; its compose
// also leaves the depth words in V.depth.  Column frame: h, h2, dcoef: the handle's settings; autoRange: from 0 to the
// largest column (V.maxWord), else lo / hi; its compose leaves the bits of the range used in V.range.
void sph_launch_render(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain, hipStream_t s);
void sph_launch_render_field(const RenderParams &R, const FrameView &V, const float4 *pos4, const float4 *vel4, int n, bool plain,
                             int field, bool autoRange, float lo, float hi, hipStream_t s);
void sph_launch_render_column(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain, float h, float h2,
                              float dcoef, bool autoRange, float lo, float hi, hipStream_t s);
// The liquid frame, the options with every default resolved: clears, the sphere splat into
// V.depth, sph_launch_render_column's splat (and maximum, where the thickness scale is automatic) into V.packed, the
// smoothing iterations, compose into V.normals and V.rgb.  Returns the plane that holds the final smoothed depth:
// V.depth where nothing was smoothed, else one of V.smooth.
struct LiquidParams {
    float radius;              // of the spheres, <= h
    float h, h2, dcoef;        // the handle's settings (the column words)
    int smoothIterations, smoothRadius;
    float smoothDepth;
    float light[3];            // not normalised
    bool autoThickness;
    float thickness;           // the scale where not automatic
};
const uint32_t *sph_launch_render_liquid(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain,
                                         const LiquidParams &Q, hipStream_t s);

// The bits of the field frame's scalar of a row, from the (vx, vy, vz, rho) sph_download_state
// reads: what the field frame colours by and the diagnostics reduce.  fp32, every operation rounded on its own.
__device__ __forceinline__ uint32_t field_bits(const float4 v, int field) {
    float s;
    if (field == SPH_FIELD_SPEED) s = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    else if (field == SPH_FIELD_DENSITY) s = v.w;
    else s = fmaxf(0.f, SPH_GAS_CONSTANT * (v.w - SPH_REST_DENSITY)); // as sph_download_state
    return __float_as_uint(s);
}

// (r, g, b) = bytes 0, 1, 2: blue - cyan - green - yellow - red over q = 0..255, integers only
__device__ __forceinline__ uint32_t field_ramp(uint32_t q) {
    if (q < 64u) return ((4u * q) << 8) | 0xFF0000u;
    if (q < 128u) return 0x00FF00u | ((255u - 4u * (q - 64u)) << 16);
    if (q < 192u) return (4u * (q - 128u)) | 0x00FF00u;
    return 0xFFu | ((255u - 4u * (q - 192u)) << 8);
}

// the quantiser of the field and column frames: q = 0..255 of s on the scale lo..hi
__device__ __forceinline__ uint32_t field_quantise(float s, float lo, float hi) {
    uint32_t q = 0u;
    if (hi != lo) {
        const float u = ((s - lo) / (hi - lo)) * 256.f;
        if (u == u) q = (uint32_t)(int)fminf(fmaxf(floorf(u), 0.f), 255.f); // (NaN: q = 0)
    }
    return q;
}

// four pixels = 12 bytes = three dwords per thread (rgb is padded to a multiple of four pixels); colour(p) = 0xBBGGRR of pixel p
template <class Colour>
__device__ __forceinline__ void compose_quad(int npix, uint32_t *__restrict__ rgb, Colour colour) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int p0 = g * 4;
    if (p0 >= npix) return;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = (p0 + k < npix) ? colour(p0 + k) : 0u;
    rgb[g * 3 + 0] = c[0] | (c[1] << 24);
    rgb[g * 3 + 1] = (c[1] >> 8) | (c[2] << 16);
    rgb[g * 3 + 2] = (c[2] >> 16) | (c[3] << 8);
}

// ---- the analysis passes ----
// The cell-sorted stream of the last grid build, as every pass that walks it reads it: sorted row j is
// position(j) = (x, y, z, id) and velocity(j) = (vx, vy, vz, rho).  Two layouts, told apart by the stride alone: the
// sorted pos4 / vel4 streams (stride 1), or -- SPH_SWEEP_LIST, whose gather leaves no sorted vel4 -- the interleaved
// records pv8 (pos = pv8, vel = pv8 + 1, stride 2).  cellRange holds {start, end} per flattened cell
// (SPH_KEY_FLATTENED only).  n == 0: no particle, every pointer null, nothing is walked.  Filled by sorted_stream()
// (sph_step.hip) and by nobody else.
struct StreamView {
    const float4 *pos, *vel;
    int stride;
    const int2 *cellRange;
    int n;
    __device__ __forceinline__ float4 position(int j) const { return pos[(size_t)j * stride]; }
    __device__ __forceinline__ float4 velocity(int j) const { return vel[(size_t)j * stride]; }
};

// ---- the field sample (sample.hip; defined in DESIGN.md section 10b) ----
struct SampleArgs {
    int nx, ny, nz;          // lattice points per axis; point (ix, iy, iz) -> out[(iz ny + iy) nx + ix]
    float ox, oy, oz;        // origin
    float sx, sy, sz;        // spacing
    int field;               // SPH_FIELD_*
    StreamView S;            // the candidates
};
// one value per lattice point into out[0, nx ny nz); plain = the one-thread-per-point check path
void sph_launch_sample(const DevParams &P, const SampleArgs &A, bool plain, float *out, hipStream_t s);

// ---- passive tracers (tracers.hip; defined in DESIGN.md section 10e) ----
struct TracerArgs {
    StreamView S;            // the candidates
    int m;                   // tracers
    float dt;
    float4 *posDen;          // [m] caller order: (x, y, z, den); read, then rewritten in place by the tracer's own lane
    float4 *velOut;          // [m] caller order: (ux, uy, uz, +0)
    uint32_t *keys, *vals;   // [m] default path: k_tracer_keys fills them (cell key, or numCells for a tracer outside; identity)
    const uint32_t *order;   // [m] default path: the sort's values, read by the walk (set by sph_launch_tracers)
    unsigned long long *counters; // [3] waves_shared, waves_direct, groups (default path)
};
constexpr int kTracerCounters = 3;
// key + sort + walk (plain: the one-thread-per-tracer check path alone); `ws` is the tracers' own sort workspace
void sph_launch_tracers(const DevParams &P, TracerArgs A, bool plain, const SortWorkspace &ws, int keyBits, hipStream_t s);

// ---- derived per-particle fields (derived.hip; defined in DESIGN.md section 10f) ----
struct DeriveArgs {
    StreamView S;            // the rows and their candidates, n > 0
    float4 *vortDiv;         // [n] particle-id order: (wx, wy, wz, divergence)
    float4 *gradRho;         // [n] particle-id order: (gx, gy, gz, rho)
    uint32_t *neighbours;    // [n] particle-id order: taken candidates
    unsigned long long *counters; // [2] runs_staged, runs_direct (default path)
};
constexpr int kDeriveCounters = 2;
// one sweep over rows [0, n); plain = the one-thread-per-row check path
void sph_launch_derive(const DevParams &P, const DeriveArgs &A, bool plain, hipStream_t s);

// ---- bodies: connected components of the link graph (bodies.hip; defined in DESIGN.md section 10g) ----
// What one call counts and the few words the host waits for, on the device: every word written by integer atomics
// (or by one thread), cleared by the first launch of a call.
struct BodyCounters {
    unsigned long long links;    // unordered linked pairs
    unsigned long long unions;   // successful merges (default path)
    unsigned long long largest;  // count << 32 | ~label of the body with the greatest count (smallest label on a tie)
    uint32_t numBodies;          // the scan's total
    uint32_t gaveUp;             // lanes that left a bounded loop at its bound (default path; always 0)
    uint32_t changed;            // check path: a row's label went down in this round
    uint32_t pad;
};
struct BodyArgs {
    StreamView S;            // the rows and their candidates, n > 0 (the velocities are not read)
    float r2;                // link length squared, rounded once
    uint32_t *parent;        // [n] default path: the union-find forest over rows; parent[i] <= i always
    uint32_t *root;          // [n] default path: the root of every row, written by the flatten launch
    uint32_t *rootId;        // [n] default path: per root the smallest particle id of its tree
    uint32_t *rowLabel;      // [n] the label of every row (check path: propagated in place)
    uint32_t *flag;          // [n] per particle id: 1 = it is a label
    uint32_t *rank;          // [n] per particle id: labels below it (exclusive scan of flag)
    uint32_t *blockSum;      // [sph_body_scan_blocks(n)] the scan's per-block sums, then offsets
    uint32_t *labels;        // [n] particle-id order: the result
    uint32_t *table;         // [8 numBodies] the result (table launches only)
    BodyCounters *counters;
};
int sph_body_scan_blocks(int n);
// default path: clear + link sweep + flatten + label + mark + scan, which leaves counters->numBodies
void sph_launch_bodies_unite(const DevParams &P, const BodyArgs &A, hipStream_t s);
// check path: clear (rowLabel = particle id); one round of min-label propagation (first: also counts the links),
// which sets counters->changed; mark + scan after the last round
void sph_launch_bodies_plain_begin(const BodyArgs &A, hipStream_t s);
void sph_launch_bodies_plain_round(const DevParams &P, const BodyArgs &A, bool first, hipStream_t s);
void sph_launch_bodies_plain_end(const BodyArgs &A, hipStream_t s);
// both paths: the table of numBodies rows, labels in id order, counters->largest
void sph_launch_bodies_table(const BodyArgs &A, int numBodies, hipStream_t s);

// ---- per-body moments (body_moments.hip; defined in DESIGN.md section 10k) ----
// A body's row is kBodyMomentStride 64-bit words, on the device and as SphBodyMomentsRaw.  While the rows are reduced
// it holds the accumulators -- [0, 18) the sums of the terms' low words, [18, 36) of their arithmetic high words, [36]
// the saturation count --, written by integer atomics only; the finish launch rewrites it in place as the raw row.
constexpr int kBodyMomentWords = 2 * SPH_BODY_SUMS + 1; // 37
constexpr int kBodyMomentStride = 38;
struct BodyMomentArgs {
    StreamView S;                 // the rows, n > 0
    const uint32_t *rowLabel;     // [n] the labelling's label of every row ...
    const uint32_t *rank;         // [n] ... its table row per label ...
    const uint32_t *table;        // [8 numBodies] ... and the table itself (label, count, ...)
    int numBodies;                // > 0
    unsigned long long *rows;     // [kBodyMomentStride numBodies] the result
    uint32_t *sizeHist;           // [SPH_BODY_SIZE_BINS] the result
};
// clear + reduce + finish; plain = the one-thread-per-row, one-atomic-per-word check path
void sph_launch_body_moments(const BodyMomentArgs &A, bool plain, hipStream_t s);

// ---- body tracks: the overlap of two labellings (body_tracks.hip; defined in DESIGN.md section 10l) ----
// What one call counts, on the device: cleared by the first launch of a call, the two words the host waits for
// (partials, edges) and what leaves with the results.
struct TrackCounters {
    unsigned long long nextTrack; // after the call (k_track_close)
    uint32_t partials;            // partial edges (the fold's appends; check path: n)
    uint32_t edges;               // the heads' scan total
    uint32_t continued, born, ended, merges, splits;
    uint32_t pad;
};
struct TrackArgs {
    StreamView S;                 // the rows, n > 0 (the fold reads the ids alone)
    const uint32_t *rowLabel;     // [n] the labelling's label of every row ...
    const uint32_t *rank;         // [n] ... its table row per label ...
    const uint32_t *labels;       // [n] ... the labels in particle-id order ...
    const uint32_t *table;        // [8 numBodies] ... and the table
    int numBodies;                // > 0
    int numPrev;                  // bodies of the reference; 0: there is none, and the three below are not read
    const uint32_t *prow;         // [n] the reference: the table row of every particle id's body ...
    const uint2 *prevBody;        // [numPrev] ... (label, count) of its bodies ...
    const unsigned long long *prevTrack; // [numPrev] ... and their tracks
    uint32_t *crow;               // [n] the same three of this labelling: the next reference once the call has succeeded
    uint2 *curBody;               // [numBodies]
    unsigned long long *curTrack; // [numBodies]
    unsigned long long *nextTrack; // the handle's next_track, on the device
    uint32_t *pPrev, *pCur, *pCount; // [n] the partial edges, in arrival order (check path: pCount holds the heads' positions)
    uint32_t *head;               // [n] per sorted partial: 1 = first of its pair; then per body: 1 = born
    uint32_t *edgeOf;             // [n] the exclusive scan of head; then of the born flags
    uint32_t *blockSum;           // [sph_track_scan_blocks(n)] the scans' per-block sums, then offsets
    SortWorkspace ws;             // the pass's own, capacity n
    uint32_t *parents, *children; // [numBodies], [numPrev] edges into / out of a body
    unsigned long long *bestParent, *bestChild; // count << 32 | ~row of the main parent / child
    SphBodyEdge *edges;           // [edges] the results
    SphBodyTrack *tracks;         // [numBodies]
    SphBodyFate *fates;           // [numPrev]
    TrackCounters *counters;
};
int sph_track_scan_blocks(int n);
// clear + one thread per particle id (crow; on the check path also the partial edges) + (default path) the fold: the
// partial edges and counters->partials
void sph_launch_track_partials(const TrackArgs &A, bool plain, hipStream_t s);
// the two stable sorts of m partials + heads + scan, which leaves counters->edges; returns which of ws.vals holds the order
int sph_launch_track_sort(const TrackArgs &A, int m, hipStream_t s);
// the edges' rows, counts and the per-body tallies from the m sorted partials (order: ws.vals[order])
void sph_launch_track_edges(const TrackArgs &A, int m, int numEdges, int order, bool plain, hipStream_t s);
// both paths: continues or born, tracks, fates, edge flags, the summary's counters, nextTrack
void sph_launch_track_assign(const TrackArgs &A, int numEdges, hipStream_t s);

// ---- neighbour lists: every particle's neighbours within a radius, as CSR (neighbours.hip) ----
struct NeighbourArgs {
    StreamView S;            // the rows and their candidates, n > 0 (the velocities are not read)
    float r2;                // radius squared, rounded once
    uint32_t *counts;        // [n] particle-id order: the length of every list
    uint64_t *offsets;       // [n + 1] particle-id order: the exclusive scan of counts, then the total
    uint32_t *neighbours;    // [total] the lists (emit and sort launches only)
    unsigned long long *blockSum; // [sph_neighbour_scan_blocks(n)] the scan's per-block sums, then offsets
    unsigned long long *totals;   // [2] the total (left by the scan) and the longest list (left by the count): what the host waits for
    unsigned long long *counters; // [2] runs_staged, runs_direct (default path; both walks add to them)
};
constexpr int kNeighbourCounters = 2;
int sph_neighbour_scan_blocks(int n);
// Four launches; plain = the check path (one thread per row, one thread per list).  count: clears totals, fills
// counts and totals[1].  scan: offsets[0, n] and totals[0] from counts.  emit: the walk again, every taken candidate's
// id to its list, in walk order.  sort: every list ascending, in place.
void sph_launch_neighbour_count(const DevParams &P, const NeighbourArgs &A, bool plain, hipStream_t s);
void sph_launch_neighbour_scan(const NeighbourArgs &A, hipStream_t s);
void sph_launch_neighbour_emit(const DevParams &P, const NeighbourArgs &A, bool plain, hipStream_t s);
void sph_launch_neighbour_sort(const NeighbourArgs &A, bool plain, hipStream_t s);

// ---- pair statistics: per bin of separation the pairs and four exact sums (pairs.hip) ----
// A partial row holds kPairWords words per bin, word-major (word w of bin b at [w bins + b]): the count, the four sums'
// low words, their high words, the saturation count, and the four sums' top words (what a high word sheds before it
// could wrap); the sum is lo + hi 2^32 + top 2^64.
constexpr int kPairCount = 0, kPairLo = 1, kPairHi = 5, kPairSat = 9, kPairTop = 10, kPairWords = 14;
constexpr int kPairLdsWords = kPairTop; // what the default path keeps in LDS: everything but the top words
constexpr int kPairMaxN = 1 << 24;      // the default path's bound on n (pairs.hip says why)
struct PairEdges {
    float e[SPH_PAIR_MAX_BINS];
};
struct PairArgs {
    StreamView S;            // the rows and their candidates, n > 0
    float r2;                // radius squared, rounded once: the last edge
    float perRadius;         // bins / radius: where the default path starts its search of the table
    int bins;
    const float *edges2;     // [bins] squared outer edges, non-decreasing (left by sph_launch_pair_table)
    unsigned long long *partials; // [rows][kPairWords bins] one row per workgroup of the default path; the check path's one row
    int rows;
    unsigned int *tile;      // the default path's tile counter
    long long shed;          // the default path: a hi word at or beyond +-shed sheds into its top word; 2^33 .. 2^62
    SphPairBinRaw *out;      // [bins] the joined table
    unsigned long long *counters; // [3] runs_staged, runs_direct (default path), the tables' pairs (the join)
};
constexpr int kPairCounters = 3;
// workgroups the default path launches on a device of `cus` compute units for n rows (= partial rows; the check path: 1);
// workgroups > 0: that many instead (SPH_PAIRS_WORKGROUPS), never more than tiles
int sph_pair_rows(int n, int cus, bool plain, int workgroups);
// the edges into device memory and an all-zero table (what a call without particles returns)
void sph_launch_pair_table(const PairEdges &E, const PairArgs &A, hipStream_t s);
// clear + walk + join; plain = the check path
void sph_launch_pair_statistics(const DevParams &P, const PairArgs &A, bool plain, hipStream_t s);

// ---- ray casting and the view frame (rays.hip; defined in DESIGN.md section 10n) ----
// The view's camera with every default resolved: the basis computed by the host, passed as data
struct ViewCamera {
    float eye[3], fwd[3], s[3], u[3];
    float tanX, tanY, tNear, tFar;
    int width, height;
    float Wf, Hf;
};
struct CastArgs {
    StreamView S;            // the candidates
    float r, r2;             // of the spheres; r r, rounded once
    const SphRay *rays;      // [m] a batch in the caller's order, or null: the pixel-centre rays of `cam`
    int m;                   // rays (a view: width x height)
    ViewCamera cam;
    unsigned long long *words; // [m] the result (a view: pixel (c, row) at [row width + c])
    uint32_t *rows;          // [m] a view: the winner's row of the stream (0 for a miss: read for hits only); a batch: null
    unsigned long long *partials; // [2 sph_cast_waves] default path: layers and tests of every wave ...
    unsigned long long *counters; // [2] ... added up here behind the walk: layers, tests
};
constexpr int kCastCounters = 2;
// waves of the default path's launch: 64 rays of a batch, an 8 x 8 tile of a view each
int sph_cast_waves(const CastArgs &A);
// one word per ray; plain = the one-thread-per-ray check path over every row
void sph_launch_cast(const DevParams &P, const CastArgs &A, bool plain, hipStream_t s);
// The view's picture from its words: shade: SPH_VIEW_*; range: the bits of lo / hi of a field
// shade's scale; light: not normalised; edgeRadius < 0: no edges
struct ViewShade {
    int shade;
    float light[3];
    float edgeRadius;
    const uint32_t *range;
};
void sph_launch_view_compose(const DevParams &P, const CastArgs &A, const ViewShade &V, uint32_t *rgb, hipStream_t s);
// the bits of lo / hi of the field frame's colour scale into range[0..1]: the given ones, or (autoRange, n > 0) the
// minimum and maximum of the field over vel4[0, n) (render.hip: the field frame's reduction)
void sph_launch_field_range(const float4 *vel4, int n, int field, bool autoRange, float lo, float hi, uint32_t *range, hipStream_t s);

// ---- the surface mesh (surface.hip; defined in DESIGN.md section 10d) ----
struct SurfaceArgs {
    int nx, ny, nz;          // lattice points per axis, each >= 2; point (ix, iy, iz) has L = (iz ny + iy) nx + ix
    float ox, oy, oz;        // origin
    float sx, sy, sz;        // spacing
    float iso;
};
struct SurfaceBuffers {
    const float *field;          // [points] the density sample of the lattice
    uint8_t *bits;               // [points] bit k: corner k of the point's cell is inside (a corner off the lattice: 0)
    uint32_t *local;             // [points] vertices (low half) and triangles (high half) before the point in its block,
                                 // written where the point owns a vertex
    uint2 *blockSum, *blockOff;  // [sph_surface_blocks] (vertices, triangles) of a block, and before it
    unsigned long long *totals;  // [2] vertices, triangles of the mesh
};
// blocks of the counting launch
int sph_surface_blocks(const SurfaceArgs &A);
// classify + count + scan: fills bits, local, blockSum, blockOff and totals from field
void sph_launch_surface_count(const SurfaceArgs &A, bool plain, const SurfaceBuffers &B, hipStream_t s);
// 3 floats per vertex into verts, 3 indices per triangle into tris, as many as *totals says
void sph_launch_surface_emit(const SurfaceArgs &A, bool plain, const SurfaceBuffers &B, float *verts, uint32_t *tris, hipStream_t s);

// ---- diagnostics (diag.hip; defined in DESIGN.md section 10c) ----
// The result block on the device: every word an integer, written by integer atomics only.
struct DiagBlock {
    unsigned long long lo[SPH_DIAG_SUMS]; // sum of q & 0xFFFFFFFF per sum
    long long hi[SPH_DIAG_SUMS];          // sum of q >> 32 (arithmetic)
    unsigned long long saturated;
    uint32_t minKey[SPH_DIAG_EXTREMA];    // ordering keys, not bit patterns (identities: 0xFFFFFFFF / 0)
    uint32_t maxKey[SPH_DIAG_EXTREMA];
    uint32_t range[2];                    // bits of the histogram's lo / hi (given, or filled in from the keys)
    uint32_t pad[2];
    unsigned long long hist[SPH_DIAG_BINS];
};
struct DiagArgs {
    const float4 *pos;  // row j: pos[j stride] = (x, y, z, id) and vel[j stride] = (vx, vy, vz, rho)
    const float4 *vel;
    int stride;
    int n;              // rows
    int histField;      // SPH_FIELD_*, -1 = no histogram
    int autoRange;      // the histogram's range is the reduced minimum / maximum of its scalar
    float lo, hi;       // ... else this one
};
// clear + reduce (+ histogram) into *blk; plain = the one-thread-per-row, one-atomic-per-term check path
void sph_launch_diagnose(const DiagArgs &A, bool plain, DiagBlock *blk, hipStream_t s);
