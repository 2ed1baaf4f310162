// What the analysis passes' kernels share (sample.hip, tracers.hip, derived.hip, bodies.hip, neighbours.hip, pairs.hip): the walks of a
// StreamView (sph_device.h) around a point or a row.  sweep_common.h stays the step's; from it come only sweep_cell and
// load_runs.  Every function is __forceinline__ and none holds a barrier -- those stay in the kernels, in plain sight --
// but one: walk_runs_staged, the staged walk of a row's nine runs, whose two barriers and the wave-uniform conditions
// around them (which runs are skipped, which walk from global memory, how many trips a run takes) are one unit that
// its two kernels must not hold in two copies.
//
// Selected terms.  The wave-shared walks read and compute unconditionally and SELECT what they add: take ? term : 0.f,
// never a product with a mask, because the term of a candidate that is not taken is garbage of either sign.  Adding the
// selected +0.f changes no bit: a float sum that starts at +0.f is never -0.f under round-to-nearest (x + y is -0 only
// when both are, an exact cancellation gives +0), although the terms may be signed.  So a walk that adds +0.f for the
// candidates it does not take gives the words of the walk that skips them.
#pragma once

#include "sweep_common.h"

// on the lambdas handed to the walks below: their bodies are inlined as early as the walks themselves
#define WALK_LAMBDA __attribute__((always_inline))

// the cell of a coordinate, (int)(p / h) like the cell hash, or -1 for a point outside the grid
// (the range tests come before the conversion: a float beyond the int range must not reach it)
__device__ __forceinline__ int point_cell(const DevParams &P, float p) {
    if (!(p >= 0.f)) return -1;
    const float q = p / P.h;
    if (!(q < (float)P.D)) return -1; // (int)q >= D
    return (int)q;
}

// The kernel weight of a candidate at squared distance d2: m = MASS (dcoef diff^3) with diff = h2 - d2, rounded in
// this order; a = dcoef diff^2 on its own for the gradient terms; taken = within h (false beyond it, true for a NaN,
// as the definitions have it).  m and a of a candidate that is not taken are garbage.
struct Poly6 {
    float a, m;
    bool taken;
};
__device__ __forceinline__ Poly6 poly6_mass(const DevParams &P, float d2) {
    Poly6 K;
    K.taken = !(d2 > P.h2);
    const float diff = P.h2 - d2;
    K.a = (P.dcoef * diff) * diff;
    K.m = SPH_MASS * (K.a * diff);
    return K;
}

// the link test of the bodies, the neighbour lists and the pair statistics (DESIGN.md sections 10g, 10j, 10m): c is the
// candidate, pi the row; link_d2 is the squared distance the test compares, for the pass that also bins it
__device__ __forceinline__ float link_d2(const float4 pi, const float4 c) {
    const float ex = c.x - pi.x, ey = c.y - pi.y, ez = c.z - pi.z;
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ bool linked(const float4 pi, const float4 c, float r2) {
    return link_d2(pi, c) <= r2; // (false for a NaN)
}

// the nine runs of the row at pi (load_runs around sweep_cell of its position), clipped to the stream
__device__ __forceinline__ void clipped_runs(const DevParams &P, const StreamView &S, const float4 pi, bool valid, int (&js)[9],
                                             int (&je)[9]) {
    load_runs(P, S.cellRange, sweep_cell(P, pi.x, pi.y, pi.z), valid, js, je);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        js[r] = max(js[r], 0);
        je[r] = min(je[r], S.n);
    }
}

// the direct walk of a point inside the grid: f(j) for every row j of the 27 cells around (cx, cy, cz), z outermost,
// each cell's run in stream order
template <class F>
__device__ __forceinline__ void for_each_candidate_27(const DevParams &P, const StreamView &S, int cx, int cy, int cz, F f) {
#pragma unroll
    for (int dz = -1; dz < 2; ++dz) {
        const int sz = cz + dz;
        if (sz < 0 || sz >= P.D) continue;
#pragma unroll
        for (int dy = -1; dy < 2; ++dy) {
            const int sy = cy + dy;
            if (sy < 0 || sy >= P.D) continue;
#pragma unroll
            for (int dx = -1; dx < 2; ++dx) {
                const int sx = cx + dx;
                if (sx < 0 || sx >= P.D) continue;
                const int2 run = S.cellRange[(sz * P.D + sy) * P.D + sx];
                for (int j = max(run.x, 0); j < min(run.y, S.n); ++j) f(j);
            }
        }
    }
}

// the direct walk of a row: f(j) for every row j of its nine clipped runs, each in stream order
template <class F>
__device__ __forceinline__ void for_each_row_candidate(const int (&js)[9], const int (&je)[9], F f) {
#pragma unroll
    for (int r = 0; r < 9; ++r)
        for (int j = js[r]; j < je[r]; ++j) f(j);
}

// A lane's window [ws, we) of the stream in the row of cells (sy, sz): the cells cx - 1 .. cx + 1 are one contiguous
// run (flattened keys: x is the fastest axis; empty cells hold {0, 0} and add nothing).  Empty -- ws > we -- for a
// lane that is not active.
__device__ __forceinline__ void lane_window(const DevParams &P, const StreamView &S, int sy, int sz, int cx, bool active, int &ws,
                                            int &we) {
    ws = 0x7fffffff, we = 0;
    if (active) {
        const int2 *cells = S.cellRange + (sz * P.D + sy) * P.D;
        for (int sx = max(cx - 1, 0); sx <= min(cx + 1, P.D - 1); ++sx) {
            const int2 run = cells[sx];
            if (run.y > run.x) {
                ws = min(ws, run.x);
                we = max(we, run.y);
            }
        }
    }
}

// the stretch a wave stages: from its first window's start to its last one's end, clipped to the stream; wave-uniform
__device__ __forceinline__ void wave_hull(int ws, int we, int n, int &s0, int &s1) {
    s0 = max(__builtin_amdgcn_readfirstlane(wave_min_i32(ws)), 0);
    s1 = min(__builtin_amdgcn_readfirstlane(wave_max_i32(we)), n);
}

// The read side of a staged walk.  A one-wave workgroup has copied `cnt` candidates (wave-uniform, at most the chunk, a
// multiple of 4 slots allocated) of kRecord float4 each into `cand` (LDS), between two barriers of its own; every lane
// now reads every one of them (one LDS address per read: a broadcast), in stream order and four to a round, so that
// the reads of a round are in flight together, and hands each to take(words, mine), mine = the candidate lies in
// the lane's own window [lo, hi) of the chunk's slots (clipped here).  take() must select, not branch (see the top of
// this file).  Slots past cnt hold stale rows: they lie outside every window.
// (The write side stays in the kernels.  Behind a functor the 32-byte records' copy, ((t & 1) ? vel : pos)[...], makes
// the compiler pick the pointer by a load inside the loop or keep the closure in scratch memory.)
template <int kRecord, class Take>
__device__ __forceinline__ void take_staged(const float4 *cand, int cnt, int lo, int hi, Take take) {
    lo = max(lo, 0), hi = min(hi, cnt);
    for (int k = 0; k < cnt; k += 4) {
        float4 c[4][kRecord];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int w = 0; w < kRecord; ++w) c[u][w] = cand[kRecord * (k + u) + w];
#pragma unroll
        for (int u = 0; u < 4; ++u) take(c[u], k + u >= lo && k + u < hi);
    }
}

// The staged walk of 64 consecutive rows' nine runs by a one-wave workgroup (k_derive_wave, k_nbr_wave): lane l holds
// the clipped runs js / je of its row.  For each of the nine runs the UNION [u0, u1) of the lanes' ranges is copied into
// `slice` (LDS, kSlice records of kRecord float4: 1 = the position words, 2 = position and velocity) between two
// barriers, and every lane walks its own range from there, kTrip candidates to a trip: take(record, mine), mine = the
// slot is in the lane's range.  The reads are unconditional -- a lane whose range is exhausted reads the union's last
// record again and stays in the trip -- so take() must select, not branch (the top of this file).  A run whose union is
// longer than the slice is walked by every lane from global memory in the same order: directFn(j).  staged / direct
// count the runs of either kind.  Everything that decides whether a barrier is reached -- the ballot, u0, u1, the trip
// count -- is wave-uniform (readfirstlane), and a workgroup is one wave.
// (The copy is picked by the record width here, not handed in: see take_staged.)
template <int kRecord, int kSlice, int kTrip, class Direct, class Take>
__device__ __forceinline__ void walk_runs_staged(const StreamView &S, const int (&js)[9], const int (&je)[9], float4 (&slice)[kRecord * kSlice],
                                                 uint32_t &staged, uint32_t &direct, Direct directFn, Take take) {
    static_assert(kRecord == 1 || kRecord == 2, "position words, or position and velocity");
    const int lane = threadIdx.x;
    // (32-byte records: a lane copies words t = lane, lane + 64, ... of a slice, all of its own parity: one stream,
    // picked once -- picked per word inside the copy loop, the pointer came from the kernel's arguments by a load per trip)
    [[maybe_unused]] const float4 *half = (lane & 1) ? S.vel : S.pos;
    // one copy of the loop body (not nine): r is wave-uniform, picking this run's bounds is 16 conditional moves
#pragma unroll 1
    for (int r = 0; r < 9; ++r) {
        int jsr = js[0], jer = je[0];
#pragma unroll
        for (int q = 1; q < 9; ++q) {
            jsr = (r == q) ? js[q] : jsr;
            jer = (r == q) ? je[q] : jer;
        }
        const bool nonempty = jer > jsr;
        if (!__ballot(nonempty)) continue;
        // the stretch of the stream the wave needs for this run: [u0, u1), the same in every lane
        const int u0 = __builtin_amdgcn_readfirstlane(wave_min_i32(nonempty ? jsr : 0x7fffffff));
        const int u1 = __builtin_amdgcn_readfirstlane(wave_max_i32(nonempty ? jer : 0));
        const int len = u1 - u0;
        if (len > kSlice) {
            direct += 1;
            for (int j = jsr; j < jer; ++j) directFn(j);
            continue;
        }
        staged += 1;
        if constexpr (kRecord == 2) {
            // 32 bytes per candidate; with the interleaved records (vel = pos + 1, stride 2) a plain copy
            for (int t = lane; t < 2 * len; t += 64) slice[t] = half[(size_t)(u0 + (t >> 1)) * S.stride];
        } else {
            for (int t = lane; t < len; t += 64) slice[t] = S.position(u0 + t);
        }
        __syncthreads();
        // this lane's range in slots of the slice, [a, b) within [0, len); every read is clamped to slot len - 1
        const int a = nonempty ? jsr - u0 : 0, b = nonempty ? jer - u0 : 0;
        const int trips = __builtin_amdgcn_readfirstlane(wave_max_i32(b - a));
        for (int k = 0; k < trips; k += kTrip) {
            float4 c[kTrip][kRecord];
#pragma unroll
            for (int u = 0; u < kTrip; ++u) {
                const int slot = min(a + k + u, len - 1);
#pragma unroll
                for (int w = 0; w < kRecord; ++w) c[u][w] = slice[kRecord * slot + w];
            }
#pragma unroll
            for (int u = 0; u < kTrip; ++u) take(c[u], a + k + u < b);
        }
        __syncthreads(); // the slice has been read: the next run may overwrite it
    }
}
