// Passive tracers: points the caller seeds, carried by the SPH-interpolated velocity of the
// state, one explicit Euler move per call.  Every operation below is fp32 and rounded on its own
// (-ffp-contract=off), in the order that section gives, whatever the handle's math mode.
//
// A tracer walks the 27 cells around its own like a lattice point of the field sample (sample.hip) does, but the
// tracers of a wave share their candidates only where the caller put them close together.  The default path
// therefore sorts the tracers by cell key first and hands 64 consecutive tracers of the sorted order to one wave.
// Tracers of one GROUP -- the same (cy, cz) row of cells and the same block of 8 cells in x -- share candidates the
// way the lanes of k_sample_tile do: for each of the nine (y, z) rows of cells the three cells of every lane are one
// contiguous run of the stream, the wave stages the hull of those runs in LDS and every lane reads every staged
// candidate by broadcast.  A lane TAKES candidate k only if k lies in its own run and the lane belongs to the group
// being walked (integer compares); the distance test alone would not do, for the reason sample.hip's header gives.
// A candidate that is not taken adds a selected +0.f, which changes no bit although the m v terms are signed
// (walk_common.h).  The wave loops over its groups wave-uniformly; a lane's whole walk happens
// inside its own group's iteration, so its order is the definition's.  A wave whose lanes fall into more than
// kTracerMaxGroups groups walks the direct way, every lane its own 27 cells from global memory: the shared walk
// serialises over groups, and 64 lone tracers would cost 64 shared walks.
#include "walk_common.h"

namespace {

// (A/B builds for scripts/studies/tracers.py: make variant EXTRA=-DTRACER_MAX_GROUPS=... ; the defaults are the
// measured choices of DESIGN.md section 10e)
#ifndef TRACER_CHUNK
#define TRACER_CHUNK 256
#endif
#ifndef TRACER_BLOCK_X
#define TRACER_BLOCK_X 8
#endif
#ifndef TRACER_MAX_GROUPS
#define TRACER_MAX_GROUPS 4
#endif
constexpr int kTracerChunk = TRACER_CHUNK;     // candidates per LDS chunk: 8 KB of 32-byte records (a multiple of 4: rounds of four)
constexpr int kTracerBlockX = TRACER_BLOCK_X;  // cells in x per group (a power of two)
static_assert(kTracerChunk % 4 == 0 && (kTracerBlockX & (kTracerBlockX - 1)) == 0, "see above");
constexpr int kTracerMaxGroups = TRACER_MAX_GROUPS; // G: a wave with more groups than this walks the direct way
constexpr int kNoGroup = 0x7fffffff;

// one candidate, c = (x, y, z, .), v = (vx, vy, vz, .): the definition written down
__device__ __forceinline__ void tracer_add(const DevParams &P, float px, float py, float pz, const float4 c, const float4 v,
                                           float &den, float &nx, float &ny, float &nz) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const Poly6 K = poly6_mass(P, (dx * dx + dy * dy) + dz * dz);
    if (!K.taken) return;
    den += K.m;
    nx += K.m * v.x;
    ny += K.m * v.y;
    nz += K.m * v.z;
}

// the same with selected terms: a candidate that is not taken, or lies beyond h, adds +0 to all four sums
__device__ __forceinline__ void tracer_add(const DevParams &P, float px, float py, float pz, const float4 c, const float4 v,
                                           bool take, float &den, float &nx, float &ny, float &nz) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const Poly6 K = poly6_mass(P, (dx * dx + dy * dy) + dz * dz);
    take = take && K.taken;
    den += take ? K.m : 0.f;
    nx += take ? K.m * v.x : 0.f;
    ny += take ? K.m * v.y : 0.f;
    nz += take ? K.m * v.z : 0.f;
}

// the direct walk of one tracer inside the grid: 27 cells of global loads (the check path, and the waves of the
// default path that hold too many groups)
__device__ __forceinline__ void tracer_walk_direct(const DevParams &P, const TracerArgs &A, float px, float py, float pz, int cx,
                                                   int cy, int cz, float &den, float &nx, float &ny, float &nz) {
    for_each_candidate_27(P, A.S, cx, cy, cz, [&](int j) WALK_LAMBDA { tracer_add(P, px, py, pz, A.S.position(j), A.S.velocity(j), den, nx, ny, nz); });
}

// velocity, move and the two stores of tracer idx; p holds its position words as they were loaded
__device__ __forceinline__ void tracer_finish(const TracerArgs &A, uint32_t idx, float4 p, float den, float nx, float ny, float nz) {
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (den > 0.f) {
        u.x = nx / den, u.y = ny / den, u.z = nz / den;
        if (A.dt != 0.f) p.x = p.x + u.x * A.dt, p.y = p.y + u.y * A.dt, p.z = p.z + u.z * A.dt;
    }
    p.w = den;
    A.posDen[idx] = p;
    A.velOut[idx] = u;
}

// the check path (SPH_TRACER_PLAIN=1, and every call on a state without particles): one thread per tracer in caller order
__global__ __launch_bounds__(256) void k_tracer_plain(DevParams P, TracerArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.m) return;
    const float4 p = A.posDen[i];
    const int cx = point_cell(P, p.x), cy = point_cell(P, p.y), cz = point_cell(P, p.z);
    float den = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (A.S.n > 0 && cx >= 0 && cy >= 0 && cz >= 0) tracer_walk_direct(P, A, p.x, p.y, p.z, cx, cy, cz, den, nx, ny, nz);
    tracer_finish(A, (uint32_t)i, p, den, nx, ny, nz);
}

// sort key and value of every tracer: its flattened cell key, or numCells (behind every cell) for one outside
__global__ __launch_bounds__(256) void k_tracer_keys(DevParams P, TracerArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.m) return;
    const float4 p = A.posDen[i];
    const int cx = point_cell(P, p.x), cy = point_cell(P, p.y), cz = point_cell(P, p.z);
    const bool inside = cx >= 0 && cy >= 0 && cz >= 0;
    A.keys[i] = inside ? (uint32_t)((cz * P.D + cy) * P.D + cx) : (uint32_t)P.numCells;
    A.vals[i] = (uint32_t)i;
}

// One wave per 64 consecutive tracers of the sorted order.
__global__ __launch_bounds__(64) void k_tracer_walk(DevParams P, TracerArgs A) {
    __shared__ float4 cand[2 * kTracerChunk];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    uint32_t idx = i < A.m ? A.order[i] : 0xffffffffu;
    const bool valid = idx < (uint32_t)A.m; // (the sort's values are a permutation of [0, m): never false for i < m)
    if (!valid) idx = 0;
    const float4 p = valid ? A.posDen[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int cx = point_cell(P, p.x), cy = point_cell(P, p.y), cz = point_cell(P, p.z);
    const bool inside = valid && cx >= 0 && cy >= 0 && cz >= 0;
    const int gkey = inside ? (cz * P.D + cy) * P.D + (cx & ~(kTracerBlockX - 1)) : kNoGroup;
    // The groups of this wave.  The lanes are sorted by cell key, the group key is monotone in it: a group begins
    // where the key differs from the lane before.
    const int before = __shfl_up(gkey, 1);
    const unsigned long long heads = __ballot(inside && (lane == 0 || gkey != before));
    const int groups = __popcll(heads);
    const bool shared = groups <= kTracerMaxGroups; // (wave-uniform)
    if (lane == 0) {
        atomicAdd(&A.counters[shared ? 0 : 1], 1ull);
        if (groups) atomicAdd(&A.counters[2], (unsigned long long)groups);
    }
    float den = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (!shared) {
        if (inside) tracer_walk_direct(P, A, p.x, p.y, p.z, cx, cy, cz, den, nx, ny, nz);
    } else {
        bool open = inside;
        for (;;) {
            // the smallest group key among the lanes still open: the same in every lane, so the branches and the
            // barriers below are wave-uniform
            const int g = __builtin_amdgcn_readfirstlane(wave_min_i32(open ? gkey : kNoGroup));
            if (g == kNoGroup) break;
            const bool act = open && gkey == g;
            open = open && !act;
            const int row = g / P.D, gy = row % P.D, gz = row / P.D;
            for (int dz = -1; dz < 2; ++dz) {
                const int sz = gz + dz;
                if (sz < 0 || sz >= P.D) continue;
                for (int dy = -1; dy < 2; ++dy) {
                    const int sy = gy + dy;
                    if (sy < 0 || sy >= P.D) continue;
                    int ws, we, s0, s1; // this lane's window (empty for a lane of another group), the wave's stretch
                    lane_window(P, A.S, sy, sz, cx, act, ws, we);
                    wave_hull(ws, we, A.S.n, s0, s1);
                    for (int base = s0; base < s1; base += kTracerChunk) {
                        const int cnt = min(kTracerChunk, s1 - base);
                        __syncthreads(); // the previous chunk has been read
                        // 32 bytes per candidate: (x, y, z, ., vx, vy, vz, .); with the interleaved records
                        // (vel = pos + 1, stride 2) a plain copy
                        for (int t = lane; t < 2 * cnt; t += 64)
                            cand[t] = ((t & 1) ? A.S.vel : A.S.pos)[(size_t)(base + (t >> 1)) * A.S.stride];
                        __syncthreads();
                        take_staged<2>(cand, cnt, ws - base, we - base, [&](const float4(&c)[2], bool mine) WALK_LAMBDA {
                            tracer_add(P, p.x, p.y, p.z, c[0], c[1], mine, den, nx, ny, nz);
                        });
                    }
                }
            }
        }
    }
    if (valid) tracer_finish(A, idx, p, den, nx, ny, nz);
}

} // namespace

void sph_launch_tracers(const DevParams &P, TracerArgs A, bool plain, const SortWorkspace &ws, int keyBits, hipStream_t s) {
    if (A.m <= 0) return;
    if (plain || A.S.n <= 0) { // (no particle: every sum is empty, no grid to read)
        k_tracer_plain<<<(A.m + 255) / 256, 256, 0, s>>>(P, A);
        return;
    }
    A.keys = ws.keys[0];
    A.vals = ws.vals[0];
    k_tracer_keys<<<(A.m + 255) / 256, 256, 0, s>>>(P, A);
    A.order = ws.vals[sph_sort_pairs(ws, A.m, keyBits, s)];
    k_tracer_walk<<<(A.m + 63) / 64, 64, 0, s>>>(P, A);
}
