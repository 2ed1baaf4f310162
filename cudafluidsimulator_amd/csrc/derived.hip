// Derived per-particle fields: vorticity, divergence, density gradient, the density sum and
// the neighbour count of every particle of the current state, from one more neighbour sweep over the grid's sorted
// stream.  Every operation below is fp32 and rounded on its own (-ffp-contract=off), in the order that section
// gives, whatever the handle's math mode.
//
// Row i walks what the density sweep walks: the nine runs of load_runs (sweep_common.h) around sweep_cell of its own
// position, each in stream order.  The default path gives one wave 64 consecutive rows -- they are in cell order
// already, so their runs overlap -- and for each of the nine runs stages the UNION of its lanes' ranges in LDS as
// 32-byte records (x, y, z, id, vx, vy, vz, .); every lane then walks its own range [js[r], je[r]) from the staged
// slice, four candidates per trip, with unconditional reads (an exhausted lane reads the slice's last record again)
// and selected terms, which change no bit (walk_common.h).  A run whose union is longer than the slice (a wave that spans two rows of cells, a crowded
// cell) is walked by every lane from global memory, in the same order with the same arithmetic, so both walks give
// the same words.  The walk itself is walk_common.h's walk_runs_staged, shared with neighbours.hip: one workgroup is one
// wave; its barriers are wave-uniform (u0, u1 and the trip count are made uniform through readfirstlane); nothing spins
// and no workgroup talks to another.
#include "walk_common.h"

namespace {

// (A/B builds for scripts/studies/derived.py: -DDERIVE_SLICE=...; the default is the measured choice of DESIGN.md
// section 10f)
#ifndef DERIVE_SLICE
#define DERIVE_SLICE 320 // staged candidates per run: 10 KB of 32-byte records, the most that leaves 16 one-wave
                         // workgroups per CU (160 KB of LDS), which is what the kernel's registers allow anyway.
                         // Measured at n = 4,194,304 (ms per sweep after step 20 / after step 100; check path 1.91 /
                         // 6.5): 128: 1.39 / 7.37, 256: 1.39 / 6.11, 320: 1.38 / 5.72, 384: 1.57 / 5.60,
                         // 512: 1.79 / 5.90 -- late in a run a quarter of the runs at 256 are longer than the slice
                         // and walk from global memory; beyond 320 the lost resident waves cost the early state more
#endif
constexpr int kDeriveSlice = DERIVE_SLICE;
constexpr int kDeriveTrip = 4;             // candidates per trip of the staged walk (2 and 8 measured within 3 % of it)

struct DeriveAcc {
    float rho = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, s = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
    uint32_t count = 0;
};

// the terms of one candidate, c = (x, y, z, .), v = (vx, vy, vz, .): the definition written down
struct DeriveTerms {
    float m, gx, gy, gz, s, cx, cy, cz;
    bool taken;
};
__device__ __forceinline__ DeriveTerms derive_terms(const DevParams &P, const float4 pi, const float4 vi, const float4 c, const float4 v) {
    DeriveTerms T;
    const float ex = c.x - pi.x, ey = c.y - pi.y, ez = c.z - pi.z;
    const Poly6 K = poly6_mass(P, (ex * ex + ey * ey) + ez * ez);
    T.taken = K.taken;
    T.m = K.m;
    const float w = SPH_MASS * K.a;
    const float ux = v.x - vi.x, uy = v.y - vi.y, uz = v.z - vi.z;
    T.gx = w * ex;
    T.gy = w * ey;
    T.gz = w * ez;
    T.s = w * ((ux * ex + uy * ey) + uz * ez);
    T.cx = w * (ey * uz - ez * uy);
    T.cy = w * (ez * ux - ex * uz);
    T.cz = w * (ex * uy - ey * ux);
    return T;
}

// a candidate of the direct walk: not taken, nothing is added
__device__ __forceinline__ void derive_add(const DevParams &P, const float4 pi, const float4 vi, const float4 c, const float4 v, DeriveAcc &S) {
    const DeriveTerms T = derive_terms(P, pi, vi, c, v);
    if (!T.taken) return;
    S.rho += T.m;
    S.gx += T.gx;
    S.gy += T.gy;
    S.gz += T.gz;
    S.s += T.s;
    S.cx += T.cx;
    S.cy += T.cy;
    S.cz += T.cz;
    S.count += 1;
}

// the same without a branch: a candidate outside the lane's range, or beyond h, adds +0 to every sum
__device__ __forceinline__ void derive_add(const DevParams &P, const float4 pi, const float4 vi, const float4 c, const float4 v, bool mine,
                                           DeriveAcc &S) {
    const DeriveTerms T = derive_terms(P, pi, vi, c, v);
    const bool take = mine && T.taken;
    S.rho += take ? T.m : 0.f;
    S.gx += take ? T.gx : 0.f;
    S.gy += take ? T.gy : 0.f;
    S.gz += take ? T.gz : 0.f;
    S.s += take ? T.s : 0.f;
    S.cx += take ? T.cx : 0.f;
    S.cy += take ? T.cy : 0.f;
    S.cz += take ? T.cz : 0.f;
    S.count += take ? 1u : 0u;
}

// results and the three stores of the row whose position words are pi: to the slot of its particle id
__device__ __forceinline__ void derive_finish(const DeriveArgs &A, const float4 pi, const DeriveAcc &S) {
    const uint32_t id = __float_as_uint(pi.w);
    if (id >= (uint32_t)A.S.n) return; // (the ids of a state are a permutation of [0, n): never taken)
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (S.rho > 0.f) {
        w.x = (6.f * S.cx) / S.rho;
        w.y = (6.f * S.cy) / S.rho;
        w.z = (6.f * S.cz) / S.rho;
        w.w = (6.f * S.s) / S.rho;
    }
    A.vortDiv[id] = w;
    A.gradRho[id] = make_float4(6.f * S.gx, 6.f * S.gy, 6.f * S.gz, S.rho);
    A.neighbours[id] = S.count;
}

// the check path (SPH_DERIVE_PLAIN=1): one thread per row of the sorted stream, every candidate from global memory
__global__ __launch_bounds__(256) void k_derive_plain(DevParams P, DeriveArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < A.S.n;
    const float4 pi = A.S.position(valid ? i : 0), vi = A.S.velocity(valid ? i : 0);
    int js[9], je[9];
    clipped_runs(P, A.S, pi, valid, js, je);
    DeriveAcc S;
    for_each_row_candidate(js, je, [&](int j) WALK_LAMBDA { derive_add(P, pi, vi, A.S.position(j), A.S.velocity(j), S); });
    if (valid) derive_finish(A, pi, S);
}

// One wave per 64 consecutive rows of the sorted stream.
__global__ __launch_bounds__(64) void k_derive_wave(DevParams P, DeriveArgs A) {
    __shared__ float4 slice[2 * kDeriveSlice];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    const bool valid = i < A.S.n;
    const float4 pi = A.S.position(valid ? i : 0), vi = A.S.velocity(valid ? i : 0);
    int js[9], je[9];
    clipped_runs(P, A.S, pi, valid, js, je);
    DeriveAcc S;
    uint32_t staged = 0, direct = 0;
    walk_runs_staged<2, kDeriveSlice, kDeriveTrip>(
        A.S, js, je, slice, staged, direct, [&](int j) WALK_LAMBDA { derive_add(P, pi, vi, A.S.position(j), A.S.velocity(j), S); },
        [&](const float4(&c)[2], bool mine) WALK_LAMBDA { derive_add(P, pi, vi, c[0], c[1], mine, S); });
    if (lane == 0) {
        if (staged) atomicAdd(&A.counters[0], (unsigned long long)staged);
        if (direct) atomicAdd(&A.counters[1], (unsigned long long)direct);
    }
    if (valid) derive_finish(A, pi, S);
}

} // namespace

void sph_launch_derive(const DevParams &P, const DeriveArgs &A, bool plain, hipStream_t s) {
    const int n = A.S.n;
    if (n <= 0) return;
    if (plain) k_derive_plain<<<(n + 255) / 256, 256, 0, s>>>(P, A);
    else k_derive_wave<<<(n + 63) / 64, 64, 0, s>>>(P, A);
}
