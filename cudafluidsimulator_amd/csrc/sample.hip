// The field sample: SPH-interpolated density, speed or pressure on a regular lattice,
// gathered from the cell-sorted stream through the cell table of a grid build.  Every operation below is fp32
// and rounded on its own (-ffp-contract=off), in the order that section gives, whatever the handle's math mode.
//
// A lattice point walks the 27 cells around its own like a particle of the density sweep does.  Unlike the
// particles of a wave of that sweep, the lattice points of one wave -- 64 consecutive ix of one lattice row
// (iy, iz) -- share their candidates by construction: cy and cz are the same for all of them, and for each of the
// nine (y, z) rows of cells the three cells cx - 1 .. cx + 1 of every lane are one contiguous run of the sorted
// stream (flattened keys: x is the fastest axis).  The wave stages the hull of its lanes' runs in LDS, chunk by
// chunk, and every lane reads every staged candidate by broadcast; a lane TAKES candidate k only if k lies in
// its own run, two integer compares.  The distance test alone would not do: a candidate two cells off can round
// to within h and add a non-zero term, and the sum would no longer be the plain walk's, bit for bit.
#include "walk_common.h"

namespace {

constexpr int kSampleChunk = 512; // candidates per LDS chunk: 8 KB (a multiple of 4: the walk reads rounds of four)

// section 10a's scalar of a row, from the (vx, vy, vz, rho) sph_download_state reads
__device__ __forceinline__ float sample_scalar(const float4 v, int field) {
    if (field == SPH_FIELD_SPEED) return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    return fmaxf(0.f, SPH_GAS_CONSTANT * (v.w - SPH_REST_DENSITY));
}

// one candidate: c = (x, y, z, a_j)
template <bool kShepard>
__device__ __forceinline__ void sample_add(const DevParams &P, float px, float py, float pz, const float4 c, float &den,
                                           float &num) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const Poly6 K = poly6_mass(P, (dx * dx + dy * dy) + dz * dz);
    if (!K.taken) return;
    if (kShepard) num += K.m * c.w;
    den += K.m;
}

// the same with selected terms (walk_common.h): a candidate that is not taken, or lies beyond h, adds +0
template <bool kShepard>
__device__ __forceinline__ void sample_add(const DevParams &P, float px, float py, float pz, const float4 c, bool take,
                                           float &den, float &num) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const Poly6 K = poly6_mass(P, (dx * dx + dy * dy) + dz * dz);
    take = take && K.taken;
    if (kShepard) num += take ? K.m * c.w : 0.f;
    den += take ? K.m : 0.f;
}

template <bool kShepard>
__device__ __forceinline__ float sample_value(float den, float num) {
    if (!kShepard) return den;
    return den > 0.f ? num / den : 0.f;
}

template <bool kShepard>
__device__ __forceinline__ float4 sample_candidate(const SampleArgs &A, int j) {
    float4 c = A.S.position(j);
    if (kShepard) c.w = sample_scalar(A.S.velocity(j), A.field);
    return c;
}

// the check path (SPH_SAMPLE_PLAIN=1): one thread per lattice point, 27 cells of direct global loads
template <bool kShepard>
__global__ __launch_bounds__(256) void k_sample_plain(DevParams P, SampleArgs A, float *__restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= A.nx * A.ny * A.nz) return;
    const int ix = g % A.nx, r = g / A.nx, iy = r % A.ny, iz = r / A.ny;
    const float px = A.ox + (float)ix * A.sx, py = A.oy + (float)iy * A.sy, pz = A.oz + (float)iz * A.sz;
    const int cx = point_cell(P, px), cy = point_cell(P, py), cz = point_cell(P, pz);
    float den = 0.f, num = 0.f;
    if (cx >= 0 && cy >= 0 && cz >= 0)
        for_each_candidate_27(P, A.S, cx, cy, cz, [&](int j) WALK_LAMBDA { sample_add<kShepard>(P, px, py, pz, sample_candidate<kShepard>(A, j), den, num); });
    out[g] = sample_value<kShepard>(den, num);
}

// One wave per brick: 64 consecutive ix of the lattice row (iy, iz).  blockIdx.x = (iz ny + iy) bricks + brick.
template <bool kShepard>
__global__ __launch_bounds__(64) void k_sample_tile(DevParams P, SampleArgs A, int bricks, float *__restrict__ out) {
    __shared__ float4 cand[kSampleChunk];
    const int lane = threadIdx.x;
    const int brick = blockIdx.x % bricks, row = blockIdx.x / bricks;
    const int iy = row % A.ny, iz = row / A.ny;
    const int ix = brick * 64 + lane;
    const bool valid = ix < A.nx;
    const float px = A.ox + (float)ix * A.sx, py = A.oy + (float)iy * A.sy, pz = A.oz + (float)iz * A.sz;
    const int cx = valid ? point_cell(P, px) : -1;
    // (the same for every lane: the branches and barriers below are wave-uniform)
    const int cy = __builtin_amdgcn_readfirstlane(point_cell(P, py)), cz = __builtin_amdgcn_readfirstlane(point_cell(P, pz));
    float den = 0.f, num = 0.f;
    if (cy >= 0 && cz >= 0) {
        for (int dz = -1; dz < 2; ++dz) {
            const int sz = cz + dz;
            if (sz < 0 || sz >= P.D) continue;
            for (int dy = -1; dy < 2; ++dy) {
                const int sy = cy + dy;
                if (sy < 0 || sy >= P.D) continue;
                int ws, we, s0, s1; // this lane's window (empty for a lane without a point), the wave's stretch
                lane_window(P, A.S, sy, sz, cx, cx >= 0, ws, we);
                wave_hull(ws, we, A.S.n, s0, s1);
                for (int base = s0; base < s1; base += kSampleChunk) {
                    const int cnt = min(kSampleChunk, s1 - base);
                    __syncthreads(); // the previous chunk has been read
                    // 16 bytes per candidate: the scalar folded into .w
                    for (int k = lane; k < cnt; k += 64) cand[k] = sample_candidate<kShepard>(A, base + k);
                    __syncthreads();
                    take_staged<1>(cand, cnt, ws - base, we - base,
                                   [&](const float4(&c)[1], bool mine) WALK_LAMBDA { sample_add<kShepard>(P, px, py, pz, c[0], mine, den, num); });
                }
            }
        }
    }
    if (valid) out[(size_t)row * A.nx + ix] = sample_value<kShepard>(den, num);
}

} // namespace

void sph_launch_sample(const DevParams &P, const SampleArgs &A, bool plain, float *out, hipStream_t s) {
    const int points = A.nx * A.ny * A.nz;
    if (A.S.n <= 0) { // no particle: every sum is empty
        (void)hipMemsetAsync(out, 0, (size_t)points * sizeof(float), s);
        return;
    }
    const bool shepard = A.field != SPH_FIELD_DENSITY;
    if (plain) {
        const int blocks = (points + 255) / 256;
        if (shepard) k_sample_plain<true><<<blocks, 256, 0, s>>>(P, A, out);
        else k_sample_plain<false><<<blocks, 256, 0, s>>>(P, A, out);
        return;
    }
    const int bricks = (A.nx + 63) / 64;
    const int blocks = bricks * A.ny * A.nz; // <= 2^24 rows x 1 brick, or 64 bricks x 2^18 rows
    if (shepard) k_sample_tile<true><<<blocks, 64, 0, s>>>(P, A, bricks, out);
    else k_sample_tile<false><<<blocks, 64, 0, s>>>(P, A, bricks, out);
}
