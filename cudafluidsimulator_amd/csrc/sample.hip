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
#include "sph_c_api.h"
#include "sph_device.h"

namespace {

constexpr int kSampleChunk = 512; // candidates per LDS chunk: 8 KB (a multiple of 4: the walk reads rounds of four)

// section 10a's scalar of a row, from the (vx, vy, vz, rho) sph_download_state reads
__device__ __forceinline__ float sample_scalar(const float4 v, int field) {
    if (field == SPH_FIELD_SPEED) return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    return fmaxf(0.f, SPH_GAS_CONSTANT * (v.w - SPH_REST_DENSITY));
}

// the cell of a coordinate, (int)(p / h) like the cell hash, or -1 for a point outside the grid
// (the range tests come before the conversion: a float beyond the int range must not reach it)
__device__ __forceinline__ int sample_cell(const DevParams &P, float p) {
    if (!(p >= 0.f)) return -1;
    const float q = p / P.h;
    if (!(q < (float)P.D)) return -1; // (int)q >= D
    return (int)q;
}

// one candidate: c = (x, y, z, a_j)
template <bool kShepard>
__device__ __forceinline__ void sample_add(const DevParams &P, float px, float py, float pz, const float4 c, float &den,
                                           float &num) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 > P.h2) return;
    const float diff = P.h2 - d2;
    const float m = SPH_MASS * (((P.dcoef * diff) * diff) * diff);
    if (kShepard) num += m * c.w;
    den += m;
}

// the same without a branch: a candidate that is not taken, or lies beyond h, adds +0 (den and num never fall
// below +0: m >= +0 and a_j >= +0, so the sums keep their bits)
template <bool kShepard>
__device__ __forceinline__ void sample_add(const DevParams &P, float px, float py, float pz, const float4 c, bool take,
                                           float &den, float &num) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    take = take && !(d2 > P.h2);
    const float diff = P.h2 - d2;
    const float m = SPH_MASS * (((P.dcoef * diff) * diff) * diff);
    if (kShepard) num += take ? m * c.w : 0.f;
    den += take ? m : 0.f;
}

template <bool kShepard>
__device__ __forceinline__ float sample_value(float den, float num) {
    if (!kShepard) return den;
    return den > 0.f ? num / den : 0.f;
}

template <bool kShepard>
__device__ __forceinline__ float4 sample_candidate(const SampleArgs &A, int j) {
    float4 c = A.pos[(size_t)j * A.stride];
    if (kShepard) c.w = sample_scalar(A.vel[(size_t)j * A.stride], A.field);
    return c;
}

// the check path (SPH_SAMPLE_PLAIN=1): one thread per lattice point, nine runs of direct global loads
template <bool kShepard>
__global__ __launch_bounds__(256) void k_sample_plain(DevParams P, SampleArgs A, float *__restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= A.nx * A.ny * A.nz) return;
    const int ix = g % A.nx, r = g / A.nx, iy = r % A.ny, iz = r / A.ny;
    const float px = A.ox + (float)ix * A.sx, py = A.oy + (float)iy * A.sy, pz = A.oz + (float)iz * A.sz;
    const int cx = sample_cell(P, px), cy = sample_cell(P, py), cz = sample_cell(P, pz);
    float den = 0.f, num = 0.f;
    if (cx >= 0 && cy >= 0 && cz >= 0) {
        for (int dz = -1; dz < 2; ++dz) {
            const int sz = cz + dz;
            if (sz < 0 || sz >= P.D) continue;
            for (int dy = -1; dy < 2; ++dy) {
                const int sy = cy + dy;
                if (sy < 0 || sy >= P.D) continue;
                for (int dx = -1; dx < 2; ++dx) {
                    const int sx = cx + dx;
                    if (sx < 0 || sx >= P.D) continue;
                    const int2 run = A.cellRange[(sz * P.D + sy) * P.D + sx];
                    for (int j = max(run.x, 0); j < min(run.y, A.n); ++j)
                        sample_add<kShepard>(P, px, py, pz, sample_candidate<kShepard>(A, j), den, num);
                }
            }
        }
    }
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
    const int cx = valid ? sample_cell(P, px) : -1;
    // (the same for every lane: the branches and barriers below are wave-uniform)
    const int cy = __builtin_amdgcn_readfirstlane(sample_cell(P, py)), cz = __builtin_amdgcn_readfirstlane(sample_cell(P, pz));
    float den = 0.f, num = 0.f;
    if (cy >= 0 && cz >= 0) {
        for (int dz = -1; dz < 2; ++dz) {
            const int sz = cz + dz;
            if (sz < 0 || sz >= P.D) continue;
            for (int dy = -1; dy < 2; ++dy) {
                const int sy = cy + dy;
                if (sy < 0 || sy >= P.D) continue;
                // this lane's window of the stream: the rows of cells cx - 1 .. cx + 1 of this (y, z) row, one
                // contiguous run (empty cells hold {0, 0} and add nothing); empty for a lane without a point
                int ws = 0x7fffffff, we = 0;
                if (cx >= 0) {
                    const int2 *cells = A.cellRange + (sz * P.D + sy) * P.D;
                    for (int sx = max(cx - 1, 0); sx <= min(cx + 1, P.D - 1); ++sx) {
                        const int2 run = cells[sx];
                        if (run.y > run.x) {
                            ws = min(ws, run.x);
                            we = max(we, run.y);
                        }
                    }
                }
                // the stretch the wave stages: from the first window's start to the last one's end
                const int s0 = max(__builtin_amdgcn_readfirstlane(wave_min_i32(ws)), 0);
                const int s1 = min(__builtin_amdgcn_readfirstlane(wave_max_i32(we)), A.n);
                for (int base = s0; base < s1; base += kSampleChunk) {
                    const int cnt = min(kSampleChunk, s1 - base);
                    __syncthreads(); // the previous chunk has been read
                    for (int k = lane; k < cnt; k += 64) cand[k] = sample_candidate<kShepard>(A, base + k);
                    __syncthreads();
                    // every lane reads every candidate (one LDS address per read: a broadcast) and takes those of
                    // its own window, in stream order.  Reads and arithmetic are unconditional and a candidate
                    // that is not taken adds +0, which changes no bit of a sum that is never below +0: the four
                    // reads of a round are in flight together instead of one wait per candidate.  (Slots past
                    // cnt hold stale rows: they lie outside every [lo, hi).)
                    const int lo = max(ws - base, 0), hi = min(we - base, cnt);
                    for (int k = 0; k < cnt; k += 4) {
                        float4 c[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) c[u] = cand[k + u];
#pragma unroll
                        for (int u = 0; u < 4; ++u) sample_add<kShepard>(P, px, py, pz, c[u], k + u >= lo && k + u < hi, den, num);
                    }
                }
            }
        }
    }
    if (valid) out[(size_t)row * A.nx + ix] = sample_value<kShepard>(den, num);
}

} // namespace

void sph_launch_sample(const DevParams &P, const SampleArgs &A, bool plain, float *out, hipStream_t s) {
    const int points = A.nx * A.ny * A.nz;
    if (A.n <= 0) { // no particle: every sum is empty
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
