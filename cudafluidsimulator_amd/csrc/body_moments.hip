// Per-body moments: the diagnostics' sums (section 10c) per body of the labelling (section
// 10g).  Eighteen sums of signed 64-bit Q32.32 terms per body, each accumulated as two integer sums (the low words and
// the arithmetic high words of the terms, section 10c's split) that the finish launch joins into one 128-bit value.
// No floating-point value is ever added to another across rows: the words depend on the set of rows of each body only.
//
// Default path: two launches, nine sums each (all eighteen in one launch spill SGPRs; section 10k).  A block takes
// kBodyFold x 256 consecutive rows of the sorted stream.  Each wave splits its 64 rows into groups of equal body
// (next_group); a group of several lanes reduces its 19 words -- nine low, nine high, the saturation count -- with
// shuffles, lane w keeps word w, and the first 19 lanes send them with one atomic instruction; a group of one lane
// sends its own words after the loop, all such lanes of the wave together.  Words of the body of the block's first row
// go to an LDS row (ds 64-bit adds) and leave the block as one set of global atomics; words of any other body go to
// global memory directly; zero words are skipped.  Nothing waits for anything across workgroups, and the one loop is
// bounded: `rest` loses at least a bit per trip.
//
// Check path (SPH_BODIES_PLAIN=1): one thread per row, every word straight to a global atomic.
#include "body_common.h"
#include "row_terms.h"

namespace {

constexpr int kHalfSums = SPH_BODY_SUMS / 2;       // a default-path launch reduces nine of the eighteen sums ...
constexpr int kHalfWords = 2 * kHalfSums + 1;       // ... as 19 words: nine low, nine high, its terms' saturation count
static_assert(kHalfSums == SPH_DIAG_SUMS, "the first half is the diagnostics' nine");

// nine terms of the row (p, v): HALF 0 the diagnostics' nine, HALF 1 the second moments and the angular terms
template <int HALF>
__device__ __forceinline__ void body_row_terms(const float4 p, const float4 v, long long *q, uint32_t &sat) {
    if constexpr (HALF == 0) {
        diag_sum_terms(p, v, field_bits(v, SPH_FIELD_PRESSURE), q, sat);
    } else {
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        const double vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
        // (every product is exact in fp64 -- 24 x 24 significant bits --, so a fused multiply-add would round the same
        // difference: only the subtraction rounds)
        q[SPH_BODY_SUM_XX - kHalfSums] = diag_q(x * x, sat);
        q[SPH_BODY_SUM_YY - kHalfSums] = diag_q(y * y, sat);
        q[SPH_BODY_SUM_ZZ - kHalfSums] = diag_q(z * z, sat);
        q[SPH_BODY_SUM_XY - kHalfSums] = diag_q(x * y, sat);
        q[SPH_BODY_SUM_XZ - kHalfSums] = diag_q(x * z, sat);
        q[SPH_BODY_SUM_YZ - kHalfSums] = diag_q(y * z, sat);
        q[SPH_BODY_SUM_LX - kHalfSums] = diag_q(y * vz - z * vy, sat);
        q[SPH_BODY_SUM_LY - kHalfSums] = diag_q(z * vx - x * vz, sat);
        q[SPH_BODY_SUM_LZ - kHalfSums] = diag_q(x * vy - y * vx, sat);
    }
}

// where word w of a half (low words, high words, the count) lives in a body's accumulators
template <int HALF>
__device__ __forceinline__ int half_word(int w) {
    return w < kHalfSums ? HALF * kHalfSums + w : w < 2 * kHalfSums ? SPH_BODY_SUMS + HALF * kHalfSums + (w - kHalfSums) : 2 * SPH_BODY_SUMS;
}

// the table row of row i's body, as k_body_table_fill finds it; false: the row belongs to no table row (never for a
// state whose ids are a permutation of [0, n))
__device__ __forceinline__ bool body_of_row(const BodyMomentArgs &A, int i, uint32_t id, uint32_t &b) {
    const uint32_t n = (uint32_t)A.S.n;
    const uint32_t lab = A.rowLabel[i];
    b = 0u;
    if (id >= n || lab >= n) return false;
    b = A.rank[lab];
    return b < (uint32_t)A.numBodies;
}

__device__ __forceinline__ unsigned long long term_lo(long long q) { return (unsigned long long)q & 0xFFFFFFFFull; }
__device__ __forceinline__ unsigned long long term_hi(long long q) { return (unsigned long long)(q >> 32); } // (two's complement: the wrap-around sum is the signed one)

// one row's nine terms onto dst, zero words skipped: the body's accumulators in global memory (at = half_word<HALF>) or
// the block's fold in LDS (at = the identity)
template <class At>
__device__ __forceinline__ void emit_row(unsigned long long *dst, At at, const long long *q, uint32_t sat) {
#pragma unroll
    for (int t = 0; t < kHalfSums; ++t) {
        if (term_lo(q[t])) atomicAdd(&dst[at(t)], term_lo(q[t]));
        if (term_hi(q[t])) atomicAdd(&dst[at(kHalfSums + t)], term_hi(q[t]));
    }
    if (sat) atomicAdd(&dst[at(2 * kHalfSums)], (unsigned long long)sat);
}

// the check path
__global__ __launch_bounds__(256) void k_body_moments_plain(BodyMomentArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.S.n) return;
    const float4 p = A.S.position(i);
    uint32_t b;
    if (!body_of_row(A, i, __float_as_uint(p.w), b)) return;
    long long q[SPH_BODY_SUMS];
    uint32_t sat = 0u;
    const float4 v = A.S.velocity(i);
    body_row_terms<0>(p, v, q, sat);
    body_row_terms<1>(p, v, q + kHalfSums, sat);
    unsigned long long *dst = A.rows + (size_t)kBodyMomentStride * b;
    for (int t = 0; t < SPH_BODY_SUMS; ++t) {
        atomicAdd(&dst[t], term_lo(q[t]));
        atomicAdd(&dst[SPH_BODY_SUMS + t], term_hi(q[t]));
    }
    if (sat) atomicAdd(&dst[2 * SPH_BODY_SUMS], (unsigned long long)sat);
}

// the default path, one launch per half of the sums (all eighteen in one launch: the compiler spills SGPRs)
template <int HALF>
__global__ __launch_bounds__(256) void k_body_moments(BodyMomentArgs A) {
    __shared__ unsigned long long fold[kHalfWords]; // the words of the body of the block's first row
    __shared__ uint32_t foldBody;
    const int base = blockIdx.x * (256 * kBodyFold);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < kHalfWords) fold[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) {
        uint32_t b;
        const bool ok = body_of_row(A, base, __float_as_uint(A.S.position(base).w), b); // (base < n: the grid is fold_blocks_of(n))
        foldBody = ok ? b : kNoId; // (kNoId: no row of the block matches, nothing is folded)
    }
    __syncthreads();
    const uint32_t dom = foldBody;
    const int word = half_word<HALF>(lane < kHalfWords ? lane : 0); // the accumulator this lane sends for a group
#pragma unroll 1
    for (int k = 0; k < kBodyFold; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        bool valid = i < A.S.n;
        const float4 p = A.S.position(valid ? i : 0);
        const float4 v = A.S.velocity(valid ? i : 0);
        uint32_t b;
        valid = body_of_row(A, valid ? i : 0, __float_as_uint(p.w), b) && valid;
        long long q[kHalfSums];
        uint32_t sat = 0u;
        body_row_terms<HALF>(p, v, q, sat);
        bool alone = false; // the only row of its body in this wave
        unsigned long long rest = __ballot(valid);
        while (rest) {
            uint32_t b0;
            int lead;
            const unsigned long long grp = next_group(b, valid, rest, b0, lead);
            if (__popcll(grp) == 1) { // no shuffles: the lane sends its own words below
                alone = alone || lane == lead;
                continue;
            }
            const bool in = (grp >> lane) & 1;
            unsigned long long mine = 0ull; // lane w: word w of the group
#pragma unroll
            for (int t = 0; t < kHalfSums; ++t) {
                const unsigned long long lo = wave_sum_u64(in ? term_lo(q[t]) : 0ull);
                const unsigned long long hi = wave_sum_u64(in ? term_hi(q[t]) : 0ull);
                mine = lane == t ? lo : lane == kHalfSums + t ? hi : mine;
            }
            const uint32_t s = wave_sum_u32(in ? sat : 0u); // (nine terms a row, 64 rows)
            mine = lane == 2 * kHalfSums ? (unsigned long long)s : mine;
            if (lane < kHalfWords && mine) {
                if (b0 == dom) atomicAdd(&fold[lane], mine);
                else atomicAdd(&A.rows[(size_t)kBodyMomentStride * b0 + word], mine);
            }
        }
        if (alone) {
            if (b == dom) emit_row(fold, [](int w) { return w; }, q, sat);
            else emit_row(A.rows + (size_t)kBodyMomentStride * b, [](int w) { return half_word<HALF>(w); }, q, sat);
        }
    }
    __syncthreads();
    if (threadIdx.x < kHalfWords && dom != kNoId && fold[threadIdx.x])
        atomicAdd(&A.rows[(size_t)kBodyMomentStride * dom + word], fold[threadIdx.x]);
}

// One thread per body: the accumulators joined into the raw row, in place, and the body counted in its size bin (a
// block's bins meet in LDS first).  L = the sum of the low words (below 2^63: fewer than 2^31 rows of words below
// 2^32), H = the signed sum of the high words (below 2^62 in magnitude); the sum is L + H 2^32 in 128 bits.
__global__ __launch_bounds__(256) void k_body_moments_finish(BodyMomentArgs A) {
    __shared__ uint32_t bins[SPH_BODY_SIZE_BINS];
    if (threadIdx.x < SPH_BODY_SIZE_BINS) bins[threadIdx.x] = 0u;
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < A.numBodies) {
        unsigned long long *r = A.rows + (size_t)kBodyMomentStride * b;
        unsigned long long w[kBodyMomentWords];
#pragma unroll
        for (int k = 0; k < kBodyMomentWords; ++k) w[k] = r[k];
        const uint32_t label = A.table[8 * (size_t)b], count = A.table[8 * (size_t)b + 1];
        r[0] = (unsigned long long)label | ((unsigned long long)count << 32);
        r[1] = w[2 * SPH_BODY_SUMS];
#pragma unroll
        for (int t = 0; t < SPH_BODY_SUMS; ++t) {
            const unsigned long long L = w[t];
            const long long H = (long long)w[SPH_BODY_SUMS + t];
            const unsigned long long lo = L + ((unsigned long long)H << 32);
            r[2 + 2 * t] = lo;
            r[3 + 2 * t] = (unsigned long long)((H >> 32) + (lo < L ? 1ll : 0ll));
        }
        if (count) atomicAdd(&bins[31 - __clz((int)count)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < SPH_BODY_SIZE_BINS && bins[threadIdx.x]) atomicAdd(&A.sizeHist[threadIdx.x], bins[threadIdx.x]);
}

static_assert(sizeof(SphBodyMomentsRaw) == kBodyMomentStride * sizeof(unsigned long long), "a raw row is the device row");
static_assert(kBodyMomentWords <= kBodyMomentStride, "the accumulators fit the row");

} // namespace

void sph_launch_body_moments(const BodyMomentArgs &A, bool plain, hipStream_t s) {
    (void)hipMemsetAsync(A.sizeHist, 0, SPH_BODY_SIZE_BINS * sizeof(uint32_t), s);
    if (A.S.n <= 0 || A.numBodies <= 0) return;
    (void)hipMemsetAsync(A.rows, 0, (size_t)A.numBodies * kBodyMomentStride * sizeof(unsigned long long), s);
    if (plain) k_body_moments_plain<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A);
    else {
        k_body_moments<0><<<fold_blocks_of(A.S.n), 256, 0, s>>>(A);
        k_body_moments<1><<<fold_blocks_of(A.S.n), 256, 0, s>>>(A);
    }
    k_body_moments_finish<<<blocks_of(A.numBodies, 256), 256, 0, s>>>(A);
}
