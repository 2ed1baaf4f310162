// Pair statistics: per bin of separation the number of pairs within a radius and four exact
// sums over them -- d2, |dv|^2, e.dv and (e.dv)^2 / d2 -- as Q32.32 terms (row_terms.h's diag_q, as it is).  A pair is
// an unordered pair of distinct particle ids the neighbour lists' link test takes (walk_common.h's linked); the row
// whose id is the smaller takes it.  The test and the differences are fp32 with every operation rounded on its own
// (-ffp-contract=off), the terms fp64 likewise, whatever the handle's math mode; everything after them is integers, so
// the words depend on the set of pairs alone.
//
// Default path, clear -> walk -> join.  The walk is derived.hip's: one wave per tile of 64 consecutive rows of the
// sorted stream, walk_runs_staged with 32-byte records.  What is new is where a candidate's result goes: not into the
// lane's registers but into a table of bins x 10 words in the workgroup's LDS, lanes of one trip hitting different
// bins.  A lane holds a taken candidate back until the wave sends what its lanes hold (PairPending), so that the fp64
// terms, the search of the table and the atomics run for many lanes at a time.  The adds are integer LDS atomics under
// the lane's mask -- the rule at the top of walk_common.h, select and never branch, is about FLOAT sums, where an
// unselected garbage term would be added; an integer add that does not happen changes no word, and the reads the walk
// shares stay unconditional.  No atomic on the table ever reaches global memory: a fixed number of workgroups is
// launched, each takes tiles from one atomic counter (nothing waits on it; the tile loop is bounded by the tile count),
// keeps its LDS table across its tiles and stores it once, plainly, to its own row of `partials`.  k_pair_join folds
// the rows and joins the words of a sum into 128 bits.
//
// No accumulator wraps.  A sum's term q is split as body_moments.hip splits it: the low 32 bits, unsigned, go to the
// lo word, q >> 32, signed, to the hi word, both 64 bits wide.  After every tile the workgroup carries lo >> 32 into hi
// and keeps lo below 2^32; a hi word beyond +-2^62 (PairArgs.shed; SPH_PAIRS_SHED_BITS lowers it, so that tests see
// the top words at work) sheds hi >> 32 into its top word (in the workgroup's row in global memory, touched by its one
// lane only) and keeps its low 32 bits.  A tile adds at most 64 (n - 1) terms to a word:
// below 2^30 2^32 to lo and below 2^30 2^31 = 2^61 to hi for n <= kPairMaxN = 2^24, so lo stays below 2^63 and hi within
// +-(2^62 + 2^61) for ANY state, all particles coincident and every term saturated included.  The top word would need
// 2^63 / 2^29 tiles.  A larger n is refused by the host.  The value of a row's sum is lo + hi 2^32 + top 2^64.
//
// Check path (SPH_PAIRS_PLAIN=1): one thread per row, every candidate from global memory (for_each_row_candidate), the
// bin by a linear scan of the table in global memory, every word one global atomic into a single row of the same
// layout; the value an atomic returns tells whether that add wrapped its word, and the wrap is carried into the next
// word, so this path is exact for any n.  The same join.
#include "row_terms.h"
#include "walk_common.h"

namespace {

// (A/B builds for scripts/studies/pairs.py: -DPAIR_SLICE=..., -DPAIR_WGS_PER_CU=..., -DPAIR_DEFER=0, -DPAIR_BIN_MAJOR=0;
// the defaults are the measured choices of DESIGN.md section 10m.)
// Measured on an MI355X at n = 4,194,304, `-i random`, 32 bins, radius h, ms per call after step 20 / after step 100
// (70,977,649 / 401,032,247 pairs), medians of 3 to 5 rounds, spread below 1 %; k_derive_wave on the same states in the
// same rounds: 1.31 / 5.60.  Shipped: 3.31 / 13.86; the check path 259.2 / 1306.0; the neighbour lists in walk order
// until they have landed on the host, the route this pass replaces: 12.76 / 63.18.  The walk is bound by latency --
// the fp64 division, the search's dependent LDS reads, the atomics behind them -- and its time falls with the number of
// waves a CU holds, which the LDS decides: every choice below is a choice of residency first.
#ifndef PAIR_SLICE
#define PAIR_SLICE 192 // kPairSlice, tests/pair_states.py's SLICE: staged candidates per run, 6 KB of 32-byte records.
                       // With 16 workgroups per CU: 192: 3.31 / 13.90 (40 % of the late runs walk from global memory),
                       // 256: 3.59 / 14.89; with 12: 320 (derived.hip's slice): 4.21 / 17.11; with 10: 384: 4.51 / 17.93;
                       // 128: 3.30 / 13.89 and 160: 3.30 / 13.82 -- a plateau
#endif
#ifndef PAIR_WGS_PER_CU
#define PAIR_WGS_PER_CU 16 // workgroups launched per compute unit: what the kernel's registers let a CU hold (4 waves per
                           // SIMD); with the default 32 bins a workgroup holds 8.7 KB of LDS and all 16 are resident,
                           // with 128 bins 16.5 KB and 9 are.  At slice 320, sent where met: 4: 11.36 / 43.79,
                           // 8: 5.84 / 22.62, 12: 4.63 / 17.84, 16 (12 resident): 4.63 / 17.80
#endif
#ifndef PAIR_DEFER
#define PAIR_DEFER 1 // 1: a lane keeps a taken candidate back (PairPending) and the wave sends what its lanes hold when one
                     // of them takes a second; 0: every taken candidate is binned and sent where it is met.  At slice
                     // 320, 12 workgroups per CU: 4.21 / 17.11 against 4.60 / 17.84; the shipped build: 3.31 / 13.86
                     // against 3.66 / 14.79
#endif
#ifndef PAIR_BIN_MAJOR
#define PAIR_BIN_MAJOR 1 // the LDS table's layout.  1, bin-major: word w of bin b at [10 b + w], a bin's words in 80
                         // consecutive bytes; 0, word-major: [w bins + b], the lanes of one atomic instruction -- which
                         // all send the same word w -- in neighbouring 8-byte words.  Conflicts do not bound the walk:
                         // one bin for everything is the FASTEST table (3.51 / 15.01 against 4.21 / 17.11 with 32
                         // bins, same build), and lanes of equal bin reducing their words with shuffles before one
                         // set of atomics (built, measured, removed) took 22.06 / 82.23 against 5.84 / 22.62.  At
                         // slice 320, 12 workgroups per CU: 4.18 / 16.79 against 4.21 / 17.11
#endif
constexpr int kPairSlice = PAIR_SLICE;
constexpr int kPairTrip = 4; // candidates per trip of the staged walk, as derived.hip's
static_assert(sizeof(SphPairBinRaw) == 80, "a raw row is ten 64-bit words");
static_assert(kPairLo + SPH_PAIR_SUMS == kPairHi && kPairHi + SPH_PAIR_SUMS == kPairSat && kPairSat + 1 == kPairTop &&
                  kPairTop + SPH_PAIR_SUMS == kPairWords,
              "count, lo words, hi words, saturation count, top words");

__device__ __forceinline__ int lds_at(int w, int b, int B) { return PAIR_BIN_MAJOR ? b * kPairLdsWords + w : w * B + b; }

__device__ __forceinline__ unsigned long long term_lo(long long q) { return (unsigned long long)q & 0xFFFFFFFFull; }
__device__ __forceinline__ long long term_hi(long long q) { return q >> 32; }

// the four terms of a taken pair: row (pi, vi), candidate (c, v), d2 = link_d2(pi, c); the definition written down
struct PairTerms {
    long long q[SPH_PAIR_SUMS];
    uint32_t sat = 0;
};
__device__ __forceinline__ PairTerms pair_terms(const float4 pi, const float4 vi, const float4 c, const float4 v, float d2) {
    PairTerms T;
    // (the link test's own differences: the same expressions, which the compiler computes once)
    const double ex = (double)(c.x - pi.x), ey = (double)(c.y - pi.y), ez = (double)(c.z - pi.z);
    const double wx = (double)(v.x - vi.x), wy = (double)(v.y - vi.y), wz = (double)(v.z - vi.z);
    // (every product of two widened fp32 values is exact in fp64: only the additions and the division round)
    const double a = (ex * wx + ey * wy) + ez * wz;
    T.q[SPH_PAIR_SUM_D2] = diag_q((double)d2, T.sat);
    T.q[SPH_PAIR_SUM_W2] = diag_q((wx * wx + wy * wy) + wz * wz, T.sat);
    T.q[SPH_PAIR_SUM_A] = diag_q(a, T.sat);
    T.q[SPH_PAIR_SUM_L2] = diag_q(d2 == 0.f ? 0.0 : (a * a) / (double)d2, T.sat);
    return T;
}

// The bin of a taken pair: the number of k < B - 1 with edges[k] < d2.  The table does not decrease, so those k are a
// prefix and the bin is where it ends: a guess from the hardware's approximate square root (no square root decides
// anything), walked down while the edge below is not below d2 and up while the edge at k is.  Either loop takes at
// most B - 1 trips; with bins of distinct edges the guess is off by one at the most.
__device__ __forceinline__ int pair_bin(const float *edges, int B, float perRadius, float d2) {
    // (clamped as a float, before the conversion: perRadius is inf for a denormal radius, and 0 inf is a NaN -> bin 0)
    const float g = __builtin_amdgcn_sqrtf(d2) * perRadius;
    int k = !(g >= 1.f) ? 0 : g < (float)(B - 1) ? (int)g : B - 1;
    while (k > 0 && !(edges[k - 1] < d2)) --k;
    while (k < B - 1 && edges[k] < d2) ++k;
    return k;
}

// one lane's pair onto the workgroup's table; zero words are skipped (the hi word of d2 is always one: d2 < 1)
__device__ __forceinline__ void lds_emit(unsigned long long *table, int B, int bin, const PairTerms &T) {
    atomicAdd(&table[lds_at(kPairCount, bin, B)], 1ull);
#pragma unroll
    for (int s = 0; s < SPH_PAIR_SUMS; ++s) {
        if (term_lo(T.q[s])) atomicAdd(&table[lds_at(kPairLo + s, bin, B)], term_lo(T.q[s]));
        if (term_hi(T.q[s])) atomicAdd(&table[lds_at(kPairHi + s, bin, B)], (unsigned long long)term_hi(T.q[s]));
    }
    if (T.sat) atomicAdd(&table[lds_at(kPairSat, bin, B)], (unsigned long long)T.sat);
}

// A taken candidate a lane holds back.  One lane in thirteen takes a given candidate of a late state, so some lane of
// the wave takes nearly every one, and binning and sending a candidate where it is met runs the fp64 terms, the search
// and the atomics for a handful of lanes at a time.  Held back, the wave's candidates are sent together when a lane
// meets its second.  Integer adds commute: the order changes no word.
struct PairPending {
    float4 c, v;
    bool full = false;
};

// what the default path's workgroup needs of a tile's row
struct PairRow {
    float4 pi, vi;
    uint32_t id;
    int js[9], je[9];
    __device__ __forceinline__ PairRow(const DevParams &P, const PairArgs &A, int i) {
        const bool valid = i < A.S.n;
        pi = A.S.position(valid ? i : 0);
        vi = A.S.velocity(valid ? i : 0);
        id = __float_as_uint(pi.w);
        clipped_runs(P, A.S, pi, valid && id < (uint32_t)A.S.n, js, je); // (not a row of the state: nine empty runs)
    }
};

// a taken candidate (c, v) of the row R: binned and sent to the workgroup's table
__device__ __forceinline__ void pair_send(const PairArgs &A, const PairRow &R, const float4 c, const float4 v, unsigned long long *table,
                                          const float *edges) {
    const float d2 = link_d2(R.pi, c);
    lds_emit(table, A.bins, pair_bin(edges, A.bins, A.perRadius, d2), pair_terms(R.pi, R.vi, c, v, d2));
}

// One candidate (c, v) of the row R: taken when it is the lane's (mine), linked and of a greater id.
__device__ __forceinline__ void pair_take(const PairArgs &A, const PairRow &R, const float4 c, const float4 v, bool mine,
                                          unsigned long long *table, const float *edges, PairPending &Q) {
    const bool take = mine && linked(R.pi, c, A.r2) && __float_as_uint(c.w) > R.id;
    if constexpr (PAIR_DEFER) {
        // (the ballot is over the lanes that are here: all of them in a staged trip, those still walking in a direct run)
        if (__ballot(take && Q.full) && Q.full) {
            pair_send(A, R, Q.c, Q.v, table, edges);
            Q.full = false;
        }
        if (take) Q.c = c, Q.v = v, Q.full = true;
    } else {
        if (take) pair_send(A, R, c, v, table, edges);
    }
}

// The default path: blockIdx.x is a partial row, not a tile.
__global__ __launch_bounds__(64) void k_pair_wave(DevParams P, PairArgs A) {
    __shared__ float4 slice[2 * kPairSlice];
    extern __shared__ unsigned long long table[]; // kPairLdsWords x bins words, then the bins edges
    const int lane = threadIdx.x, B = A.bins;
    float *edges = reinterpret_cast<float *>(table + kPairLdsWords * B);
    unsigned long long *row = A.partials + (size_t)blockIdx.x * (kPairWords * B); // (blockIdx.x < A.rows: the grid)
    for (int t = lane; t < kPairLdsWords * B; t += 64) table[t] = 0ull;
    for (int t = lane; t < B; t += 64) edges[t] = A.edges2[t];
    for (int t = lane; t < SPH_PAIR_SUMS * B; t += 64) row[kPairTop * B + t] = 0ull;
    __syncthreads();
    const int tiles = (A.S.n + 63) / 64;
    uint32_t staged = 0, direct = 0;
#pragma unroll 1
    for (int trip = 0; trip < tiles; ++trip) { // (a workgroup takes at most every tile)
        unsigned int next = 0u;
        if (lane == 0) next = atomicAdd(A.tile, 1u);
        const unsigned int tile = __builtin_amdgcn_readfirstlane(next); // (lane 0's, the same in every lane)
        if (tile >= (unsigned int)tiles) break;
        const PairRow R(P, A, (int)tile * 64 + lane);
        PairPending Q;
        walk_runs_staged<2, kPairSlice, kPairTrip>(
            A.S, R.js, R.je, slice, staged, direct,
            [&](int j) WALK_LAMBDA { pair_take(A, R, A.S.position(j), A.S.velocity(j), true, table, edges, Q); },
            [&](const float4(&c)[2], bool mine) WALK_LAMBDA { pair_take(A, R, c[0], c[1], mine, table, edges, Q); });
        if (Q.full) pair_send(A, R, Q.c, Q.v, table, edges); // what the lanes still hold
        __syncthreads();
        // the carries (the top of this file): lane t mod 64 owns sum t / B of bin t mod B, in LDS and in the row
        for (int t = lane; t < SPH_PAIR_SUMS * B; t += 64) {
            const int s = t / B, b = t - s * B;
            const unsigned long long lo = table[lds_at(kPairLo + s, b, B)];
            long long hi = (long long)(table[lds_at(kPairHi + s, b, B)] + (lo >> 32));
            table[lds_at(kPairLo + s, b, B)] = lo & 0xFFFFFFFFull;
            if (hi >= A.shed || hi < -A.shed) {
                row[kPairTop * B + t] += (unsigned long long)(hi >> 32);
                hi &= 0xFFFFFFFFll;
            }
            table[lds_at(kPairHi + s, b, B)] = (unsigned long long)hi;
        }
        __syncthreads();
    }
    for (int t = lane; t < kPairLdsWords * B; t += 64) {
        const int w = t / B;
        row[t] = table[lds_at(w, t - w * B, B)];
    }
    if (lane == 0) {
        if (staged) atomicAdd(&A.counters[0], (unsigned long long)staged);
        if (direct) atomicAdd(&A.counters[1], (unsigned long long)direct);
    }
}

// ---- the check path ----
// hi += a, signed; the value the atomic returns tells whether THIS add carried the word over the end of its range
// (every add sees its own old value, whatever the others do), and 2^64 hi units are 2^32 top units
__device__ __forceinline__ void plain_add_hi(unsigned long long *hi, unsigned long long *top, long long a) {
    if (!a) return;
    const long long old = (long long)atomicAdd(hi, (unsigned long long)a);
    const long long now = (long long)((unsigned long long)old + (unsigned long long)a);
    if (a > 0 && now < old) atomicAdd(top, 1ull << 32);
    if (a < 0 && now > old) atomicAdd(top, (unsigned long long)(-(1ll << 32)));
}
// lo += a, unsigned; a wrap is 2^64 = 2^32 hi units
__device__ __forceinline__ void plain_add_lo(unsigned long long *lo, unsigned long long *hi, unsigned long long *top, unsigned long long a) {
    if (!a) return;
    const unsigned long long old = atomicAdd(lo, a);
    if (old + a < old) plain_add_hi(hi, top, 1ll << 32);
}

__global__ __launch_bounds__(256) void k_pair_plain(DevParams P, PairArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x, B = A.bins;
    const bool valid = i < A.S.n;
    const float4 pi = A.S.position(valid ? i : 0), vi = A.S.velocity(valid ? i : 0);
    const uint32_t id = __float_as_uint(pi.w);
    int js[9], je[9];
    clipped_runs(P, A.S, pi, valid && id < (uint32_t)A.S.n, js, je);
    unsigned long long *row = A.partials;
    for_each_row_candidate(js, je, [&](int j) WALK_LAMBDA {
        const float4 c = A.S.position(j);
        if (!(linked(pi, c, A.r2) && __float_as_uint(c.w) > id)) return;
        const float d2 = link_d2(pi, c);
        int bin = 0;
        while (bin < B - 1 && A.edges2[bin] < d2) ++bin; // (the edges below d2 are a prefix of the table)
        const PairTerms T = pair_terms(pi, vi, c, A.S.velocity(j), d2);
        atomicAdd(&row[kPairCount * B + bin], 1ull);
        for (int s = 0; s < SPH_PAIR_SUMS; ++s) {
            unsigned long long *hi = &row[(kPairHi + s) * B + bin], *top = &row[(kPairTop + s) * B + bin];
            plain_add_lo(&row[(kPairLo + s) * B + bin], hi, top, term_lo(T.q[s]));
            plain_add_hi(hi, top, term_hi(T.q[s]));
        }
        if (T.sat) atomicAdd(&row[kPairSat * B + bin], (unsigned long long)T.sat);
    });
}

// ---- the join, both paths ----
// One wave per word of the table (item 0 the count, 1 .. 4 the sums, 5 the saturation count; bin b): every partial
// row's word as a 128-bit two's complement value -- lo + hi 2^32 + top 2^64, as body_moments.hip's finish joins two
// words, with the carry --, the rows' values added as four 32-bit limbs in 64-bit sums (below 2^32 rows), the limbs
// carried into each other once.
__global__ __launch_bounds__(64) void k_pair_join(PairArgs A) {
    const int B = A.bins, item = blockIdx.x / B, b = blockIdx.x - item * B, lane = threadIdx.x;
    unsigned long long limb[4] = {0ull, 0ull, 0ull, 0ull};
    for (int r = lane; r < A.rows; r += 64) {
        const unsigned long long *row = A.partials + (size_t)r * (kPairWords * B);
        unsigned long long lo, hi = 0ull;
        if (item == 0 || item == 5) {
            lo = row[(item == 0 ? kPairCount : kPairSat) * B + b];
        } else {
            const int s = item - 1;
            const unsigned long long L = row[(kPairLo + s) * B + b];
            const long long H = (long long)row[(kPairHi + s) * B + b];
            lo = L + ((unsigned long long)H << 32);
            hi = (unsigned long long)(H >> 32) + (lo < L ? 1ull : 0ull) + row[(kPairTop + s) * B + b];
        }
        limb[0] += lo & 0xFFFFFFFFull;
        limb[1] += lo >> 32;
        limb[2] += hi & 0xFFFFFFFFull;
        limb[3] += hi >> 32;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) limb[k] = wave_sum_u64(limb[k]);
    if (lane != 0) return;
    unsigned long long carry = limb[0];
    const unsigned long long w0 = carry & 0xFFFFFFFFull;
    carry = (carry >> 32) + limb[1];
    const unsigned long long w1 = carry & 0xFFFFFFFFull;
    carry = (carry >> 32) + limb[2];
    const unsigned long long w2 = carry & 0xFFFFFFFFull;
    carry = (carry >> 32) + limb[3];
    const unsigned long long lo = w0 | (w1 << 32), hi = w2 | (carry << 32); // (mod 2^128)
    SphPairBinRaw &out = A.out[b];
    if (item == 0) {
        out.pairs = lo;
        if (lo) atomicAdd(&A.counters[2], lo);
    } else if (item == 5) {
        out.saturated = lo;
    } else {
        out.sums[item - 1].lo = lo;
        out.sums[item - 1].hi = (long long)hi;
    }
}

// the call's table of edges into device memory, and an all-zero result
__global__ __launch_bounds__(SPH_PAIR_MAX_BINS) void k_pair_table(PairEdges E, float *edges2, unsigned long long *out, int bins) {
    const int t = threadIdx.x;
    if (t >= bins) return;
    edges2[t] = E.e[t];
    constexpr int kRowWords = (int)(sizeof(SphPairBinRaw) / sizeof(unsigned long long));
    for (int w = 0; w < kRowWords; ++w) out[t * kRowWords + w] = 0ull;
}

} // namespace

int sph_pair_rows(int n, int cus, bool plain, int workgroups) {
    if (plain || n <= 0) return 1;
    return max(1, min(blocks_of(n, 64), workgroups > 0 ? workgroups : max(cus, 1) * PAIR_WGS_PER_CU));
}

void sph_launch_pair_table(const PairEdges &E, const PairArgs &A, hipStream_t s) {
    k_pair_table<<<1, SPH_PAIR_MAX_BINS, 0, s>>>(E, const_cast<float *>(A.edges2), reinterpret_cast<unsigned long long *>(A.out), A.bins);
}

void sph_launch_pair_statistics(const DevParams &P, const PairArgs &A, bool plain, hipStream_t s) {
    if (A.S.n <= 0) return;
    if (plain) {
        (void)hipMemsetAsync(A.partials, 0, (size_t)kPairWords * A.bins * sizeof(unsigned long long), s);
        k_pair_plain<<<blocks_of(A.S.n, 256), 256, 0, s>>>(P, A);
    } else {
        (void)hipMemsetAsync(A.tile, 0, sizeof(unsigned int), s);
        const size_t lds = (size_t)kPairLdsWords * A.bins * sizeof(unsigned long long) + (size_t)A.bins * sizeof(float);
        k_pair_wave<<<A.rows, 64, lds, s>>>(P, A);
    }
    k_pair_join<<<6 * A.bins, 64, 0, s>>>(A);
}
