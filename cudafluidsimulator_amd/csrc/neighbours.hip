// Neighbour lists: for every particle of the current state the ids of the particles within a
// radius, as CSR in particle-id order.  The test is the bodies' link test (walk_common.h), fp32 with every operation
// rounded on its own (-ffp-contract=off), whatever the handle's math mode; everything after it is integers.
//
// count -> scan -> emit -> sort, four launches, nothing waits for anything inside one: no barrier across workgroups,
// no flag is polled, every loop is bounded.
//
// Count and emit are one templated walk (nbr_take): row i walks what the density sweep walks, the nine runs of
// load_runs (sweep_common.h) around sweep_cell of its own position, each in stream order.  The default path is
// derived.hip's, the staged walk of walk_common.h (walk_runs_staged): one wave per 64 consecutive rows, for each of the
// nine runs the UNION of the lanes' ranges staged in LDS -- here as 16-byte records (x, y, z, id) --, a selected test;
// a run whose union is longer than the slice is walked by every lane from global memory in the same order.  The
// count adds a selected 0 / 1; the emit stores the id under a mask (integers: nothing to select) at
// neighbours[offsets[id] + k++], so a list is in the order of the walk.  The check path (SPH_NEIGHBOURS_PLAIN=1) is
// one thread per row with every candidate from global memory.
//
// The scan is scan_common.h's with 64-bit sums, over the n counts in id order.
//
// The sort puts every list in ascending order, in place.  Ids are distinct, so the rank of an id -- how many ids of
// its list are smaller -- is its place.  Default path: one wave per kSortLists consecutive lists, which are one
// contiguous stretch of `neighbours`.  As many of them as fit kSortSlice entries are staged in LDS together and ranked
// there, one ENTRY per lane (never one list per lane: the lanes of one list read the same LDS word in the same trip, a
// broadcast); how the entries are dealt to the lanes depends on the lists' lengths (rank_staged).  A list longer than the slice
// is sorted by odd-even transposition over chunks of half a slice: the window of two adjacent chunks is staged,
// ranked as one list and stored back, C phases for C chunks -- the contents of the chunks after a phase do not depend
// on the order inside them, so this is the textbook merge-split network, and every chunk has been in a window by the
// end (C >= 3).  The windows of a list are stored and staged again by the same one-wave workgroup, a barrier between.
// Check path: one thread per list, heapsort in global memory.
#include "scan_common.h"
#include "walk_common.h"

namespace {

// (A/B builds for scripts/studies/neighbours.py: -DNBR_SLICE=..., -DNBR_SORT_SLICE=..., -DNBR_SORT_LISTS=...; the
// defaults are the measured choices of DESIGN.md section 10j)
// Measured on an MI355X at n = 4,194,304, `-i random`, ms per launch after step 20 / after step 100 (141,955,298
// entries, longest list 68 / 802,064,494 entries, longest 533), medians of 5 rounds, spread below 1 %:
//   shipped: count 0.885 / 2.130, scan 0.049 / 0.050, emit 1.232 / 4.538, sort 0.852 / 15.50; check path: 1.272 / 4.139,
//   0.049 / 0.049, 1.883 / 6.880, 12.94 / 192.7; k_derive_wave on the same states in the same rounds: 1.386 / 5.905.
#ifndef NBR_SLICE
#define NBR_SLICE 640 // kNbrSlice, tests/test_gpu_neighbours.py's SLICE: staged candidates per run of the count and
                      // emit walks: 10 KB of 16-byte records, the LDS of derived.hip's 320 32-byte records (16
                      // one-wave workgroups per CU) with twice the rows.  count / emit: 320: 0.953 / 2.686 and
                      // 1.307 / 6.045 (a fifth of the late runs walk from global memory), 640: 0.885 / 2.125 and
                      // 1.231 / 4.628, 1024: 1.154 / 3.222 and 1.445 / 4.481 (10 resident waves per CU)
#endif
#ifndef NBR_SORT_SLICE
#define NBR_SORT_SLICE 1024 // kSortSlice, the tests' SORT_SLICE: entries the sort stages at once, 4 KB of ids; a longer
                            // list takes the chunked path.  sort: 512: 0.807 / 23.64, 1024: 0.771 / 23.18,
                            // 2048: 1.080 / 30.85 (before the list-by-list dealing below; with it 2048: 1.127 / 16.35)
#endif
#ifndef NBR_SORT_LISTS
#define NBR_SORT_LISTS 64 // consecutive lists per wave of the sort.  sort, entry dealing alone: 1 (a wave per list):
                          // 1.438 / 16.73, 16: 0.779 / 22.16, 64: 0.771 / 23.18; with the list-by-list dealing:
                          // 1: 1.416 / 15.43, 16: 0.871 / 15.06, 64: 0.852 / 15.50
#endif
#ifndef NBR_SORT_WIDE
#define NBR_SORT_WIDE 64 // a batch whose lists hold this many entries or more on average is ranked list by list
                         // (rank_staged).  sort: 32: 0.903 / 15.60, 64: 0.852 / 15.50, 128: 0.826 / 16.16
#endif
constexpr int kSortWide = NBR_SORT_WIDE;
constexpr int kNbrSlice = NBR_SLICE;
constexpr int kNbrTrip = 4; // candidates per trip of the staged walk, as derived.hip's
constexpr int kSortSlice = NBR_SORT_SLICE;
constexpr int kSortLists = NBR_SORT_LISTS;
static_assert(kSortLists >= 1 && kSortLists <= 64 && kSortSlice >= 4 && kSortSlice % 2 == 0, "one lane per list of a batch");

// One candidate c of the row (pi, id): taken when it is the lane's (mine), within the radius and another particle.
// Count: k += 0 / 1.  Emit: the id goes to out[k] first (out = the row's list, room = its length as counted: the
// same walk took as many, the bound only keeps a store inside the list whatever happens).
template <bool kEmit>
__device__ __forceinline__ void nbr_take(const float4 pi, uint32_t id, float r2, const float4 c, bool mine, uint32_t *out, uint32_t room,
                                         uint32_t &k) {
    const uint32_t cid = __float_as_uint(c.w);
    const bool take = mine && linked(pi, c, r2) && cid != id;
    if constexpr (kEmit) {
        if (take && k < room) out[k] = cid;
    }
    k += take ? 1u : 0u;
}

// what a row needs before its walk: its words, whether it takes part, its runs, and (emit) its list
template <bool kEmit>
struct NbrRow {
    float4 pi;
    uint32_t id;
    bool ok; // a row of the stream whose id is one (the ids of a state are a permutation of [0, n): always)
    int js[9], je[9];
    uint32_t *out = nullptr;
    uint32_t room = 0, k = 0;
    __device__ __forceinline__ NbrRow(const DevParams &P, const NeighbourArgs &A, int i) {
        const bool valid = i < A.S.n;
        pi = A.S.position(valid ? i : 0);
        id = __float_as_uint(pi.w);
        ok = valid && id < (uint32_t)A.S.n;
        clipped_runs(P, A.S, pi, ok, js, je); // (not ok: nine empty runs)
        if (kEmit && ok) out = A.neighbours + A.offsets[id], room = A.counts[id];
    }
    // count: the length to the id's slot, the longest of the wave to totals[1]
    __device__ __forceinline__ void finish(const NeighbourArgs &A) const {
        if constexpr (!kEmit) {
            if (ok) A.counts[id] = k;
            const int longest = wave_max_i32(ok ? (int)k : 0); // (k < n <= INT_MAX)
            if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(&A.totals[1], (unsigned long long)longest);
        }
    }
};

// the check path: one thread per row of the sorted stream, every candidate from global memory
template <bool kEmit>
__global__ __launch_bounds__(256) void k_nbr_plain(DevParams P, NeighbourArgs A) {
    NbrRow<kEmit> R(P, A, blockIdx.x * 256 + threadIdx.x);
    for_each_row_candidate(R.js, R.je, [&](int j) WALK_LAMBDA { nbr_take<kEmit>(R.pi, R.id, A.r2, A.S.position(j), true, R.out, R.room, R.k); });
    R.finish(A);
}

// One wave per 64 consecutive rows of the sorted stream.
template <bool kEmit>
__global__ __launch_bounds__(64) void k_nbr_wave(DevParams P, NeighbourArgs A) {
    __shared__ float4 slice[kNbrSlice];
    const int lane = threadIdx.x;
    NbrRow<kEmit> R(P, A, blockIdx.x * 64 + lane);
    uint32_t staged = 0, direct = 0;
    walk_runs_staged<1, kNbrSlice, kNbrTrip>(
        A.S, R.js, R.je, slice, staged, direct,
        [&](int j) WALK_LAMBDA { nbr_take<kEmit>(R.pi, R.id, A.r2, A.S.position(j), true, R.out, R.room, R.k); },
        [&](const float4(&c)[1], bool mine) WALK_LAMBDA { nbr_take<kEmit>(R.pi, R.id, A.r2, c[0], mine, R.out, R.room, R.k); });
    if (lane == 0) {
        if (staged) atomicAdd(&A.counters[0], (unsigned long long)staged);
        if (direct) atomicAdd(&A.counters[1], (unsigned long long)direct);
    }
    R.finish(A);
}

// ---- the sort ----
// `cnt` staged entries (slice[0, cnt), between two barriers of the caller's) hold `m` lists back to back, list q at
// [lo[q], lo[q + 1]) (lo[m] = cnt; empty lists among them): every entry's rank in its list is its place in dst.
// Two ways of dealing the entries to the lanes, picked per batch (wave-uniform).  Short lists: entry e to lane e mod 64,
// whatever list it is in -- every lane has work, the lanes of one list read the same word in the same trip, and a
// trip lasts as long as the longest list among its lanes.  Long lists (kSortWide entries or more on average): one list
// after the other, its entries to the lanes -- every lane of a trip ranks against the same list, so the trip count is
// uniform, nothing waits for a longer neighbour, and the list is read four ids to a 16-byte broadcast.
__device__ __forceinline__ void rank_staged(const uint32_t *slice, const uint32_t *lo, int m, int cnt, uint32_t *dst) {
    if (cnt < kSortWide * m) {
        int q = 0;
        for (int e = threadIdx.x; e < cnt; e += 64) {
            while (q < m - 1 && (uint32_t)e >= lo[q + 1]) ++q; // (at most m - 1 steps over the whole loop)
            const uint32_t ls = lo[q], le = lo[q + 1];
            const uint32_t mine = slice[e];
            uint32_t rank = 0;
            for (uint32_t t = ls; t < le; ++t) rank += slice[t] < mine ? 1u : 0u;
            dst[ls + rank] = mine; // (rank < le - ls: the entry itself is not below itself)
        }
        return;
    }
    for (int q = 0; q < m; ++q) {
        const uint32_t ls = lo[q], le = lo[q + 1]; // (the same in every lane)
        const uint32_t head = min((ls + 3u) & ~3u, le), body = head + ((le - head) & ~3u);
        for (uint32_t e = ls + threadIdx.x; e < le; e += 64) {
            const uint32_t mine = slice[e];
            uint32_t rank = 0;
            for (uint32_t t = ls; t < head; ++t) rank += slice[t] < mine ? 1u : 0u;
            for (uint32_t t = head; t < body; t += 4) {
                const uint4 v = *reinterpret_cast<const uint4 *>(slice + t); // (t is a multiple of 4, the slice 16-byte aligned)
                rank += (v.x < mine ? 1u : 0u) + (v.y < mine ? 1u : 0u) + (v.z < mine ? 1u : 0u) + (v.w < mine ? 1u : 0u);
            }
            for (uint32_t t = body; t < le; ++t) rank += slice[t] < mine ? 1u : 0u;
            dst[ls + rank] = mine;
        }
    }
}

// a list longer than the slice: odd-even transposition over chunks of half a slice (the top of this file)
__device__ __forceinline__ void sort_long(uint32_t *list, uint64_t len, uint32_t *slice, uint32_t *lo) {
    constexpr uint64_t kHalf = kSortSlice / 2;
    const uint64_t chunks = (len + kHalf - 1) / kHalf;
    for (uint64_t phase = 0; phase < chunks; ++phase)
        for (uint64_t c = phase & 1; c + 1 < chunks; c += 2) {
            uint32_t *window = list + c * kHalf;
            const uint64_t rest = len - c * kHalf;
            const int cnt = (int)(rest < (uint64_t)kSortSlice ? rest : (uint64_t)kSortSlice);
            if (threadIdx.x == 0) lo[0] = 0, lo[1] = (uint32_t)cnt;
            for (int t = threadIdx.x; t < cnt; t += 64) slice[t] = window[t];
            __syncthreads();
            rank_staged(slice, lo, 1, cnt, window);
            __syncthreads(); // the window is stored (the next one reads half of it) and the slice is free again
        }
}

// One wave per kSortLists consecutive lists.
__global__ __launch_bounds__(64) void k_nbr_sort_wave(NeighbourArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t slice[kSortSlice];
    __shared__ uint32_t lo[kSortLists + 1];
    const int lane = threadIdx.x;
    const int first = blockIdx.x * kSortLists;
    const int lists = min(kSortLists, A.S.n - first);
    // lane l: where list first + l begins and ends
    const bool has = lane < lists;
    const unsigned long long s = has ? A.offsets[first + lane] : 0ull, e = has ? A.offsets[first + lane + 1] : 0ull;
    int a = 0; // the first list not sorted yet (wave-uniform); every trip takes at least one
    for (int trip = 0; trip < kSortLists && a < lists; ++trip) {
        const unsigned long long base = __shfl(s, a);
        // the lists a, a + 1, ... that end within a slice of base (their ends ascend: a prefix)
        const int m = __popcll(__ballot(has && lane >= a && e - base <= (unsigned long long)kSortSlice));
        if (m == 0) {
            sort_long(A.neighbours + base, __shfl(e, a) - base, slice, lo);
            a += 1;
            continue;
        }
        const int cnt = (int)(__shfl(e, a + m - 1) - base);
        if (lane >= a && lane < a + m) lo[lane - a] = (uint32_t)(s - base);
        if (lane == 0) lo[m] = (uint32_t)cnt;
        for (int t = lane; t < cnt; t += 64) slice[t] = A.neighbours[base + t];
        __syncthreads();
        rank_staged(slice, lo, m, cnt, A.neighbours + base);
        __syncthreads(); // slice and lo have been read: the next batch may overwrite them
        a += m;
    }
}

// the check path: one thread per list, heapsort in place in global memory (every loop bounded by the list's length)
__device__ __forceinline__ void sift_down(uint32_t *a, uint32_t root, uint32_t end) {
    const uint32_t v = a[root];
    while (2 * (uint64_t)root + 1 < end) {
        uint32_t child = 2 * root + 1;
        uint32_t cv = a[child];
        if (child + 1 < end) {
            const uint32_t rv = a[child + 1];
            if (rv > cv) child += 1, cv = rv;
        }
        if (cv <= v) break;
        a[root] = cv;
        root = child;
    }
    a[root] = v;
}

__global__ __launch_bounds__(256) void k_nbr_sort_plain(NeighbourArgs A) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= A.S.n) return;
    const uint64_t begin = A.offsets[id], len64 = A.offsets[id + 1] - begin;
    if (len64 < 2 || len64 > 0xFFFFFFFFull) return; // (a list is shorter than n)
    uint32_t *a = A.neighbours + begin;
    const uint32_t len = (uint32_t)len64;
    for (uint32_t start = len / 2; start-- > 0;) sift_down(a, start, len);
    for (uint32_t end = len - 1; end > 0; --end) {
        const uint32_t top = a[0];
        a[0] = a[end];
        a[end] = top;
        sift_down(a, 0, end);
    }
}

} // namespace

int sph_neighbour_scan_blocks(int n) { return scan_blocks(n); }

void sph_launch_neighbour_count(const DevParams &P, const NeighbourArgs &A, bool plain, hipStream_t s) {
    if (A.S.n <= 0) return;
    (void)hipMemsetAsync(A.totals, 0, 2 * sizeof(unsigned long long), s);
    if (plain) k_nbr_plain<false><<<blocks_of(A.S.n, 256), 256, 0, s>>>(P, A);
    else k_nbr_wave<false><<<blocks_of(A.S.n, 64), 64, 0, s>>>(P, A);
}

void sph_launch_neighbour_scan(const NeighbourArgs &A, hipStream_t s) {
    if (A.S.n <= 0) return;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are scanned as unsigned long long");
    unsigned long long *offsets = reinterpret_cast<unsigned long long *>(A.offsets);
    launch_exclusive_scan<unsigned long long>(A.counts, A.S.n, A.blockSum, offsets, &A.totals[0], offsets + A.S.n, s);
}

void sph_launch_neighbour_emit(const DevParams &P, const NeighbourArgs &A, bool plain, hipStream_t s) {
    if (A.S.n <= 0) return;
    if (plain) k_nbr_plain<true><<<blocks_of(A.S.n, 256), 256, 0, s>>>(P, A);
    else k_nbr_wave<true><<<blocks_of(A.S.n, 64), 64, 0, s>>>(P, A);
}

void sph_launch_neighbour_sort(const NeighbourArgs &A, bool plain, hipStream_t s) {
    if (A.S.n <= 0) return;
    if (plain) k_nbr_sort_plain<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A);
    else k_nbr_sort_wave<<<blocks_of(A.S.n, kSortLists), 64, 0, s>>>(A);
}
