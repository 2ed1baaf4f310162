// Body tracks: the overlap of two labellings (section 10g) of the same particle ids -- the
// distinct pairs (previous body, current body) with the number of ids of each --, and from it which current body
// continues which previous one.  Integers only; every value is a count, a sum of counts or a maximum of packed words,
// so the words depend on the two labellings alone.
//
// Default path.  k_track_fold: a block takes kBodyFold x 256 consecutive rows of the sorted stream; each wave splits
// its 64 rows into groups of equal (previous, current) pair (next_group); groups of the pair of the block's first row
// are counted in LDS and leave the block once, every other group becomes one partial edge, kept in registers until the
// block has reserved its span of the partial buffer with ONE atomicAdd; the groups' leads then write into it.  The M
// partials are sorted by (current, previous) with two stable sorts (sort.hip), the first partial of every run of equal
// pairs is flagged and the flags scanned (scan_common.h): the number of edges and every partial's edge.
// k_track_reduce adds the partial counts onto their edge (a wave's partials of one edge are summed first),
// k_track_tally leaves the number of parents and children per body and the main parent / child as an atomicMax of
// count << 32 | ~row (k_body_table_finish's idiom: greatest count, smallest row on a tie).
//
// Check path (SPH_BODIES_PLAIN=1): every particle id is a partial of count 1, the same sorts and heads over all n; an
// edge's count is the distance between two heads; one thread per current body walks its run of edges, and after a
// stable sort of the edges by previous body one thread per previous body walks its run.  No atomics.
//
// Both: k_track_ids (the rows of this labelling in id order, the next reference), k_track_decide, the scan of the born
// flags, k_track_write, k_track_close.  Nothing waits for anything across workgroups; the loops are bounded -- a group
// loop loses a bit of `rest` per trip, a binary search halves its range (at most 32 trips), a walk ends with the edges.
#include "body_common.h"
#include "scan_common.h"

namespace {

static_assert(sizeof(SphBodyEdge) == 16 && sizeof(SphBodyTrack) == 24 && sizeof(SphBodyFate) == 32, "the rows of sph_c_api.h");

__device__ __forceinline__ unsigned long long best_word(uint32_t count, uint32_t row) { return ((unsigned long long)count << 32) | (unsigned long long)(~row); }
__device__ __forceinline__ uint32_t best_row(unsigned long long w) { return ~(uint32_t)(w & 0xFFFFFFFFull); }
__device__ __forceinline__ uint32_t best_count(unsigned long long w) { return (uint32_t)(w >> 32); }

// the pair of row i and its particle id; false: the row belongs to no pair (never for a state whose ids are a
// permutation of [0, n) and a reference of the same n)
__device__ __forceinline__ bool pair_of_row(const TrackArgs &A, int i, uint32_t &id, uint32_t &p, uint32_t &c) {
    const uint32_t n = (uint32_t)A.S.n;
    id = __float_as_uint(A.S.position(i).w);
    const uint32_t lab = A.rowLabel[i];
    p = c = 0u;
    if (id >= n || lab >= n) return false;
    c = A.rank[lab];
    p = A.prow[id];
    return c < (uint32_t)A.numBodies && p < (uint32_t)A.numPrev;
}

// partial `slot`: its pair and count, and the first sort's key and value
__device__ __forceinline__ void emit_partial(const TrackArgs &A, uint32_t slot, uint32_t p, uint32_t c, uint32_t count) {
    if (slot >= (uint32_t)A.S.n) return; // (never: a partial holds at least one row of its own)
    A.pPrev[slot] = p, A.pCur[slot] = c, A.pCount[slot] = count;
    A.ws.keys[0][slot] = p, A.ws.vals[0][slot] = slot;
}

__global__ __launch_bounds__(256) void k_track_fold(TrackArgs A) {
    __shared__ uint32_t foldCount, domPrev, domCur; // rows of the pair of the block's first row
    __shared__ uint32_t waveTotal[4], blockBase;     // partials of each wave; the block's span of the buffer
    const int base = blockIdx.x * (256 * kBodyFold);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        uint32_t id, p, c;
        const bool ok = pair_of_row(A, base, id, p, c); // (base < n: the grid is fold_blocks_of(n))
        domPrev = ok ? p : kNoId, domCur = ok ? c : kNoId; // (kNoId: no row of the block matches, nothing is folded)
        foldCount = 0u;
    }
    __syncthreads();
    const uint32_t dp = domPrev, dc = domCur;
    // trip k: the pair of the lane's row and, where the lane leads a group that leaves the wave as a partial, its rows
    uint32_t prevOf[kBodyFold], curOf[kBodyFold], mine[kBodyFold];
    uint32_t total = 0u; // the wave's partials
#pragma unroll
    for (int k = 0; k < kBodyFold; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        bool valid = i < A.S.n;
        uint32_t id;
        valid = pair_of_row(A, valid ? i : 0, id, prevOf[k], curOf[k]) && valid;
        mine[k] = 0u;
        unsigned long long rest = __ballot(valid);
        while (rest) {
            uint32_t p0, c0;
            int lead;
            const unsigned long long grp = next_group(prevOf[k], curOf[k], valid, rest, p0, c0, lead);
            if (p0 == dp && c0 == dc) {
                if (lane == lead) atomicAdd(&foldCount, (uint32_t)__popcll(grp));
            } else {
                mine[k] = lane == lead ? (uint32_t)__popcll(grp) : mine[k];
                total += 1u;
            }
        }
    }
    // the block's span of the buffer: ONE atomic on the counter (a wave's -- 16,384 a million rows -- are served one
    // after the other: measured, they were most of the launch)
    if (lane == 0) waveTotal[w] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = waveTotal[0] + waveTotal[1] + waveTotal[2] + waveTotal[3] + (foldCount != 0u ? 1u : 0u);
        blockBase = all ? atomicAdd(&A.counters->partials, all) : 0u;
    }
    __syncthreads();
    uint32_t at = blockBase;
#pragma unroll
    for (int q = 0; q < 4; ++q) at += q < w ? waveTotal[q] : 0u;
#pragma unroll
    for (int k = 0; k < kBodyFold; ++k) {
        const unsigned long long leads = __ballot(mine[k] != 0u);
        if (mine[k]) emit_partial(A, at + (uint32_t)__popcll(leads & ((1ull << lane) - 1ull)), prevOf[k], curOf[k], mine[k]);
        at += (uint32_t)__popcll(leads);
    }
    if (threadIdx.x == 255 && foldCount != 0u) emit_partial(A, at, dp, dc, foldCount); // (the last wave: `at` is the span's last slot)
}

// One thread per particle id, both paths: crow; and with `partials` (the check path) the id as a partial of count 1
__global__ __launch_bounds__(256) void k_track_ids(TrackArgs A, bool partials) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= A.S.n) return;
    const uint32_t lab = A.labels[id];
    uint32_t c = lab < (uint32_t)A.S.n ? A.rank[lab] : 0u;
    if (c >= (uint32_t)A.numBodies) c = 0u; // (never)
    A.crow[id] = c;
    if (!partials) return;
    uint32_t p = A.prow[id];
    if (p >= (uint32_t)A.numPrev) p = 0u; // (never)
    emit_partial(A, (uint32_t)id, p, c, 1u);
    if (id == 0) A.counters->partials = (uint32_t)A.S.n;
}

// between the two sorts: the second key of every partial, in the first sort's order
__global__ __launch_bounds__(256) void k_track_regather(TrackArgs A, int m, const uint32_t *order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t a = order[j]; // (order may be ws.vals[0] itself: the thread rewrites its own word)
    A.ws.keys[0][j] = a < (uint32_t)m ? A.pCur[a] : 0u;
    A.ws.vals[0][j] = a;
}

__global__ __launch_bounds__(256) void k_track_heads(TrackArgs A, int m, const uint32_t *order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    uint32_t hd = 1u;
    if (j > 0) {
        const uint32_t a = order[j], b = order[j - 1];
        hd = (A.pPrev[a] != A.pPrev[b] || A.pCur[a] != A.pCur[b]) ? 1u : 0u;
    }
    A.head[j] = hd;
}

// default path: the edges' counts and the per-body tallies start from zero (one launch, not five clears)
__global__ __launch_bounds__(256) void k_track_clear(TrackArgs A, int numEdges) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < numEdges) A.edges[i] = SphBodyEdge{0u, 0u, 0u, 0u};
    if (i < A.numBodies) A.parents[i] = 0u, A.bestParent[i] = 0ull;
    if (i < A.numPrev) A.children[i] = 0u, A.bestChild[i] = 0ull;
}

// default path: the heads write their edge's pair, every partial adds its count
__global__ __launch_bounds__(256) void k_track_reduce(TrackArgs A, int m, int numEdges, const uint32_t *order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = j < m;
    const uint32_t a = valid ? order[j] : 0u;
    const uint32_t hd = valid ? A.head[j] : 0u;
    const uint32_t e = valid ? A.edgeOf[j] + hd - 1u : 0u;
    valid = valid && e < (uint32_t)numEdges; // (never false: the scan's total is numEdges)
    const uint32_t count = valid ? A.pCount[a] : 0u;
    if (valid && hd) A.edges[e].prev = A.pPrev[a], A.edges[e].cur = A.pCur[a];
    uint32_t own = 0u; // the only partial of its edge in this wave
    unsigned long long rest = __ballot(valid);
    while (rest) {
        uint32_t e0;
        int lead;
        const unsigned long long grp = next_group(e, valid, rest, e0, lead);
        if (__popcll(grp) == 1) {
            own = lane == lead ? count : own;
            continue;
        }
        const uint32_t sum = wave_sum_u32(((grp >> lane) & 1) ? count : 0u);
        if (lane == lead) atomicAdd(&A.edges[e0].count, sum);
    }
    if (own) atomicAdd(&A.edges[e].count, own);
}

__global__ __launch_bounds__(256) void k_track_tally(TrackArgs A, int numEdges) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= numEdges) return;
    const SphBodyEdge ed = A.edges[e];
    if (ed.prev >= (uint32_t)A.numPrev || ed.cur >= (uint32_t)A.numBodies) return; // (never)
    atomicAdd(&A.parents[ed.cur], 1u);
    atomicAdd(&A.children[ed.prev], 1u);
    atomicMax(&A.bestParent[ed.cur], best_word(ed.count, ed.prev));
    atomicMax(&A.bestChild[ed.prev], best_word(ed.count, ed.cur));
}

// ---- the check path ----
__global__ __launch_bounds__(256) void k_track_run_heads(TrackArgs A, int m, int numEdges, const uint32_t *order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m || !A.head[j]) return;
    const uint32_t e = A.edgeOf[j];
    if (e >= (uint32_t)numEdges) return; // (never)
    const uint32_t a = order[j];
    A.edges[e].prev = A.pPrev[a], A.edges[e].cur = A.pCur[a];
    A.pCount[e] = (uint32_t)j; // (every partial's count is 1 here: the buffer holds the heads' positions instead)
}

__global__ __launch_bounds__(256) void k_track_run_counts(TrackArgs A, int m, int numEdges) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= numEdges) return;
    A.edges[e].count = (e + 1 < numEdges ? A.pCount[e + 1] : (uint32_t)m) - A.pCount[e];
}

// the first of [0, count) whose key is not below `want`; key(i) ascends
template <class Key>
__device__ __forceinline__ int lower_bound(int count, uint32_t want, Key key) {
    int lo = 0, hi = count;
    for (int trip = 0; trip < 32 && lo < hi; ++trip) { // (the range halves: 32 trips cover 2^31 edges)
        const int mid = lo + (hi - lo) / 2;
        if (key(mid) < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one thread per current body: its run of the edges (ascending previous row: a later edge wins only with more)
__global__ __launch_bounds__(256) void k_track_parents_plain(TrackArgs A, int numEdges) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= A.numBodies) return;
    uint32_t count = 0u;
    unsigned long long best = 0ull;
    for (int e = lower_bound(numEdges, (uint32_t)c, [&](int i) { return A.edges[i].cur; }); e < numEdges && A.edges[e].cur == (uint32_t)c; ++e) {
        const unsigned long long w = best_word(A.edges[e].count, A.edges[e].prev);
        best = w > best ? w : best;
        ++count;
    }
    A.parents[c] = count, A.bestParent[c] = best;
}

__global__ __launch_bounds__(256) void k_track_child_keys(TrackArgs A, int numEdges) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= numEdges) return;
    A.ws.keys[0][e] = A.edges[e].prev, A.ws.vals[0][e] = (uint32_t)e;
}

// one thread per previous body: its run of the edges sorted (stably) by previous row
__global__ __launch_bounds__(256) void k_track_children_plain(TrackArgs A, int numEdges, const uint32_t *keys, const uint32_t *order) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.numPrev) return;
    uint32_t count = 0u;
    unsigned long long best = 0ull;
    for (int k = lower_bound(numEdges, (uint32_t)p, [&](int i) { return keys[i]; }); k < numEdges && keys[k] == (uint32_t)p; ++k) {
        const uint32_t e = order[k];
        if (e >= (uint32_t)numEdges) break; // (never)
        const unsigned long long w = best_word(A.edges[e].count, A.edges[e].cur);
        best = w > best ? w : best;
        ++count;
    }
    A.children[p] = count, A.bestChild[p] = best;
}

// ---- both paths ----
// c continues p exactly when p is c's main parent and c is p's main child
__global__ __launch_bounds__(256) void k_track_decide(TrackArgs A) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= A.numBodies) return;
    uint32_t born = 1u;
    if (A.numPrev > 0 && A.parents[c] > 0u) {
        const uint32_t p = best_row(A.bestParent[c]);
        if (p < (uint32_t)A.numPrev && best_row(A.bestChild[p]) == (uint32_t)c) born = 0u;
    }
    A.head[c] = born;
}

__global__ __launch_bounds__(256) void k_track_write(TrackArgs A) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool valid = c < A.numBodies;
    bool merged = false, continues = false;
    if (valid) {
        const uint32_t np = A.numPrev > 0 ? A.parents[c] : 0u;
        const unsigned long long bp = np ? A.bestParent[c] : 0ull;
        const uint32_t born = A.head[c];
        merged = np >= 2u, continues = !born;
        SphBodyTrack t;
        t.track = born ? *A.nextTrack + (unsigned long long)A.edgeOf[c] : A.prevTrack[best_row(bp)];
        t.parents = np;
        t.main_parent = np ? best_row(bp) : kNoId;
        t.main_overlap = best_count(bp);
        t.flags = (born ? SPH_TRACK_BORN : SPH_TRACK_CONTINUES) | (merged ? SPH_TRACK_MERGED : 0);
        A.tracks[c] = t;
        A.curTrack[c] = t.track;
        A.curBody[c] = make_uint2(A.table[8 * (size_t)c], A.table[8 * (size_t)c + 1]);
    }
    const unsigned long long m = __ballot(merged), k = __ballot(continues);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(&A.counters->merges, (uint32_t)__popcll(m));
        if (k) atomicAdd(&A.counters->continued, (uint32_t)__popcll(k));
    }
}

// One launch for what is left: the fates of the previous bodies, the edges' flags, and next_track (k_track_write, the
// launch before, has read the old value)
__global__ __launch_bounds__(256) void k_track_close(TrackArgs A, int numEdges) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool split = false, ended = false;
    if (i < A.numPrev) {
        const uint32_t nc = A.children[i];
        const unsigned long long bc = A.bestChild[i];
        const uint32_t mc = best_row(bc);
        const bool continues = nc > 0u && mc < (uint32_t)A.numBodies && best_row(A.bestParent[mc]) == (uint32_t)i;
        split = nc >= 2u, ended = !continues;
        SphBodyFate f;
        f.track = A.prevTrack[i];
        f.label = A.prevBody[i].x, f.count = A.prevBody[i].y;
        f.children = nc;
        f.main_child = nc ? mc : kNoId;
        f.main_overlap = best_count(bc);
        f.flags = (continues ? SPH_FATE_CONTINUES : SPH_FATE_ENDED) | (split ? SPH_FATE_SPLIT : 0);
        A.fates[i] = f;
    }
    const unsigned long long s = __ballot(split), x = __ballot(ended);
    if ((threadIdx.x & 63) == 0) {
        if (s) atomicAdd(&A.counters->splits, (uint32_t)__popcll(s));
        if (x) atomicAdd(&A.counters->ended, (uint32_t)__popcll(x));
    }
    if (i < numEdges) {
        const uint32_t p = A.edges[i].prev, c = A.edges[i].cur;
        if (p < (uint32_t)A.numPrev && c < (uint32_t)A.numBodies) // (never false)
            A.edges[i].flags = (best_row(A.bestParent[c]) == p ? SPH_EDGE_MAIN_PARENT : 0) | (best_row(A.bestChild[p]) == c ? SPH_EDGE_MAIN_CHILD : 0);
    }
    if (i == 0) {
        const unsigned long long next = *A.nextTrack + (unsigned long long)A.counters->born;
        *A.nextTrack = next;
        A.counters->nextTrack = next;
    }
}

// key bits of rows [0, count)
int row_bits(int count) {
    int bits = 1;
    while (bits < 31 && (1ll << bits) < (long long)count) ++bits;
    return bits;
}

} // namespace

int sph_track_scan_blocks(int n) { return scan_blocks(n); }

void sph_launch_track_partials(const TrackArgs &A, bool plain, hipStream_t s) {
    (void)hipMemsetAsync(A.counters, 0, sizeof(TrackCounters), s);
    if (A.S.n <= 0 || A.numBodies <= 0) return;
    // (crow in id order, coalesced: written from the fold it would be a scatter of single words)
    const bool ids = plain && A.numPrev > 0;
    k_track_ids<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A, ids);
    if (A.numPrev > 0 && !plain) k_track_fold<<<fold_blocks_of(A.S.n), 256, 0, s>>>(A);
}

int sph_launch_track_sort(const TrackArgs &A, int m, hipStream_t s) {
    if (m <= 0) return 0;
    const int first = sph_sort_pairs(A.ws, m, row_bits(A.numPrev), s);
    k_track_regather<<<blocks_of(m, 256), 256, 0, s>>>(A, m, A.ws.vals[first]);
    const int order = sph_sort_pairs(A.ws, m, row_bits(A.numBodies), s);
    k_track_heads<<<blocks_of(m, 256), 256, 0, s>>>(A, m, A.ws.vals[order]);
    launch_exclusive_scan<uint32_t>(A.head, m, A.blockSum, A.edgeOf, &A.counters->edges, nullptr, s);
    return order;
}

void sph_launch_track_edges(const TrackArgs &A, int m, int numEdges, int order, bool plain, hipStream_t s) {
    if (m <= 0 || numEdges <= 0) return;
    if (!plain) {
        const int most = numEdges > A.numBodies ? (numEdges > A.numPrev ? numEdges : A.numPrev) : (A.numBodies > A.numPrev ? A.numBodies : A.numPrev);
        k_track_clear<<<blocks_of(most, 256), 256, 0, s>>>(A, numEdges);
        k_track_reduce<<<blocks_of(m, 256), 256, 0, s>>>(A, m, numEdges, A.ws.vals[order]);
        k_track_tally<<<blocks_of(numEdges, 256), 256, 0, s>>>(A, numEdges);
        return;
    }
    k_track_run_heads<<<blocks_of(m, 256), 256, 0, s>>>(A, m, numEdges, A.ws.vals[order]);
    k_track_run_counts<<<blocks_of(numEdges, 256), 256, 0, s>>>(A, m, numEdges);
    k_track_parents_plain<<<blocks_of(A.numBodies, 256), 256, 0, s>>>(A, numEdges);
    k_track_child_keys<<<blocks_of(numEdges, 256), 256, 0, s>>>(A, numEdges);
    const int r = sph_sort_pairs(A.ws, numEdges, row_bits(A.numPrev), s);
    k_track_children_plain<<<blocks_of(A.numPrev, 256), 256, 0, s>>>(A, numEdges, A.ws.keys[r], A.ws.vals[r]);
}

void sph_launch_track_assign(const TrackArgs &A, int numEdges, hipStream_t s) {
    if (A.S.n <= 0 || A.numBodies <= 0) return;
    k_track_decide<<<blocks_of(A.numBodies, 256), 256, 0, s>>>(A);
    launch_exclusive_scan<uint32_t>(A.head, A.numBodies, A.blockSum, A.edgeOf, &A.counters->born, nullptr, s);
    k_track_write<<<blocks_of(A.numBodies, 256), 256, 0, s>>>(A);
    const int most = numEdges > A.numPrev ? numEdges : A.numPrev;
    k_track_close<<<blocks_of(most > 0 ? most : 1, 256), 256, 0, s>>>(A, numEdges);
}
