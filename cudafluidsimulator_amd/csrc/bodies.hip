// Bodies: the connected components of the link graph over the particles of the current
// state -- two particles are linked when d2 <= r2 --, every particle's label (the smallest particle id of its
// component) and one table row per component.  The link test is fp32, every operation rounded on its own
// (-ffp-contract=off), whatever the handle's math mode; everything after it is integers.
//
// Default path: a concurrent union-find over the rows of the sorted stream.  parent[x] <= x always, and a row whose
// parent is itself is a root.  The one thing that ever changes a root is atomicCAS(&parent[a], a, b) with b < a, so a
// row that has a parent never becomes a root again, every value parent[x] ever held is a row of x's own component,
// and a climb -- however old the values it reads -- ends at a row of that component: two climbs that meet have proved
// the rows connected, and whether a row still IS a root is decided by the value the CAS returns and by nothing else.
// Nothing waits for anything: no barrier across workgroups, no flag is polled, the phases are separate launches.
// (Climbs also halve the paths behind them with atomicMin(&parent[x], grandparent): parent[] only ever falls, which
// keeps all of the above.)  Every loop is bounded: each trip of unite() makes one of its two cursors strictly smaller
// (a climb step goes to a parent below the row; a CAS that fails returns the row's parent, which is below it), the
// cursors start below n, so it ends within 2n trips; a lane that reaches the bound of 2n + 2 counts itself in
// counters->gaveUp and leaves its loops.
//
// Check path (SPH_BODIES_PLAIN=1): another algorithm, min-label propagation.  Every row starts with its particle id
// and takes the minimum over itself and its linked neighbours, all 27 cells from global memory, one launch per
// round, until a round changes nothing.
//
// Both paths then share mark + scan (which particle ids are labels, and how many labels lie below each: the scan of
// scan_common.h) and the table launches.  Candidates are read from global memory on both paths (no LDS staging;
// section 10g says why).
#include "body_common.h"
#include "scan_common.h"
#include "walk_common.h"

namespace {

// a load that is served by the device's coherent level, never by this CU's L1 (the forest and the check path's
// labels change under the launch that reads them)
__device__ __forceinline__ uint32_t load_shared(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t trip_bound(int n) {
    const unsigned long long b = 2ull * (unsigned long long)n + 2ull;
    return b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}

// One climb to the root of row a's tree as this lane sees it.  Every step halves the path behind it: a row that is
// not a root is handed its grandparent (atomicMin: parent[] only ever falls, and a row that has a parent keeps one).
// The cursor falls with every trip; a lane whose budget runs out sets gave and stops where it is.
__device__ __forceinline__ uint32_t climb(const BodyArgs &A, uint32_t a, uint32_t &budget, bool &gave) {
    if (gave) return a;
    uint32_t p = min(load_shared(&A.parent[a]), a); // (parent[a] <= a always: min() keeps the cursor falling whatever is read)
    while (p != a) {
        const uint32_t gp = min(load_shared(&A.parent[p]), p);
        if (gp != p) atomicMin(&A.parent[a], gp);
        a = p, p = gp;
        if (--budget == 0) {
            gave = true;
            break;
        }
    }
    return a;
}

// Merges the trees that hold rows a and b and returns a row of the merged tree at or near its root (the caller's next
// cursor).
__device__ __forceinline__ uint32_t unite(const BodyArgs &A, uint32_t a, uint32_t b, uint32_t budget, uint32_t &unions, bool &gave) {
    while (!gave) {
        a = climb(A, a, budget, gave);
        b = climb(A, b, budget, gave);
        if (gave || a == b) break;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        // a > b, both roots as far as this lane has seen: the CAS's own answer says whether a still is one
        const uint32_t old = atomicCAS(&A.parent[a], a, b);
        if (old == a) {
            unions += 1;
            return b;
        }
        a = min(old, a); // a has a parent by now (old < a): go on from there
        if (--budget == 0) gave = true;
    }
    return min(a, b);
}

// first launch of a call: every row its own tree (check path: its own label), no particle id a label yet
__global__ __launch_bounds__(256) void k_body_clear(BodyArgs A, bool plain) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.S.n) return;
    A.flag[i] = 0;
    if (plain) {
        A.rowLabel[i] = __float_as_uint(A.S.position(i).w);
    } else {
        A.parent[i] = (uint32_t)i;
        A.rootId[i] = kNoId;
    }
}

// The link sweep: row i tests the rows before it in the stream among its 27 cells -- the runs of dz = -1, the run
// dz = 0, dy = -1 and its own run up to itself (the later runs hold later rows only: the stream is in cell order) --
// so every unordered pair is met once, by its later row.
__global__ __launch_bounds__(256) void k_body_link(DevParams P, BodyArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < A.S.n;
    const float4 pi = A.S.position(valid ? i : 0);
    int js[9], je[9];
    clipped_runs(P, A.S, pi, valid, js, je);
    const uint32_t budget = trip_bound(A.S.n);
    uint32_t links = 0, unions = 0;
    bool gave = false;
    uint32_t mine = (uint32_t)(valid ? i : 0); // a row of i's tree, at or near its root
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int end = min(je[r], i);
        for (int j = js[r]; j < end; ++j) {
            if (!linked(pi, A.S.position(j), A.r2)) continue;
            links += 1;
            // j hangs right under mine: one tree already (whatever parent[j] holds is a row of j's component)
            if (load_shared(&A.parent[j]) == mine) continue;
            mine = unite(A, mine, (uint32_t)j, budget, unions, gave);
        }
    }
    // (mine is a row of i's tree at or below i: the next climb from i starts there)
    if (valid && !gave && mine != (uint32_t)i) atomicMin(&A.parent[i], mine);
    const uint32_t wl = wave_sum_u32(links), wu = wave_sum_u32(unions);
    if ((threadIdx.x & 63) == 0) {
        if (wl) atomicAdd(&A.counters->links, (unsigned long long)wl);
        if (wu) atomicAdd(&A.counters->unions, (unsigned long long)wu);
    }
    if (gave) atomicAdd(&A.counters->gaveUp, 1u);
}

// root[i]: the links are all in (they were made by an earlier launch), so the root a climb ends at is the tree's; the
// climbs go on halving paths for each other, which moves no row to another tree
__global__ __launch_bounds__(256) void k_body_flatten(BodyArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.S.n) return;
    uint32_t budget = trip_bound(A.S.n);
    bool gave = false;
    A.root[i] = climb(A, (uint32_t)i, budget, gave);
    if (gave) atomicAdd(&A.counters->gaveUp, 1u);
}

// rootId[root] = the smallest particle id of the tree (next_group, kBodyFold: body_common.h)
__global__ __launch_bounds__(256) void k_body_root_id(BodyArgs A) {
    __shared__ uint32_t fold[2]; // the root of the block's first row, the smallest id seen under it
    const int base = blockIdx.x * (256 * kBodyFold);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) fold[0] = A.root[base], fold[1] = kNoId;
    __syncthreads();
    const uint32_t dom = fold[0];
#pragma unroll 1
    for (int k = 0; k < kBodyFold; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        const bool valid = i < A.S.n;
        const uint32_t rt = valid ? A.root[i] : 0u;
        const uint32_t id = valid ? __float_as_uint(A.S.position(i).w) : kNoId;
        unsigned long long rest = __ballot(valid);
        while (rest) {
            uint32_t r0;
            int lead;
            const unsigned long long grp = next_group(rt, valid, rest, r0, lead);
            const bool in = (grp >> lane) & 1;
            const uint32_t m = __popcll(grp) == 1 ? id : wave_min_u32(in ? id : kNoId);
            if (lane == lead) {
                if (r0 == dom) atomicMin(&fold[1], m);
                else atomicMin(&A.rootId[r0], m);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && fold[1] != kNoId) atomicMin(&A.rootId[dom], fold[1]);
}

// rowLabel (default path: from the roots) and the flag of every particle id that is a label
__global__ __launch_bounds__(256) void k_body_mark(BodyArgs A, bool plain) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.S.n) return;
    const uint32_t id = __float_as_uint(A.S.position(i).w);
    uint32_t lab;
    if (plain) lab = A.rowLabel[i];
    else A.rowLabel[i] = lab = A.rootId[A.root[i]];
    if (lab == id && id < (uint32_t)A.S.n) A.flag[id] = 1;
}

// ---- the check path's round ----
__global__ __launch_bounds__(256) void k_body_plain_round(DevParams P, BodyArgs A, bool first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < A.S.n;
    const float4 pi = A.S.position(valid ? i : 0);
    int js[9], je[9];
    clipped_runs(P, A.S, pi, valid, js, je);
    const uint32_t mine = valid ? load_shared(&A.rowLabel[i]) : 0u;
    uint32_t m = mine, links = 0;
    for_each_row_candidate(js, je, [&](int j) WALK_LAMBDA {
        if (j == i || !linked(pi, A.S.position(j), A.r2)) return;
        links += j < i ? 1u : 0u;
        m = min(m, load_shared(&A.rowLabel[j]));
    });
    const bool lower = valid && m < mine;
    if (lower) __hip_atomic_store(&A.rowLabel[i], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (its only writer)
    const unsigned long long any = __ballot(lower);
    const uint32_t wl = first ? wave_sum_u32(links) : 0u;
    if ((threadIdx.x & 63) == 0) {
        if (any) atomicOr(&A.counters->changed, 1u);
        if (wl) atomicAdd(&A.counters->links, (unsigned long long)wl);
    }
}

// ---- the table ----
// the row of every label: label, count 0, the identities of the key minima and maxima
__global__ __launch_bounds__(256) void k_body_table_init(BodyArgs A, int numBodies) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= A.S.n || !A.flag[id]) return;
    const uint32_t b = A.rank[id];
    if (b >= (uint32_t)numBodies) return; // (never: the ranks of the flagged ids are 0 .. numBodies - 1)
    uint32_t *t = A.table + 8 * (size_t)b;
    t[0] = (uint32_t)id;
    t[1] = 0;
    t[2] = t[3] = t[4] = 0xFFFFFFFFu;
    t[5] = t[6] = t[7] = 0;
}

// (t: a table row in global memory, or the block's fold in LDS)
__device__ __forceinline__ void body_row_add(uint32_t *t, uint32_t count, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t x1, uint32_t y1, uint32_t z1) {
    atomicAdd(&t[1], count);
    atomicMin(&t[2], x0), atomicMin(&t[3], y0), atomicMin(&t[4], z0);
    atomicMax(&t[5], x1), atomicMax(&t[6], y1), atomicMax(&t[7], z1);
}

// every row into its body's table row, its label to its particle id's slot; one set of atomics per group of a wave's
// rows that share their body, the groups of the block's first body folded in LDS first
__global__ __launch_bounds__(256) void k_body_table_fill(BodyArgs A, int numBodies) {
    __shared__ uint32_t fold[8]; // laid out as a table row; [0]: the body of the block's first row
    const int base = blockIdx.x * (256 * kBodyFold);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        const uint32_t lab = A.rowLabel[base];
        const uint32_t b = lab < (uint32_t)A.S.n ? A.rank[lab] : kNoId;
        fold[0] = b < (uint32_t)numBodies ? b : kNoId; // (kNoId: no row of the block matches, nothing is folded)
        fold[1] = 0;
        fold[2] = fold[3] = fold[4] = 0xFFFFFFFFu;
        fold[5] = fold[6] = fold[7] = 0;
    }
    __syncthreads();
    const uint32_t dom = fold[0];
#pragma unroll 1
    for (int k = 0; k < kBodyFold; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        bool valid = i < A.S.n;
        const float4 p = A.S.position(valid ? i : 0);
        const uint32_t id = __float_as_uint(p.w);
        const uint32_t lab = valid ? A.rowLabel[i] : 0u;
        valid = valid && id < (uint32_t)A.S.n && lab < (uint32_t)A.S.n;
        const uint32_t b = valid ? A.rank[lab] : 0u;
        valid = valid && b < (uint32_t)numBodies; // (never false for a state whose ids are a permutation of [0, n))
        if (valid) A.labels[id] = lab;
        const uint32_t kx = order_key(__float_as_uint(p.x)), ky = order_key(__float_as_uint(p.y)), kz = order_key(__float_as_uint(p.z));
        unsigned long long rest = __ballot(valid);
        while (rest) {
            uint32_t b0;
            int lead;
            const unsigned long long grp = next_group(b, valid, rest, b0, lead);
            const bool in = (grp >> lane) & 1;
            uint32_t x0 = kx, y0 = ky, z0 = kz, x1 = kx, y1 = ky, z1 = kz;
            if (__popcll(grp) > 1) {
                x0 = wave_min_u32(in ? kx : 0xFFFFFFFFu), y0 = wave_min_u32(in ? ky : 0xFFFFFFFFu), z0 = wave_min_u32(in ? kz : 0xFFFFFFFFu);
                x1 = wave_max_u32(in ? kx : 0u), y1 = wave_max_u32(in ? ky : 0u), z1 = wave_max_u32(in ? kz : 0u);
            }
            if (lane == lead) {
                if (b0 == dom) body_row_add(fold, (uint32_t)__popcll(grp), x0, y0, z0, x1, y1, z1);
                else body_row_add(A.table + 8 * (size_t)b0, (uint32_t)__popcll(grp), x0, y0, z0, x1, y1, z1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && fold[1] != 0)
        body_row_add(A.table + 8 * (size_t)dom, fold[1], fold[2], fold[3], fold[4], fold[5], fold[6], fold[7]);
}

// keys back to bit patterns; the largest body: greatest count, then smallest label
__global__ __launch_bounds__(256) void k_body_table_finish(BodyArgs A, int numBodies) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    unsigned long long packed = 0;
    if (b < numBodies) {
        uint32_t *t = A.table + 8 * (size_t)b;
#pragma unroll
        for (int k = 2; k < 8; ++k) t[k] = order_bits(t[k]);
        packed = ((unsigned long long)t[1] << 32) | (unsigned long long)(~t[0]);
    }
    packed = wave_max_u64(packed);
    if ((threadIdx.x & 63) == 0 && packed) atomicMax(&A.counters->largest, packed);
}

void launch_mark_and_scan(const BodyArgs &A, bool plain, hipStream_t s) {
    k_body_mark<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A, plain);
    // rank = the exclusive scan of flag, numBodies = its total
    launch_exclusive_scan<uint32_t>(A.flag, A.S.n, A.blockSum, A.rank, &A.counters->numBodies, nullptr, s);
}

} // namespace

int sph_body_scan_blocks(int n) { return scan_blocks(n); }

void sph_launch_bodies_unite(const DevParams &P, const BodyArgs &A, hipStream_t s) {
    if (A.S.n <= 0) return;
    (void)hipMemsetAsync(A.counters, 0, sizeof(BodyCounters), s);
    k_body_clear<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A, false);
    k_body_link<<<blocks_of(A.S.n, 256), 256, 0, s>>>(P, A);
    k_body_flatten<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A);
    k_body_root_id<<<fold_blocks_of(A.S.n), 256, 0, s>>>(A);
    launch_mark_and_scan(A, false, s);
}

void sph_launch_bodies_plain_begin(const BodyArgs &A, hipStream_t s) {
    if (A.S.n <= 0) return;
    (void)hipMemsetAsync(A.counters, 0, sizeof(BodyCounters), s);
    k_body_clear<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A, true);
}

void sph_launch_bodies_plain_round(const DevParams &P, const BodyArgs &A, bool first, hipStream_t s) {
    if (A.S.n <= 0) return;
    (void)hipMemsetAsync(&A.counters->changed, 0, sizeof(uint32_t), s);
    k_body_plain_round<<<blocks_of(A.S.n, 256), 256, 0, s>>>(P, A, first);
}

void sph_launch_bodies_plain_end(const BodyArgs &A, hipStream_t s) {
    if (A.S.n <= 0) return;
    launch_mark_and_scan(A, true, s);
}

void sph_launch_bodies_table(const BodyArgs &A, int numBodies, hipStream_t s) {
    if (A.S.n <= 0 || numBodies <= 0) return;
    k_body_table_init<<<blocks_of(A.S.n, 256), 256, 0, s>>>(A, numBodies);
    k_body_table_fill<<<fold_blocks_of(A.S.n), 256, 0, s>>>(A, numBodies);
    k_body_table_finish<<<blocks_of(numBodies, 256), 256, 0, s>>>(A, numBodies);
}
