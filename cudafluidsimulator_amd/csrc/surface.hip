// The surface mesh: marching tetrahedra over the density sample of a lattice.  Three
// launches behind two launchers: classify + count + scan within a block, the scan across the blocks' sums (one
// small block that walks them in order: no look-back, nothing spins), and, once the host has sized the output
// from the two totals, emit.  Vertex arithmetic is fp32, every operation rounded on its own (-ffp-contract=off).
//
// Both paths give a thread one lattice point and a wave 64 consecutive L, so one scan serves both.  The production
// path reads a wave's eight corners as four coalesced runs -- L, L + nx, L + nx ny, L + nx ny + nx -- and takes the
// +x corner from the next lane; only lane 63 reads its +x neighbours itself.  That holds for each of the three
// arrays a pass reads (the field, the corner bytes, the offsets), and emit reads nothing but one byte per point
// for a wave that no part of the surface crosses.  (One wave per 64 ix of a lattice row, k_sample_tile's layout,
// was measured first: at nx = 101 and 201 it leaves a fifth of the lanes without a point and lost to the check
// path)  The check path (SPH_SURFACE_PLAIN=1): every corner a global load.
#include "sph_device.h"
#include "surface_tables.h"

namespace {

namespace st = surface_tables;

__constant__ st::Tables kTab = st::kTables;

constexpr int kCountBlock = 1024, kCountWaves = kCountBlock / 64; // points per block of the counting launch
constexpr int kEmitBlock = 256;

struct Point {
    int ix, iy, iz;
    uint32_t L;
    bool valid; // the thread has a lattice point
};

__device__ __forceinline__ Point point_of(const SurfaceArgs &A, uint32_t g) {
    Point p;
    p.valid = g < (uint32_t)(A.nx * A.ny * A.nz);
    p.L = g;
    const int r = g / A.nx;
    p.ix = g % A.nx, p.iy = r % A.ny, p.iz = r / A.ny;
    return p;
}

// a[.] at the eight corners of the point's cell, corner k = dx + 2 dy + 4 dz; 0 for a corner off the lattice
template <class Load>
__device__ __forceinline__ void corners_plain(Load ld, const SurfaceArgs &A, const Point &p, uint32_t v[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int x = p.ix + (k & 1), y = p.iy + (k >> 1 & 1), z = p.iz + (k >> 2);
        v[k] = p.valid && x < A.nx && y < A.ny && z < A.nz ? ld(((size_t)z * A.ny + y) * A.nx + x) : 0u;
    }
}
// the same for a wave of consecutive L (every lane calls it): the lane above holds this lane's +x corner unless
// this lane ends its row, where that corner is off the lattice
template <class Load>
__device__ __forceinline__ void corners_wave(Load ld, const SurfaceArgs &A, const Point &p, uint32_t v[8]) {
    const int lane = threadIdx.x & 63;
    const bool more = p.ix + 1 < A.nx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = p.iy + (r & 1), z = p.iz + (r >> 1);
        const bool row = p.valid && y < A.ny && z < A.nz;
        const size_t at = ((size_t)z * A.ny + y) * A.nx + p.ix;
        const uint32_t own = row ? ld(at) : 0u;
        uint32_t next = __shfl_down(own, 1);
        if (lane == 63) next = row && more ? ld(at + 1) : 0u;
        v[2 * r] = own, v[2 * r + 1] = row && more ? next : 0u;
    }
}

// the corners of the cell of (x, y, z) that lie in the lattice
__device__ __forceinline__ uint32_t valid_corners(const SurfaceArgs &A, int x, int y, int z) {
    uint32_t v = 0xFFu;
    if (x + 1 >= A.nx) v &= 0x55u;
    if (y + 1 >= A.ny) v &= 0x33u;
    if (z + 1 >= A.nz) v &= 0x0Fu;
    return v;
}
// the corners that differ from corner 0, of those in the lattice
__device__ __forceinline__ uint32_t crossed_corners(uint32_t byte, uint32_t vc) { return (byte ^ (byte & 1u ? 0xFFu : 0u)) & vc; }
// ... as the mask of crossed edges by direction d: corners 1 2 4 3 5 6 7
static_assert(st::kDirCorner[0] == 1 && st::kDirCorner[1] == 2 && st::kDirCorner[2] == 4 && st::kDirCorner[3] == 3 &&
              st::kDirCorner[4] == 5 && st::kDirCorner[5] == 6 && st::kDirCorner[6] == 7, "edge_mask spells this order out");
__device__ __forceinline__ uint32_t edge_mask(uint32_t byte, uint32_t vc) {
    const uint32_t x = crossed_corners(byte, vc);
    return (x >> 1 & 3u) | (x >> 4 & 1u) << 2 | (x >> 3 & 1u) << 3 | (x >> 5 & 7u) << 4;
}

template <bool kPlain>
__global__ __launch_bounds__(kCountBlock) void k_surface_count(SurfaceArgs A, SurfaceBuffers B) {
    __shared__ uint32_t waveSum[kCountWaves];
    const Point p = point_of(A, blockIdx.x * kCountBlock + threadIdx.x);
    const auto field = [&](size_t i) { return __float_as_uint(B.field[i]); };
    uint32_t f[8];
    if (kPlain) corners_plain(field, A, p, f);
    else corners_wave(field, A, p, f);
    const uint32_t vc = p.valid ? valid_corners(A, p.ix, p.iy, p.iz) : 0u;
    uint32_t byte = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((vc >> k & 1u) && __uint_as_float(f[k]) >= A.iso) byte |= 1u << k; // (a NaN is outside)
    const uint32_t nv = __popc(edge_mask(byte, vc));             // <= 7
    const uint32_t nt = vc == 0xFFu ? kTab.cellTris[byte] : 0u;  // <= 12; only a point with all eight corners anchors a cell
    // Exclusive scan of both counts over the wave: one ballot per bit of (nv, nt), the lanes below counted.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t x = nv | nt << 3;
    uint32_t pre = 0, sum = 0; // vertices in the low half, triangles in the high half (a block: <= 7168 and <= 12288)
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const unsigned long long m = __ballot(x >> b & 1u);
        const int sh = b < 3 ? b : b - 3 + 16;
        pre += (uint32_t)__popcll(m & below) << sh;
        sum += (uint32_t)__popcll(m) << sh;
    }
    if (lane == 0) waveSum[wave] = sum;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCountWaves; ++w) {
        before += w < wave ? waveSum[w] : 0u;
        all += waveSum[w];
    }
    if (p.valid) B.bits[p.L] = (uint8_t)byte;
    // (emit reads the offsets of a point only where it owns a vertex -- a cell with a triangle has a corner that
    // differs from corner 0, so its anchor does: the other words of `local` are never written and mean nothing)
    if (nv > 0) B.local[p.L] = before + pre;
    if (threadIdx.x == 0) B.blockSum[blockIdx.x] = make_uint2(all & 0xFFFFu, all >> 16);
}

// exclusive scan of the blocks' sums, in order, by one block: rounds of 1024 threads x kScanItems consecutive sums;
// the two totals (< 2^27 and < 2^28 for 2^24 points)
constexpr int kScanItems = 2;
__global__ __launch_bounds__(1024) void k_surface_scan(const uint2 *__restrict__ sums, uint2 *__restrict__ offs, int blocks,
                                                        unsigned long long *__restrict__ totals) {
    __shared__ uint2 waveSum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint2 carry = make_uint2(0u, 0u);
    for (int base = 0; base < blocks; base += 1024 * kScanItems) {
        const int first = base + threadIdx.x * kScanItems;
        uint2 v[kScanItems];
        uint2 mine = make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            v[k] = first + k < blocks ? sums[first + k] : make_uint2(0u, 0u);
            mine.x += v[k].x, mine.y += v[k].y;
        }
        uint2 inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t a = __shfl_up(inc.x, off), b = __shfl_up(inc.y, off);
            if (lane >= off) inc.x += a, inc.y += b;
        }
        if (lane == 63) waveSum[wave] = inc;
        __syncthreads();
        uint2 before = carry;
        for (int w = 0; w < 16; ++w) {
            const uint2 s = waveSum[w];
            if (w < wave) before.x += s.x, before.y += s.y;
            carry.x += s.x, carry.y += s.y;
        }
        before.x += inc.x - mine.x, before.y += inc.y - mine.y;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            if (first + k < blocks) offs[first + k] = before;
            before.x += v[k].x, before.y += v[k].y;
        }
        __syncthreads(); // waveSum is rewritten by the next round
    }
    if (threadIdx.x == 0) totals[0] = carry.x, totals[1] = carry.y;
}

template <bool kPlain>
__global__ __launch_bounds__(kEmitBlock) void k_surface_emit(SurfaceArgs A, SurfaceBuffers B, float *__restrict__ verts,
                                                             uint32_t *__restrict__ tris) {
    // production path: first vertex and edge mask of the seven corners that can own an edge of this thread's cell
    __shared__ uint32_t cornerOff[kPlain ? 1 : 7][kEmitBlock], cornerMask[kPlain ? 1 : 7][kEmitBlock];
    const Point p = point_of(A, blockIdx.x * kEmitBlock + threadIdx.x);
    const uint32_t vc = p.valid ? valid_corners(A, p.ix, p.iy, p.iz) : 0u;
    const uint32_t own = p.valid ? B.bits[p.L] : 0u;
    const bool crossed = crossed_corners(own, vc) != 0; // else: no vertex on the point's edges, no triangle in its cell
    if (kPlain ? !crossed : __ballot(crossed) == 0ull) return;
    const auto field = [&](size_t i) { return __float_as_uint(B.field[i]); };
    const auto bits = [&](size_t i) { return (uint32_t)B.bits[i]; };
    const auto local = [&](size_t i) { return B.local[i]; };
    uint32_t f[8], cb[8], cl[8];
    if (kPlain) {
        corners_plain(field, A, p, f);
    } else {
        corners_wave(field, A, p, f);
        corners_wave(bits, A, p, cb);
        corners_wave(local, A, p, cl);
    }
    if (!crossed) return;
    const uint2 blockOff = B.blockOff[p.L / kCountBlock];
    const uint32_t loc = B.local[p.L];
    const uint32_t voff = blockOff.x + (loc & 0xFFFFu), toff = blockOff.y + (loc >> 16);

    // the vertices of the edges this point owns, by d ascending
    const uint32_t m = edge_mask(own, vc);
    const float fa = __uint_as_float(f[0]);
    const float pa[3] = {A.ox + (float)p.ix * A.sx, A.oy + (float)p.iy * A.sy, A.oz + (float)p.iz * A.sz};
    const float pb[3] = {A.ox + (float)(p.ix + 1) * A.sx, A.oy + (float)(p.iy + 1) * A.sy, A.oz + (float)(p.iz + 1) * A.sz};
    uint32_t v = voff;
#pragma unroll
    for (int d = 0; d < st::kDirs; ++d) {
        if (!(m >> d & 1u)) continue;
        constexpr int corner[st::kDirs] = {1, 2, 4, 3, 5, 6, 7};
        const int c = corner[d];
        const float t = (A.iso - fa) / (__uint_as_float(f[c]) - fa);
#pragma unroll
        for (int k = 0; k < 3; ++k) verts[(size_t)v * 3 + k] = pa[k] + t * ((c >> k & 1 ? pb[k] : pa[k]) - pa[k]);
        v += 1;
    }

    if (vc != 0xFFu) return; // no cell is anchored here
    if (!kPlain) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const int x = p.ix + (c & 1), y = p.iy + (c >> 1 & 1), z = p.iz + (c >> 2);
            const uint32_t q = ((uint32_t)z * A.ny + y) * A.nx + x;
            cornerOff[c][threadIdx.x] = B.blockOff[q / kCountBlock].x + (cl[c] & 0xFFFFu);
            cornerMask[c][threadIdx.x] = edge_mask(cb[c], valid_corners(A, x, y, z));
        }
    }
    // the vertex on the edge that leaves corner c of this cell in direction d
    const auto vertex = [&](int c, int d) -> uint32_t {
        uint32_t first, mask;
        if (kPlain) {
            const int x = p.ix + (c & 1), y = p.iy + (c >> 1 & 1), z = p.iz + (c >> 2);
            const size_t q = ((size_t)z * A.ny + y) * A.nx + x;
            first = B.blockOff[q / kCountBlock].x + (B.local[q] & 0xFFFFu);
            mask = edge_mask(B.bits[q], valid_corners(A, x, y, z));
        } else {
            first = cornerOff[c][threadIdx.x], mask = cornerMask[c][threadIdx.x];
        }
        return first + __popc(mask & ((1u << d) - 1u));
    };
    uint32_t tri = toff;
    for (int s = 0; s < st::kTets; ++s) {
        uint32_t cs = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) cs |= (own >> kTab.path[s][k] & 1u) << k;
        const st::Entry &E = kTab.tet[s][cs];
        for (int t = 0; t < E.ntri; ++t, ++tri)
            for (int k = 0; k < 3; ++k) tris[(size_t)tri * 3 + k] = vertex(E.ref[3 * t + k] >> 3, E.ref[3 * t + k] & 7);
    }
}

} // namespace

int sph_surface_blocks(const SurfaceArgs &A) { return (A.nx * A.ny * A.nz + kCountBlock - 1) / kCountBlock; }

void sph_launch_surface_count(const SurfaceArgs &A, bool plain, const SurfaceBuffers &B, hipStream_t s) {
    const int blocks = sph_surface_blocks(A);
    if (plain) k_surface_count<true><<<blocks, kCountBlock, 0, s>>>(A, B);
    else k_surface_count<false><<<blocks, kCountBlock, 0, s>>>(A, B);
    k_surface_scan<<<1, 1024, 0, s>>>(B.blockSum, B.blockOff, blocks, B.totals);
}

void sph_launch_surface_emit(const SurfaceArgs &A, bool plain, const SurfaceBuffers &B, float *verts, uint32_t *tris, hipStream_t s) {
    const int blocks = (A.nx * A.ny * A.nz + kEmitBlock - 1) / kEmitBlock;
    if (plain) k_surface_emit<true><<<blocks, kEmitBlock, 0, s>>>(A, B, verts, tris);
    else k_surface_emit<false><<<blocks, kEmitBlock, 0, s>>>(A, B, verts, tris);
}
