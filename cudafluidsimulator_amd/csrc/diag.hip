// Run diagnostics: nine exact sums, six pairs of extrema and an optional 256-bin histogram
// of the rows (x, y, z, vx, vy, vz, rho) sph_download_state returns.  Every sum is a sum of signed 64-bit Q32.32
// terms q(t) = floor(t 2^32), accumulated as two integer sums (the low words and the arithmetic high words of the
// terms) that the host joins into one 128-bit value; the extrema are minima and maxima of integer keys.  No
// floating-point value is ever added to another across rows, so the words depend on the set of rows only: not on
// their order, the launch shape or how many slabs reduce them.
//
// The production path reads 32 bytes per row and writes nothing per row: each lane keeps its 18 accumulators, 12
// keys and the saturation count in registers over a grid-stride loop, the wave reduces them with shuffles of the
// 32-bit halves, the four waves of a workgroup meet in LDS, and the workgroup sends at most one integer atomic per
// word.  The check path (SPH_DIAG_PLAIN=1) sends every term of every row straight to global atomics.
#include "row_terms.h"

namespace {

constexpr int kDiagThreads = 256;
constexpr int kDiagWaves = kDiagThreads / SPH_WAVE;
constexpr int kDiagMaxBlocks = 1024; // 4 workgroups per CU: every lane takes ceil(n / 2^18) rows beyond that

// One row: its nine terms and the bit patterns of its six extrema candidates.
struct DiagRow {
    long long q[SPH_DIAG_SUMS];
    uint32_t b[SPH_DIAG_EXTREMA];
};

__device__ __forceinline__ DiagRow diag_row(const float4 p, const float4 v, uint32_t &sat) {
    DiagRow r;
    const uint32_t prsBits = field_bits(v, SPH_FIELD_PRESSURE);
    diag_sum_terms(p, v, prsBits, r.q, sat); // (row_terms.h)
    r.b[SPH_DIAG_EXT_X] = __float_as_uint(p.x);
    r.b[SPH_DIAG_EXT_Y] = __float_as_uint(p.y);
    r.b[SPH_DIAG_EXT_Z] = __float_as_uint(p.z);
    r.b[SPH_DIAG_EXT_SPEED] = field_bits(v, SPH_FIELD_SPEED);
    r.b[SPH_DIAG_EXT_RHO] = __float_as_uint(v.w);
    r.b[SPH_DIAG_EXT_PRS] = prsBits;
    return r;
}

// the whole block: zero sums and bins, the identities of the extrema, the given range of the histogram
__global__ __launch_bounds__(kDiagThreads) void k_diag_clear(DiagBlock *__restrict__ blk, uint32_t loBits, uint32_t hiBits) {
    const int t = threadIdx.x;
    blk->hist[t] = 0ull; // (SPH_DIAG_BINS == kDiagThreads)
    if (t < SPH_DIAG_SUMS) {
        blk->lo[t] = 0ull;
        blk->hi[t] = 0ll;
    }
    if (t < SPH_DIAG_EXTREMA) {
        blk->minKey[t] = 0xFFFFFFFFu;
        blk->maxKey[t] = 0u;
    }
    if (t == 0) {
        blk->saturated = 0ull;
        blk->range[0] = loBits;
        blk->range[1] = hiBits;
        blk->pad[0] = blk->pad[1] = 0u;
    }
}
static_assert(SPH_DIAG_BINS == kDiagThreads, "k_diag_clear and the histogram flush take one bin per thread");

// the check path: one thread per row, every term a global atomic
__global__ __launch_bounds__(kDiagThreads) void k_diag_plain(DiagArgs A, DiagBlock *__restrict__ blk) {
    const long long i = (long long)blockIdx.x * kDiagThreads + threadIdx.x; // (n may come within 256 of 2^31)
    if (i >= A.n) return;
    uint32_t sat = 0u;
    const DiagRow r = diag_row(A.pos[(size_t)i * A.stride], A.vel[(size_t)i * A.stride], sat);
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
        atomicAdd(&blk->lo[k], (unsigned long long)r.q[k] & 0xFFFFFFFFull);
        atomicAdd((unsigned long long *)&blk->hi[k], (unsigned long long)(r.q[k] >> 32));
    }
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
        atomicMin(&blk->minKey[k], order_key(r.b[k]));
        atomicMax(&blk->maxKey[k], order_key(r.b[k]));
    }
    if (sat) atomicAdd(&blk->saturated, (unsigned long long)sat);
}

// the production path
__global__ __launch_bounds__(kDiagThreads) void k_diag_reduce(DiagArgs A, DiagBlock *__restrict__ blk) {
    __shared__ unsigned long long sSum[kDiagWaves][2 * SPH_DIAG_SUMS + 1];
    __shared__ uint32_t sKey[kDiagWaves][2 * SPH_DIAG_EXTREMA];
    unsigned long long lo[SPH_DIAG_SUMS], hi[SPH_DIAG_SUMS];
    uint32_t mn[SPH_DIAG_EXTREMA], mx[SPH_DIAG_EXTREMA];
    uint32_t sat = 0u;
#pragma unroll
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) lo[k] = hi[k] = 0ull;
#pragma unroll
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
        mn[k] = 0xFFFFFFFFu;
        mx[k] = 0u;
    }
    for (long long i = (long long)blockIdx.x * kDiagThreads + threadIdx.x; i < A.n; i += (long long)gridDim.x * kDiagThreads) {
        const DiagRow r = diag_row(A.pos[(size_t)i * A.stride], A.vel[(size_t)i * A.stride], sat);
#pragma unroll
        for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
            lo[k] += (unsigned long long)r.q[k] & 0xFFFFFFFFull;
            hi[k] += (unsigned long long)(r.q[k] >> 32); // (two's complement: the wrap-around sum is the signed one)
        }
#pragma unroll
        for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
            const uint32_t key = order_key(r.b[k]);
            mn[k] = min(mn[k], key);
            mx[k] = max(mx[k], key);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
        lo[k] = wave_sum_u64(lo[k]);
        hi[k] = wave_sum_u64(hi[k]);
    }
    const unsigned long long satw = wave_sum_u32(sat); // (9 terms a row, n < 2^31 rows over >= 2^18 lanes: a wave's count fits)
#pragma unroll
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
        mn[k] = wave_min_u32(mn[k]);
        mx[k] = wave_max_u32(mx[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
            sSum[wave][k] = lo[k];
            sSum[wave][SPH_DIAG_SUMS + k] = hi[k];
        }
        sSum[wave][2 * SPH_DIAG_SUMS] = satw;
#pragma unroll
        for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
            sKey[wave][k] = mn[k];
            sKey[wave][SPH_DIAG_EXTREMA + k] = mx[k];
        }
    }
    __syncthreads();
    // one thread per word: 19 sums, then 12 keys
    const int t = threadIdx.x;
    if (t < 2 * SPH_DIAG_SUMS + 1) {
        unsigned long long s = 0ull;
        for (int w = 0; w < kDiagWaves; ++w) s += sSum[w][t];
        unsigned long long *dst = t < SPH_DIAG_SUMS ? &blk->lo[t]
                                  : t < 2 * SPH_DIAG_SUMS ? (unsigned long long *)&blk->hi[t - SPH_DIAG_SUMS] : &blk->saturated;
        if (s) atomicAdd(dst, s);
    } else if (t < 2 * SPH_DIAG_SUMS + 1 + 2 * SPH_DIAG_EXTREMA) {
        const int k = t - (2 * SPH_DIAG_SUMS + 1);
        if (k < SPH_DIAG_EXTREMA) {
            uint32_t m = 0xFFFFFFFFu;
            for (int w = 0; w < kDiagWaves; ++w) m = min(m, sKey[w][k]);
            atomicMin(&blk->minKey[k], m);
        } else {
            uint32_t m = 0u;
            for (int w = 0; w < kDiagWaves; ++w) m = max(m, sKey[w][k]);
            atomicMax(&blk->maxKey[k - SPH_DIAG_EXTREMA], m);
        }
    }
}

// the extremum pair of a histogram field
__device__ __forceinline__ int diag_ext_of(int field) {
    return field == SPH_FIELD_SPEED ? SPH_DIAG_EXT_SPEED : field == SPH_FIELD_DENSITY ? SPH_DIAG_EXT_RHO : SPH_DIAG_EXT_PRS;
}

// the range of the bins: the given one (k_diag_clear left it in the block) or the reduced extrema of the field
__device__ __forceinline__ void diag_range(const DiagArgs &A, const DiagBlock *blk, float &lo, float &hi) {
    if (A.autoRange) {
        const int e = diag_ext_of(A.histField);
        lo = __uint_as_float(order_bits(blk->minKey[e]));
        hi = __uint_as_float(order_bits(blk->maxKey[e]));
    } else {
        lo = __uint_as_float(blk->range[0]);
        hi = __uint_as_float(blk->range[1]);
    }
}

// the field frame's q of a scalar (render.hip, field_rgb), to the letter
__device__ __forceinline__ uint32_t diag_bin(float s, float lo, float hi) {
    uint32_t q = 0u;
    if (hi != lo) {
        const float u = ((s - lo) / (hi - lo)) * 256.f;
        if (u == u) q = (uint32_t)(int)fminf(fmaxf(floorf(u), 0.f), 255.f); // (NaN: q = 0)
    }
    return q;
}

// automatic range: the bits the bins were cut over, for the host (one thread, behind k_diag_reduce / k_diag_plain)
__global__ void k_diag_publish_range(DiagArgs A, DiagBlock *__restrict__ blk) {
    float lo, hi;
    diag_range(A, blk, lo, hi);
    blk->range[0] = __float_as_uint(lo);
    blk->range[1] = __float_as_uint(hi);
}

__global__ __launch_bounds__(kDiagThreads) void k_diag_hist_plain(DiagArgs A, DiagBlock *__restrict__ blk) {
    const long long i = (long long)blockIdx.x * kDiagThreads + threadIdx.x; // (n may come within 256 of 2^31)
    if (i >= A.n) return;
    float lo, hi;
    diag_range(A, blk, lo, hi);
    const float s = __uint_as_float(field_bits(A.vel[(size_t)i * A.stride], A.histField));
    atomicAdd(&blk->hist[diag_bin(s, lo, hi)], 1ull);
}

// a private histogram per workgroup in LDS (a workgroup's rows are fewer than 2^32: no bin overflows), flushed with
// one 64-bit atomic per non-empty bin
__global__ __launch_bounds__(kDiagThreads) void k_diag_hist(DiagArgs A, DiagBlock *__restrict__ blk) {
    __shared__ uint32_t bins[SPH_DIAG_BINS];
    bins[threadIdx.x] = 0u;
    float lo, hi;
    diag_range(A, blk, lo, hi);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kDiagThreads + threadIdx.x; i < A.n; i += (long long)gridDim.x * kDiagThreads) {
        const float s = __uint_as_float(field_bits(A.vel[(size_t)i * A.stride], A.histField));
        atomicAdd(&bins[diag_bin(s, lo, hi)], 1u);
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(&blk->hist[threadIdx.x], (unsigned long long)c);
}

} // namespace

void sph_launch_diagnose(const DiagArgs &A, bool plain, DiagBlock *blk, hipStream_t s) {
    const bool hist = A.histField >= 0;
    k_diag_clear<<<1, kDiagThreads, 0, s>>>(blk, hist && !A.autoRange ? __builtin_bit_cast(uint32_t, A.lo) : 0u,
                                            hist && !A.autoRange ? __builtin_bit_cast(uint32_t, A.hi) : 0u);
    if (A.n <= 0) return; // no row: the host reports the identities
    const int rowBlocks = (A.n + kDiagThreads - 1) / kDiagThreads;
    const int blocks = rowBlocks < kDiagMaxBlocks ? rowBlocks : kDiagMaxBlocks;
    if (plain) k_diag_plain<<<rowBlocks, kDiagThreads, 0, s>>>(A, blk);
    else k_diag_reduce<<<blocks, kDiagThreads, 0, s>>>(A, blk);
    if (!hist) return;
    // behind the reduction: an automatic range is its result
    if (plain) k_diag_hist_plain<<<rowBlocks, kDiagThreads, 0, s>>>(A, blk);
    else k_diag_hist<<<blocks, kDiagThreads, 0, s>>>(A, blk);
    if (A.autoRange) k_diag_publish_range<<<1, 1, 0, s>>>(A, blk);
}
