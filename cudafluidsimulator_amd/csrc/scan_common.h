// The exclusive scan of n uint32 words in id order that the bodies (T = uint32_t: labels below an id) and the neighbour
// lists (T = unsigned long long: entries before a list) share, three launches: every block's sum of its 2,048 words,
// the offsets of the block sums (one block, which also leaves the total), every word's offset.  Nothing waits for
// anything inside a launch.  (surface.hip scans pairs packed from ballots and sort.hip scans digits on the step's path:
// both keep their own.)
#pragma once

#include "sph_device.h"

constexpr int kScanTile = 2048; // words per block: 256 threads x 8
inline int scan_blocks(int n) { return n > 0 ? blocks_of(n, kScanTile) : 0; }

// exclusive scan of one value per thread over a block of 256; total: the block's sum, in every thread
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T &total) {
    __shared__ T waveSum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) waveSum[w] = incl;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        base += q < w ? waveSum[q] : (T)0;
        total += waveSum[q];
    }
    __syncthreads(); // waveSum may be written again by the next call
    return base + incl - v;
}

// the thread's 8 consecutive words of its block's tile (0 past n) and their sum
template <class T>
__device__ __forceinline__ T scan_slice(const uint32_t *in, int n, uint32_t (&c)[8]) {
    const int first = blockIdx.x * kScanTile + threadIdx.x * 8;
    T sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[k] = first + k < n ? in[first + k] : 0u;
        sum += c[k];
    }
    return sum;
}

template <class T>
__global__ __launch_bounds__(256) void k_scan_sums(const uint32_t *in, int n, T *blockSum) {
    uint32_t c[8];
    T total;
    const T mine = scan_slice<T>(in, n, c);
    (void)block_exclusive_scan(mine, total);
    if (threadIdx.x == 0) blockSum[blockIdx.x] = total;
}

// blockSum[0, blocks) in place, in rounds of 256 with the total so far carried from round to round; the grand total to
// *total and, where given, to *total2
template <class T>
__global__ __launch_bounds__(256) void k_scan_offsets(T *blockSum, int blocks, T *total, T *total2) {
    T carry = 0;
    for (int k = 0; k < blocks; k += 256) { // (uniform trip count: the barriers inside are reached by every thread)
        const int b = k + threadIdx.x;
        const T v = b < blocks ? blockSum[b] : (T)0;
        T sum;
        const T before = block_exclusive_scan(v, sum);
        if (b < blocks) blockSum[b] = carry + before;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (total2) *total2 = carry;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_scan_final(const uint32_t *in, int n, const T *blockSum, T *out) {
    uint32_t c[8];
    T total;
    const T mine = scan_slice<T>(in, n, c);
    T before = blockSum[blockIdx.x] + block_exclusive_scan(mine, total);
    const int first = blockIdx.x * kScanTile + threadIdx.x * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (first + k < n) out[first + k] = before;
        before += c[k];
    }
}

// out[0, n) = the exclusive scan of in[0, n), n > 0; blockSum: scan_blocks(n) words of scratch
template <class T>
inline void launch_exclusive_scan(const uint32_t *in, int n, T *blockSum, T *out, T *total, T *total2, hipStream_t s) {
    const int sb = scan_blocks(n);
    k_scan_sums<T><<<sb, 256, 0, s>>>(in, n, blockSum);
    k_scan_offsets<T><<<1, 256, 0, s>>>(blockSum, sb, total, total2);
    k_scan_final<T><<<sb, 256, 0, s>>>(in, n, blockSum, out);
}
