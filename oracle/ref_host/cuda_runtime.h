/*
 * cuda_runtime.h -- a host stand-in for the CUDA runtime.  TEST INFRASTRUCTURE ONLY.
 *
 * With this header the reference's simulator.cu compiles as plain C++ and its kernels run
 * serially on the CPU (oracle/Makefile, target ref; oracle/reference.py).
 * It supplies what that file names and nothing else: the vector types, empty function-space
 * qualifiers, the four built-in index variables as globals (defined by reference_driver.cpp),
 * a dozen runtime calls over malloc / memcpy, a serial atomicCAS, and the launcher behind the
 * REF_LAUNCH macro that the build recipe puts in place of the <<< >>> launch syntax.
 *
 * Execution order.  ref_launch() runs every (block, thread) of a launch in ascending order,
 * one after the other, except the kernel named kernelBuildGrid: its threads push onto per-cell
 * lists by head insertion, so the order in which they run IS the order of every list, and any
 * order is an admissible execution of the racing original.  That kernel runs in the schedule
 * the driver supplies (ref_build_schedule: linear thread indices, first to run first; threads
 * it does not name run before it), or in descending thread index without one.
 */
#ifndef SPH_REF_HOST_CUDA_RUNTIME_H
#define SPH_REF_HOST_CUDA_RUNTIME_H

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __global__
#define __device__
#define __constant__
#define __host__

struct float3 { float x, y, z; };
struct int3 { int x, y, z; };
struct int2 { int x, y; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }

/* the built-in index variables: globals, written by ref_launch() only */
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

/* the schedule of kernelBuildGrid's threads (see above); null: descending thread index */
extern const int *ref_build_schedule;
extern long ref_build_schedule_len;

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

template <class T> static inline cudaError_t cudaMalloc(T **p, size_t bytes) {
    *p = static_cast<T *>(std::malloc(bytes ? bytes : 1));
    return *p ? cudaSuccess : 2;
}
static inline cudaError_t cudaMemset(void *p, int v, size_t bytes) { std::memset(p, v, bytes); return cudaSuccess; }
static inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t bytes, cudaMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return cudaSuccess;
}
template <class T> static inline cudaError_t cudaMemcpyToSymbol(T &symbol, const void *src, size_t bytes) {
    std::memcpy(&symbol, src, bytes);
    return cudaSuccess;
}
/* A no-op on purpose: the reference's destructor hands cudaFree() list nodes that live INSIDE
 * the particle block, which free() must never see. */
static inline cudaError_t cudaFree(void *) { return cudaSuccess; }
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }

/* one thread at a time: compare-and-swap without contention */
static inline unsigned long long atomicCAS(unsigned long long *address, unsigned long long compare,
                                           unsigned long long val) {
    unsigned long long old = *address;
    if (old == compare) *address = val;
    return old;
}

template <class Body> static inline void ref_run_thread(unsigned long linear, const dim3 &block, Body &body) {
    /* a 1-D launch: linear = blockIdx.x * blockDim.x + threadIdx.x */
    blockIdx = uint3{static_cast<unsigned>(linear / block.x), 0u, 0u};
    threadIdx = uint3{static_cast<unsigned>(linear % block.x), 0u, 0u};
    body();
}

/* A function, not a macro body: the caller has locals named gridDim and blockDim that hide the
 * globals at the call site. */
template <class Body> static inline void ref_launch(const char *name, dim3 grid, dim3 block, Body body) {
    ::gridDim = grid;
    ::blockDim = block;
    if (std::strcmp(name, "kernelBuildGrid") == 0) {
        if (grid.y != 1 || grid.z != 1 || block.y != 1 || block.z != 1) {
            std::fprintf(stderr, "ref_launch: %s is expected as a 1-D launch\n", name);
            std::abort();
        }
        const long total = static_cast<long>(grid.x) * block.x;
        const long listed = ref_build_schedule ? ref_build_schedule_len : 0;
        for (long t = total - 1; t >= listed; --t) ref_run_thread(static_cast<unsigned long>(t), block, body);
        for (long i = 0; i < listed; ++i) ref_run_thread(static_cast<unsigned long>(ref_build_schedule[i]), block, body);
        return;
    }
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx)
                for (unsigned tz = 0; tz < block.z; ++tz)
                    for (unsigned ty = 0; ty < block.y; ++ty)
                        for (unsigned tx = 0; tx < block.x; ++tx) {
                            blockIdx = uint3{bx, by, bz};
                            threadIdx = uint3{tx, ty, tz};
                            body();
                        }
}

/* kernel<<<grid, block>>>(args...)  ->  REF_LAUNCH(kernel, grid, block, args...)  (the build recipe's sed) */
#define REF_LAUNCH(kernel, grid, block, ...) \
    ref_launch(#kernel, dim3(grid), dim3(block), [&]() { kernel(__VA_ARGS__); })

#endif
