// What the launches that reduce rows onto bodies share (bodies.hip: the roots' ids and the table; body_moments.hip:
// the moments; body_tracks.hip: the partial edges): the split of a wave's rows into groups of equal body and the shape of a folding block.  DESIGN.md
// sections 10g, 10k.  Device code only.
#pragma once

#include "sph_device.h"

constexpr uint32_t kNoId = 0xFFFFFFFFu;

// The lanes of a wave that hold the same key as its first lane still in `rest`, taken out of `rest`: a wave's rows are
// neighbours in the stream, so they fall into a few groups, and each group makes one set of atomics instead of one per
// row (a body of millions of rows would otherwise put them all on one address).  Wave-uniform.
__device__ __forceinline__ unsigned long long next_group(uint32_t key, bool valid, unsigned long long &rest, uint32_t &key0, int &lead) {
    lead = __ffsll((long long)rest) - 1;
    key0 = (uint32_t)__shfl((int)key, lead);
    const unsigned long long grp = __ballot(valid && key == key0) & rest;
    rest &= ~grp;
    return grp;
}

// The same for a key of two words (body_tracks.hip: a row's previous and current body).
__device__ __forceinline__ unsigned long long next_group(uint32_t keyA, uint32_t keyB, bool valid, unsigned long long &rest, uint32_t &a0,
                                                         uint32_t &b0, int &lead) {
    lead = __ffsll((long long)rest) - 1;
    a0 = (uint32_t)__shfl((int)keyA, lead);
    b0 = (uint32_t)__shfl((int)keyB, lead);
    const unsigned long long grp = __ballot(valid && keyA == a0 && keyB == b0) & rest;
    rest &= ~grp;
    return grp;
}

// Launches that reduce rows onto bodies give a block kBodyFold x 256 consecutive rows and a few words of LDS for the
// body (or root) of its first row: groups of that body are folded there and leave the block as one set of global
// atomics, groups of any other body go to global memory directly.  A body of millions of rows then costs a set per
// 2,048 rows instead of one per wave -- the atomics of one address are served one after the other.
constexpr int kBodyFold = 8;

inline int fold_blocks_of(int n) { return blocks_of(n, 256 * kBodyFold); }
