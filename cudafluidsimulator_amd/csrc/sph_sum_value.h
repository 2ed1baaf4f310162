// value(S) of an SphSum128: what the pure host functions of the diagnostics
// (sph_diag_values.cpp) and of the bodies' moments (sph_body_values.cpp) derive their doubles from.  Plain C++.
#pragma once

#include "sph_c_api.h"

#include <cmath>

namespace sph_sum {

typedef unsigned __int128 u128;

inline u128 words(const SphSum128 &s) { return ((u128)(uint64_t)s.hi << 64) | s.lo; }

// value(S) = (double)S 2^-32, the conversion of the 128-bit integer rounded correctly to nearest-even (what Python's
// int / 2**32 gives).  Done by hand: the magnitude's top 53 bits, the rest as round and sticky.
inline double sum_value(const SphSum128 &s) {
    const bool neg = s.hi < 0;
    u128 u = words(s);
    if (neg) u = ~u + 1; // the magnitude (2^127 is its own magnitude as an unsigned word)
    if (u == 0) return 0.0;
    int top = 127;
    while (!((u >> top) & 1)) --top;
    double d;
    if (top <= 52) {
        d = (double)(uint64_t)u;
    } else {
        const int shift = top - 52;
        uint64_t m = (uint64_t)(u >> shift); // 53 bits
        const u128 rest = u & (((u128)1 << shift) - 1), half = (u128)1 << (shift - 1);
        if (rest > half || (rest == half && (m & 1))) ++m; // (2^53 is still a double)
        d = std::ldexp((double)m, shift);
    }
    d = std::ldexp(d, -32); // exact: the smallest magnitude is 2^-32
    return neg ? -d : d;
}

} // namespace sph_sum
