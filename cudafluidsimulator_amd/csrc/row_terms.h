// The Q32.32 terms of a row (DESIGN.md sections 10c, 10k): what the diagnostics (diag.hip) sum over the whole fluid and
// the bodies' moments (body_moments.hip) sum per body.  One copy, so the two cannot drift apart.  Device code only.
#pragma once

#include "sph_c_api.h"
#include "sph_device.h"

// q(t): NaN -> 0, t >= 2^31 -> INT64_MAX, t < -2^31 -> INT64_MIN (each counted in sat), else (int64)floor(t 2^32).
// The scaling is exact, and the floor of a double below 2^63 in magnitude converts exactly.
__device__ __forceinline__ long long diag_q(double t, uint32_t &sat) {
    if (t != t) {
        sat += 1u;
        return 0ll;
    }
    if (t >= 2147483648.0) {
        sat += 1u;
        return 0x7FFFFFFFFFFFFFFFll;
    }
    if (t < -2147483648.0) {
        sat += 1u;
        return (long long)0x8000000000000000ull;
    }
    return (long long)floor(t * 4294967296.0);
}

// The nine terms SPH_DIAG_SUM_* of the row (p, v) into q[0, 9); prsBits = field_bits(v, SPH_FIELD_PRESSURE).
__device__ __forceinline__ void diag_sum_terms(const float4 p, const float4 v, uint32_t prsBits, long long *q, uint32_t &sat) {
    q[SPH_DIAG_SUM_X] = diag_q((double)p.x, sat);
    q[SPH_DIAG_SUM_Y] = diag_q((double)p.y, sat);
    q[SPH_DIAG_SUM_Z] = diag_q((double)p.z, sat);
    q[SPH_DIAG_SUM_VX] = diag_q((double)v.x, sat);
    q[SPH_DIAG_SUM_VY] = diag_q((double)v.y, sat);
    q[SPH_DIAG_SUM_VZ] = diag_q((double)v.z, sat);
    q[SPH_DIAG_SUM_RHO] = diag_q((double)v.w, sat);
    q[SPH_DIAG_SUM_PRS] = diag_q((double)__uint_as_float(prsBits), sat);
    // (the three products are exact in fp64 -- 24 x 24 significant bits -- so a fused multiply-add would round the
    // same two sums)
    const double vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
    q[SPH_DIAG_SUM_V2] = diag_q((vx * vx + vy * vy) + vz * vz, sat);
}
