// Diagnostics, the two pure host functions: sph_diagnostics_add merges the words of two
// sets of rows, sph_diagnostics_values derives the doubles.  Plain C++: no HIP, no handle, no GPU -- built into
// libsph_hip.so and, on its own under the host sanitizers, into the stand-alone check of tests/test_diagnostics_cpu.py.
#include "sph_c_api.h"
#include "sph_sum_value.h"

#include <cmath>
#include <cstring>

namespace {

// the physics constants these values use, as the fp32 numbers the kernels hold (sph_device.h; simulator.h:6-12)
constexpr float kMass = 0.02f;
constexpr float kMinusGravity = 9.8f;

using sph_sum::u128;
using sph_sum::sum_value;
using sph_sum::words;

uint32_t key_of(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

double as_double(uint32_t bits) {
    float f;
    memcpy(&f, &bits, sizeof f);
    return (double)f;
}

} // namespace

extern "C" {

int sph_diagnostics_add(SphDiagnosticsRaw *into, const SphDiagnosticsRaw *part) {
    if (!into || !part) return SPH_EINVAL;
    if (into->struct_size != (int32_t)sizeof *into || part->struct_size != (int32_t)sizeof *part) return SPH_EINVAL;
    if (into->n < 0 || part->n < 0) return SPH_EINVAL;
    if (into->hist_field != part->hist_field || into->hist_lo_bits != part->hist_lo_bits ||
        into->hist_hi_bits != part->hist_hi_bits)
        return SPH_EINVAL;
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
        const u128 s = words(into->sum[k]) + words(part->sum[k]); // (two's complement: the wrap-around sum is the signed one)
        into->sum[k].lo = (uint64_t)s;
        into->sum[k].hi = (int64_t)(uint64_t)(s >> 64);
    }
    if (part->n > 0) // (a part without rows holds the identities, not candidates)
        for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
            if (into->n == 0 || key_of(part->min_bits[k]) < key_of(into->min_bits[k])) into->min_bits[k] = part->min_bits[k];
            if (into->n == 0 || key_of(part->max_bits[k]) > key_of(into->max_bits[k])) into->max_bits[k] = part->max_bits[k];
        }
    into->n += part->n;
    into->saturated += part->saturated;
    for (int k = 0; k < SPH_DIAG_BINS; ++k) into->hist[k] += part->hist[k];
    return SPH_OK;
}

int sph_diagnostics_values(const SphDiagnosticsRaw *raw, const SphSettings *settings, SphDiagnostics *out) {
    if (!raw || !settings || !out) return SPH_EINVAL;
    if (raw->struct_size != (int32_t)sizeof *raw || raw->n < 0) return SPH_EINVAL;
    // every expression in the order DESIGN.md section 10c writes it: one rounding per operation
    const double MASS = (double)kMass, G = (double)kMinusGravity;
    const double n = (double)raw->n;
    double v[SPH_DIAG_SUMS];
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) v[k] = sum_value(raw->sum[k]);
    memset(out, 0, sizeof *out);
    out->struct_size = (int32_t)sizeof *out;
    out->n = raw->n;
    out->mass = n * MASS;
    for (int k = 0; k < 3; ++k) {
        out->com[k] = raw->n ? v[SPH_DIAG_SUM_X + k] / n : 0.0;
        out->momentum[k] = MASS * v[SPH_DIAG_SUM_VX + k];
        out->box_min[k] = as_double(raw->min_bits[SPH_DIAG_EXT_X + k]);
        out->box_max[k] = as_double(raw->max_bits[SPH_DIAG_EXT_X + k]);
    }
    out->kinetic = (0.5 * MASS) * v[SPH_DIAG_SUM_V2];
    out->potential = (MASS * G) * v[SPH_DIAG_SUM_Y];
    out->mean_rho = raw->n ? v[SPH_DIAG_SUM_RHO] / n : 0.0;
    out->mean_prs = raw->n ? v[SPH_DIAG_SUM_PRS] / n : 0.0;
    out->min_rho = as_double(raw->min_bits[SPH_DIAG_EXT_RHO]);
    out->max_rho = as_double(raw->max_bits[SPH_DIAG_EXT_RHO]);
    out->max_speed = as_double(raw->max_bits[SPH_DIAG_EXT_SPEED]);
    out->cfl = (out->max_speed * (double)settings->timestep) / (double)settings->h;
    out->saturated = raw->saturated;
    return SPH_OK;
}

} // extern "C"
