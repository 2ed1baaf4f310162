// Pair statistics, the pure host functions: sph_pair_edges fills the table of squared bin
// edges a call of sph_pair_statistics uses, sph_pair_values derives the doubles of every bin from its raw row.  Plain
// C++: no HIP, no handle, no GPU -- tests/test_pairs_cpu.py holds both to their Python restatements bit for bit.
#include "sph_c_api.h"
#include "sph_sum_value.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int kDefaultBins = 32;
constexpr double kPi = 3.141592653589793; // (Python's math.pi)

} // namespace

extern "C" int sph_pair_edges(float radius_or_0, float h, int bins, float *edges2) {
    if (!edges2 || bins < 0 || bins > SPH_PAIR_MAX_BINS) return SPH_EINVAL;
    if (!std::isfinite(h) || !(h > 0.f)) return SPH_EINVAL;
    if (!std::isfinite(radius_or_0) || radius_or_0 < 0.f || radius_or_0 > h) return SPH_EINVAL;
    const float radius = radius_or_0 == 0.f ? h : radius_or_0;
    const int B = bins ? bins : kDefaultBins;
    // every expression in the order DESIGN.md section 10m writes it: one rounding per operation
    for (int k = 0; k < B; ++k) {
        const double t = ((double)radius * (double)(k + 1)) / (double)B;
        edges2[k] = (float)(t * t);
    }
    edges2[B - 1] = radius * radius; // r2 itself, the word the link test compares with
    return SPH_OK;
}

extern "C" int sph_pair_values(const SphPairBinRaw *rows, const float *edges2, int bins, const SphSettings *settings, int64_t n,
                               SphPairValues *out) {
    if (!rows || !edges2 || !settings || !out || bins < 1 || bins > SPH_PAIR_MAX_BINS || n < 0) return SPH_EINVAL;
    for (int k = 0; k < bins; ++k)
        if (edges2[k] != edges2[k] || (k > 0 && edges2[k] < edges2[k - 1])) return SPH_EINVAL;
    const double nd = (double)n;
    const double couples = (nd * (nd - 1.0)) / 2.0;
    const double box = (double)settings->boxDim;
    const double volume = (box * box) * box;
    for (int k = 0; k < bins; ++k) {
        const SphPairBinRaw &r = rows[k];
        SphPairValues &o = out[k];
        memset(&o, 0, sizeof o);
        o.r_lo = k ? std::sqrt((double)edges2[k - 1]) : 0.0;
        o.r_hi = std::sqrt((double)edges2[k]);
        o.pairs = (double)r.pairs;
        const bool any = r.pairs != 0;
        o.mean_r2 = any ? sph_sum::sum_value(r.sums[SPH_PAIR_SUM_D2]) / o.pairs : 0.0;
        o.s2 = any ? sph_sum::sum_value(r.sums[SPH_PAIR_SUM_W2]) / o.pairs : 0.0;
        o.s2_par = any ? sph_sum::sum_value(r.sums[SPH_PAIR_SUM_L2]) / o.pairs : 0.0;
        o.approach = any ? sph_sum::sum_value(r.sums[SPH_PAIR_SUM_A]) / o.pairs : 0.0;
        const double shell = ((4.0 * kPi) / 3.0) * ((o.r_hi * o.r_hi) * o.r_hi - (o.r_lo * o.r_lo) * o.r_lo);
        const double ideal = (couples * shell) / volume;
        o.g = ideal > 0.0 ? o.pairs / ideal : 0.0;
        o.saturated = r.saturated;
    }
    return SPH_OK;
}
