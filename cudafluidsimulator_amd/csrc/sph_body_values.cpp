// Per-body moments, the pure host function: sph_body_values derives the doubles of every body
// from its raw row.  Plain C++: no HIP, no handle, no GPU -- built into libsph_hip.so and, on its own under the host
// sanitizers, into the stand-alone check of tests/test_body_moments_cpu.py.
#include "sph_c_api.h"
#include "sph_sum_value.h"

#include <cmath>
#include <cstring>

namespace {

constexpr float kMass = 0.02f; // as the fp32 number the kernels hold (sph_device.h; simulator.h:6-12)

} // namespace

extern "C" int sph_body_values(const SphBodyMomentsRaw *rows, int num_bodies, const SphSettings *settings, SphBodyValues *out) {
    if (num_bodies < 0 || !settings) return SPH_EINVAL;
    if (num_bodies > 0 && (!rows || !out)) return SPH_EINVAL;
    // every expression in the order DESIGN.md section 10k writes it: one rounding per operation
    const double MASS = (double)kMass;
    for (int b = 0; b < num_bodies; ++b) {
        const SphBodyMomentsRaw &r = rows[b];
        SphBodyValues &o = out[b];
        double S[SPH_BODY_SUMS];
        for (int k = 0; k < SPH_BODY_SUMS; ++k) S[k] = sph_sum::sum_value(r.sum[k]);
        memset(&o, 0, sizeof o);
        const double nd = (double)r.count;
        const bool any = r.count != 0; // (a table row always has rows; without any, every quotient is 0)
        o.mass = nd * MASS;
        for (int a = 0; a < 3; ++a) {
            o.com[a] = any ? S[SPH_DIAG_SUM_X + a] / nd : 0.0;
            o.velocity[a] = any ? S[SPH_DIAG_SUM_VX + a] / nd : 0.0;
            o.momentum[a] = MASS * S[SPH_DIAG_SUM_VX + a];
        }
        const double *c = o.com, *v = o.velocity;
        o.kinetic = (0.5 * MASS) * S[SPH_DIAG_SUM_V2];
        o.kinetic_internal = o.kinetic - (0.5 * o.mass) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        o.mean_rho = any ? S[SPH_DIAG_SUM_RHO] / nd : 0.0;
        o.mean_prs = any ? S[SPH_DIAG_SUM_PRS] / nd : 0.0;
        static const int A[6] = {0, 1, 2, 0, 0, 1}, B[6] = {0, 1, 2, 1, 2, 2}; // xx yy zz xy xz yz
        for (int k = 0; k < 6; ++k) o.covariance[k] = (any ? S[SPH_BODY_SUM_XX + k] / nd : 0.0) - c[A[k]] * c[B[k]];
        o.gyration = std::sqrt(std::fmax(0.0, (o.covariance[0] + o.covariance[1]) + o.covariance[2]));
        const double arm[3] = {c[1] * v[2] - c[2] * v[1], c[2] * v[0] - c[0] * v[2], c[0] * v[1] - c[1] * v[0]};
        for (int a = 0; a < 3; ++a) o.angular[a] = MASS * (S[SPH_BODY_SUM_LX + a] - nd * arm[a]);
        o.saturated = r.saturated;
    }
    return SPH_OK;
}
