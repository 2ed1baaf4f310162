// Passive tracers: sph_tracers_set / sph_tracers_advect and what reads their results (kernels: tracers.hip).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

constexpr int kMaxTracers = 1 << 24;

// (re)allocate the tracer buffers for m tracers; nothing may be in flight (sph_tracers_set has waited)
int tracer_reserve(sph_handle *h, size_t m) {
    if (m <= h->tracerCap) return SPH_OK;
    h->tracerCap = 0;
    HIPCHK(h, h->tracerPosDen.alloc(m));
    HIPCHK(h, h->tracerVel.alloc(m));
    HIPCHK(h, h->tracerPosDenHost.alloc(m));
    HIPCHK(h, h->tracerVelHost.alloc(m));
    h->tracerCap = m;
    return SPH_OK;
}

// the tracers' own sort workspace (the grid's still serves sph_download_grid), sized for the buffers' capacity
int tracer_sort_reserve(sph_handle *h) {
    if ((size_t)h->tracerWs.capacity >= h->tracerCap) return SPH_OK;
    HIPCHK(h, hipStreamSynchronize(h->compute)); // an earlier advect may still sort in the old one
    h->tracerWs = SortWorkspace{};
    const size_t nb = sph_sort_workspace_blocks((int)h->tracerCap);
    for (int b = 0; b < 2; ++b) {
        HIPCHK(h, h->tracerKeys[b].alloc(h->tracerCap));
        HIPCHK(h, h->tracerVals[b].alloc(h->tracerCap));
    }
    HIPCHK(h, h->tracerBlockHist.alloc(1024 * nb));
    HIPCHK(h, h->tracerDigitTotal.alloc(1024));
    SortWorkspace ws{};
    for (int b = 0; b < 2; ++b) ws.keys[b] = h->tracerKeys[b], ws.vals[b] = h->tracerVals[b];
    ws.blockHist = h->tracerBlockHist;
    ws.digitTotal = h->tracerDigitTotal;
    ws.capacity = (int)h->tracerCap;
    ws.maxBlocks = (int)nb;
    h->tracerWs = ws;
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_tracers_set(sph_handle *h, const float *pos_xyz, int m) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU runs carry no tracers");
    if (m < 0 || m > kMaxTracers) return fail(h, SPH_EINVAL, "the number of tracers must be 0..1 << 24");
    if (!pos_xyz && m > 0) return fail(h, SPH_EINVAL, "null argument");
    // the last advect may still write the device buffers, its copy the pinned ones
    int rc = pass_quiesce(h, h->tracer);
    if (rc) return rc;
    h->tracerCount = 0;
    if ((rc = tracer_reserve(h, (size_t)m))) return rc;
    if (m > 0) {
        float4 *pd = h->tracerPosDenHost, *u = h->tracerVelHost;
        for (int i = 0; i < m; ++i) {
            // (member-wise: the words travel as they are, a NaN keeps its payload)
            memcpy(&pd[i], pos_xyz + 3 * (size_t)i, 3 * sizeof(float));
            pd[i].w = 0.f;
            u[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        HIPCHK(h, hipMemcpyAsync(h->tracerPosDen, pd, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, h->compute));
        HIPCHK(h, hipStreamSynchronize(h->compute));
    }
    h->tracerCount = m;
    return SPH_OK;
}

int sph_tracers_advect(sph_handle *h, float dt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the tracers' advect", ": multi-GPU runs carry no tracers");
    if (rc) return rc;
    if (!std::isfinite(dt)) return fail(h, SPH_EINVAL, "dt must be finite");
    const int m = h->tracerCount;
    if (m == 0) return SPH_OK;
    if ((rc = analysis_grid(h))) return rc;
    const bool plain = plain_path("SPH_TRACER_PLAIN");
    if (!plain && h->n > 0) {
        if ((rc = tracer_sort_reserve(h))) return rc;
        if ((rc = h->tracerCounters.ensure(h))) return rc;
    }
    if ((rc = outbound_fence(h, h->tracer.out))) return rc; // the previous advect's copy still reads the device buffers
    TracerArgs A{};
    A.S = sorted_stream(h);
    A.m = m;
    A.dt = dt;
    A.posDen = h->tracerPosDen;
    A.velOut = h->tracerVel;
    A.counters = h->tracerCounters.dev;
    // keys up to numCells itself (a tracer outside the grid)
    int bits = 1;
    while ((1ll << bits) <= (long long)h->P.numCells) ++bits;
    if ((rc = timed_launch(h, &h->tracer.seconds, [&] { sph_launch_tracers(h->P, A, plain, h->tracerWs, bits, h->compute); }))) return rc;
    h->tracer.calls += 1;
    return outbound_send(h, h->tracer.out, {{h->tracerPosDenHost.get(), h->tracerPosDen.get(), (size_t)m * sizeof(float4)},
                                           {h->tracerVelHost.get(), h->tracerVel.get(), (size_t)m * sizeof(float4)}});
}

int sph_tracers_host(sph_handle *h, const float **pos_den, const float **vel, int *m) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    HIPCHK(h, outbound_wait(h->tracer.out));
    const bool any = h->tracerCount > 0;
    if (pos_den) *pos_den = any ? &h->tracerPosDenHost.get()->x : nullptr;
    if (vel) *vel = any ? &h->tracerVelHost.get()->x : nullptr;
    if (m) *m = h->tracerCount;
    return SPH_OK;
}

int sph_get_tracer_stats(sph_handle *h, SphTracerStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphTracerStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->tracer.seconds, &h->tracer.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if ((rc = h->tracerCounters.read(h, reset))) return rc;
    if (const unsigned long long *c = h->tracerCounters.host) S.waves_shared = c[0], S.waves_direct = c[1], S.groups = c[2];
    *out = S;
    return SPH_OK;
}

} // extern "C"
