// Ray casting: sph_cast_rays and what reads its results; what it shares with sph_render_view (sph_frame.hip)
// (kernels: rays.hip).
#include "sph_handle.h"

#include <cmath>
#include <cstring>

using namespace sph_host;

namespace sph_host {

const char *bad_cast_radius(const sph_handle *h, float radius) {
    return radius == 0.f || (radius > 0.f && radius <= h->P.h) ? nullptr : "radius must be 0 (0.5 h) or 0 < radius <= h";
}

int cast_path(sph_handle *h, size_t rays, bool &plain) {
    plain = plain_path("SPH_CAST_PLAIN");
    if (plain && (unsigned long long)rays * (unsigned long long)(h->n > 0 ? h->n : 0) > (1ull << 32))
        return fail(h, SPH_EINVAL, "SPH_CAST_PLAIN: " + std::to_string(rays) + " rays x " + std::to_string(h->n) +
                                       " particles, more than the 2^32 pairs the check path admits");
    return SPH_OK;
}

int cast_prepare(sph_handle *h, CastArgs &A, float radius, bool plain) {
    A.S = sorted_stream(h);
    A.r = radius == 0.f ? 0.5f * h->P.h : radius;
    A.r2 = A.r * A.r;
    if (plain) return SPH_OK;
    const size_t waves = (size_t)sph_cast_waves(A);
    if (waves > h->castWaveCap) {
        HIPCHK(h, hipStreamSynchronize(h->compute)); // a queued count may still read the old words
        h->castWaveCap = 0;
        HIPCHK(h, h->castPartials.alloc(2 * waves));
        h->castWaveCap = waves;
    }
    if (int rc = h->castCounters.ensure(h)) return rc;
    A.partials = h->castPartials;
    A.counters = h->castCounters.dev;
    return SPH_OK;
}

void cast_account(sph_handle *h, const CastArgs &A, bool plain) {
    h->castRaysSum += (unsigned long long)A.m;
    if (plain) h->castPlainTests += (unsigned long long)A.m * (unsigned long long)A.S.n;
}

} // namespace sph_host

namespace {

// (re)allocate the rays and their words for m rays
int cast_reserve(sph_handle *h, size_t m) {
    if (m <= h->castCap) return SPH_OK;
    int rc = pass_quiesce(h, h->cast); // the old buffers may still be read by a queued copy
    if (rc) return rc;
    h->castCap = 0;
    HIPCHK(h, h->castRays.alloc(m));
    HIPCHK(h, h->castWords.alloc(m));
    HIPCHK(h, h->castWordsHost.alloc(m));
    h->castCap = m;
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_cast_rays(sph_handle *h, const SphRay *rays, int m, const SphCastOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the ray cast", ": multi-GPU runs cast no rays");
    if (rc) return rc;
    SphCastOptions o{};
    if ((rc = copy_options(h, opt, o, "SphCastOptions.struct_size is not set"))) return rc;
    if (const char *bad = bad_cast_radius(h, o.radius)) return fail(h, SPH_EINVAL, bad);
    if (m < 0 || m > SPH_CAST_MAX_RAYS) return fail(h, SPH_EINVAL, "m must be 0 .. 1 << 24");
    if (m > 0 && !rays) return fail(h, SPH_EINVAL, "rays is NULL");
    bool plain;
    if ((rc = cast_path(h, (size_t)m, plain))) return rc;
    if ((rc = cast_reserve(h, (size_t)m))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    if ((rc = outbound_fence(h, h->cast.out))) return rc; // the previous cast's copy still reads the device words
    h->cast.valid = false;
    if (m > 0) {
        static_assert(sizeof(SphRay) == 2 * sizeof(float4), "a ray is two float4");
        const auto fill = [&](size_t k, float4 *dst, size_t cnt) { memcpy(dst, reinterpret_cast<const float4 *>(rays) + k, cnt * sizeof(float4)); };
        if ((rc = staged_upload(h, reinterpret_cast<float4 *>(h->castRays.get()), 2 * (size_t)m, fill))) return rc;
        CastArgs A{};
        A.rays = h->castRays;
        A.m = m;
        A.words = h->castWords;
        if ((rc = cast_prepare(h, A, o.radius, plain))) return rc;
        if ((rc = timed_launch(h, &h->cast.seconds, [&] { sph_launch_cast(h->P, A, plain, h->compute); }))) return rc;
        h->cast.calls += 1;
        cast_account(h, A, plain);
        if ((rc = outbound_send(h, h->cast.out, {{h->castWordsHost.get(), h->castWords.get(), (size_t)m * sizeof(uint64_t)}}))) return rc;
    }
    h->castM = m;
    h->cast.valid = true;
    return SPH_OK;
}

int sph_cast_host(sph_handle *h, const uint64_t **words, int *m) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->cast.valid) return fail(h, SPH_ESTATE, "sph_cast_rays must come first");
    HIPCHK(h, outbound_wait(h->cast.out));
    if (words) *words = h->castM ? reinterpret_cast<const uint64_t *>(h->castWordsHost.get()) : nullptr;
    if (m) *m = h->castM;
    return SPH_OK;
}

int sph_get_cast_stats(sph_handle *h, SphCastStats *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SphCastStats S{};
    S.struct_size = (int32_t)sizeof S;
    int rc = timed_total(h, &h->cast.seconds, &h->cast.calls, &S.seconds, &S.calls, reset);
    if (rc) return rc;
    if ((rc = h->castCounters.read(h, reset))) return rc;
    if (const unsigned long long *c = h->castCounters.host) S.layers = c[0], S.tests = c[1];
    S.calls += h->castViews;
    S.rays = h->castRaysSum;
    S.tests += h->castPlainTests;
    if (reset) h->castViews = 0, h->castRaysSum = 0, h->castPlainTests = 0;
    *out = S;
    return SPH_OK;
}

} // extern "C"
