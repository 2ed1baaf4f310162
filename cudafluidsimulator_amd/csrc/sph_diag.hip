// Run diagnostics: sph_diagnose / sph_slab_diagnose and what reads their result (kernels: diag.hip; the pure host
// functions sph_diagnostics_values / sph_diagnostics_add: sph_diag_values.cpp).
#include "sph_handle.h"

#include <cmath>

using namespace sph_host;

namespace {

const char *const kUnset = "SphDiagnosticsOptions.struct_size is not set";

// the caller's options into `o` (NULL: no histogram), checked
int diag_options(sph_handle *h, const SphDiagnosticsOptions *opt, SphDiagnosticsOptions &o) {
    o = SphDiagnosticsOptions{};
    o.hist_field = -1;
    int rc = copy_options(h, opt, o, kUnset);
    if (rc) return rc;
    if (o.hist_field == -1) return SPH_OK;
    if (bad_field(o.hist_field)) return fail(h, SPH_EINVAL, "unknown field");
    if (!std::isfinite(o.value_lo) || !std::isfinite(o.value_hi)) return fail(h, SPH_EINVAL, "value_lo / value_hi must be finite");
    if (o.value_hi < o.value_lo) return fail(h, SPH_EINVAL, "value_hi < value_lo");
    return SPH_OK;
}

// clear + reduce (+ histogram) of `n` rows on the compute stream, timed, and the result block on its way to pinned memory
int diag_run(sph_handle *h, const float4 *pos, const float4 *vel, int n, const SphDiagnosticsOptions &o) {
    if (!h->diagDev) HIPCHK(h, h->diagDev.alloc(1));
    if (!h->diagHost) HIPCHK(h, h->diagHost.alloc(1));
    const bool plain = plain_path("SPH_DIAG_PLAIN");
    int rc = outbound_fence(h, h->diag.out); // the previous call's copy still reads the block the clear is about to rewrite
    if (rc) return rc;
    DiagArgs A{};
    A.pos = pos, A.vel = vel, A.stride = 1;
    A.n = n;
    A.histField = o.hist_field;
    A.autoRange = o.hist_field >= 0 && o.value_lo == 0.f && o.value_hi == 0.f;
    A.lo = o.value_lo, A.hi = o.value_hi;
    if ((rc = timed_launch(h, &h->diag.seconds, [&] { sph_launch_diagnose(A, plain, h->diagDev, h->compute); }))) return rc;
    h->diag.calls += 1;
    h->diag.valid = false; // (until the copy is queued: the pinned block still holds the previous result)
    if ((rc = outbound_send(h, h->diag.out, {{h->diagHost.get(), h->diagDev.get(), sizeof(DiagBlock)}}))) return rc;
    h->diagN = n;
    h->diagOpt = o;
    h->diagAuto = A.autoRange != 0;
    h->diag.valid = true;
    return SPH_OK;
}

uint32_t unkey(uint32_t k) { return (k >> 31) ? (k ^ 0x80000000u) : ~k; }

uint32_t bits_of(float f) {
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return b;
}

} // namespace

extern "C" {

int sph_diagnose(sph_handle *h, const SphDiagnosticsOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": use sph_slab_diagnose");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    SphDiagnosticsOptions o;
    int rc = diag_options(h, opt, o);
    if (rc) return rc;
    // pos4[cur] / vel4[cur]: the rows sph_render_field draws and sph_download_state reads.  A grid built ahead for the
    // next step, and an open grid phase, only read them.
    return diag_run(h, h->pos4[h->cur], h->vel4[h->cur], h->n, o);
}

int sph_slab_diagnose(sph_handle *h, int buf, int i_begin, int i_end, const SphDiagnosticsOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->external) return fail(h, SPH_ESTATE, "create with SPH_FLAG_EXTERNAL_STATE");
    SphDiagnosticsOptions o;
    int rc = diag_options(h, opt, o);
    if (rc) return rc;
    if (o.hist_field >= 0 && o.value_lo == 0.f && o.value_hi == 0.f)
        return fail(h, SPH_EINVAL, "a slab cannot know the global range: give value_lo / value_hi");
    if (!h->pos4[0]) return fail(h, SPH_ESTATE, "sph_bind_buffers first");
    if ((buf != 0 && buf != 1) || i_begin < 0 || i_end < i_begin || i_end > h->cap) return fail(h, SPH_EINVAL, "bad slab range");
    return diag_run(h, h->pos4[buf] + i_begin, h->vel4[buf] + i_begin, i_end - i_begin, o);
}

int sph_diagnostics_host(sph_handle *h, SphDiagnosticsRaw *out) {
    if (!h || !out) return SPH_EINVAL;
    if (!h->diag.valid) return fail(h, SPH_ESTATE, "sph_diagnose must come first");
    SPH_ON_DEVICE(h);
    HIPCHK(h, outbound_wait(h->diag.out));
    const DiagBlock &B = *h->diagHost;
    SphDiagnosticsRaw R{};
    R.struct_size = (int32_t)sizeof R;
    R.n = h->diagN;
    for (int k = 0; k < SPH_DIAG_SUMS; ++k) {
        // the two integer sums joined: 2^32 (sum of the high words) + (sum of the low words), in 128 bits
        const __int128 s = (__int128)B.hi[k] * ((__int128)1 << 32) + (__int128)B.lo[k];
        R.sum[k].lo = (uint64_t)s;
        R.sum[k].hi = (int64_t)(s >> 64);
    }
    for (int k = 0; k < SPH_DIAG_EXTREMA; ++k) {
        R.min_bits[k] = h->diagN > 0 ? unkey(B.minKey[k]) : 0x7F800000u;
        R.max_bits[k] = h->diagN > 0 ? unkey(B.maxKey[k]) : 0xFF800000u;
    }
    R.saturated = B.saturated;
    R.hist_field = h->diagOpt.hist_field;
    if (R.hist_field >= 0) {
        const int e = R.hist_field == SPH_FIELD_SPEED ? SPH_DIAG_EXT_SPEED
                      : R.hist_field == SPH_FIELD_DENSITY ? SPH_DIAG_EXT_RHO : SPH_DIAG_EXT_PRS;
        // (an automatic range over no rows: the identities)
        R.hist_lo_bits = !h->diagAuto ? bits_of(h->diagOpt.value_lo) : h->diagN > 0 ? B.range[0] : R.min_bits[e];
        R.hist_hi_bits = !h->diagAuto ? bits_of(h->diagOpt.value_hi) : h->diagN > 0 ? B.range[1] : R.max_bits[e];
        for (int k = 0; k < SPH_DIAG_BINS; ++k) R.hist[k] = B.hist[k];
    }
    *out = R;
    return SPH_OK;
}

int sph_get_diagnostics_time(sph_handle *h, double *seconds, int64_t *calls, int reset) {
    if (!h) return SPH_EINVAL;
    return timed_total(h, &h->diag.seconds, &h->diag.calls, seconds, calls, reset);
}

} // extern "C"
