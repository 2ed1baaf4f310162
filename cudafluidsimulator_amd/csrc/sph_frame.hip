// The visualiser's frame: sph_render_frame / sph_render_field / sph_render_column and what reads their results
// (kernels: render.hip).
#include "sph_handle.h"

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

using namespace sph_host;

namespace {

// (re)allocate the frame buffers for a width x height image and draw the static edge layer
int render_resize(sph_handle *h, int width, int height) {
    if (h->rp.width == width && h->rp.height == height && h->rDepth) return SPH_OK;
    // the old buffers may still be read by a queued compose / frame copy
    int rc = pass_quiesce(h, h->frame);
    if (rc) return rc;
    h->rPacked.reset(); // (sized by the image: the next field or column frame allocates it again)
    h->rRays.reset();
    h->frameKind = FrameKind::Flat;
    h->rp.width = h->rp.height = 0;
    const size_t npix = (size_t)width * (size_t)height;
    const size_t rgbBytes = (npix + 3) / 4 * 12; // whole groups of four pixels (k_render_compose)
    HIPCHK(h, h->rDepth.alloc(npix));
    HIPCHK(h, h->rCount.alloc(npix));
    HIPCHK(h, h->rEdge.alloc(npix));
    HIPCHK(h, h->rRgb.alloc(rgbBytes / sizeof(uint32_t)));
    HIPCHK(h, h->frameHost.alloc(rgbBytes));
    memset(h->frameHost, 0, rgbBytes);
    RenderParams R = h->rp;
    R.width = width;
    R.height = height;
    R.Wf = (float)width;
    R.Hf = (float)height;
    sph_launch_render_edges(R, h->rEdge, h->compute);
    HIPCHK(h, hipGetLastError());
    h->rp = R;
    return SPH_OK;
}

// The renderers up to their launch: state and option checks (`rest(o)`: the entry point's own, a message or
// null), the buffers, the wait for the previous frame's copy.
template <class Opt, class Rest>
int frame_begin(sph_handle *h, const Opt *opt, const char *unset, Rest rest, FrameKind kind, Opt &o, bool &plain) {
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU frames are not rendered");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    int rc = copy_options(h, opt, o, unset);
    if (rc) return rc;
    const int width = o.width == 0 ? 800 : o.width, height = o.height == 0 ? 600 : o.height;
    int pointSize = 3; // (the column frame draws no points)
    if constexpr (!std::is_same_v<Opt, SphColumnFrameOptions>) pointSize = o.point_size == 0 ? 3 : o.point_size;
    if (width < 1 || width > 4096 || height < 1 || height > 4096) return fail(h, SPH_EINVAL, "frame size must be 1..4096 x 1..4096");
    if (pointSize < 1 || pointSize > 9 || (pointSize & 1) == 0) return fail(h, SPH_EINVAL, "point_size must be odd, 1..9");
    if (const char *bad = rest(o)) return fail(h, SPH_EINVAL, bad);
    if ((rc = render_resize(h, width, height))) return rc;
    if (kind != FrameKind::Flat) {
        if (!h->rPacked) HIPCHK(h, h->rPacked.alloc((size_t)width * height));
        if (!h->rRange) HIPCHK(h, h->rRange.alloc(2));
        if (!h->rangeHost) HIPCHK(h, h->rangeHost.alloc(2));
    }
    if (kind == FrameKind::Column) {
        if (!h->rColumnMax) HIPCHK(h, h->rColumnMax.alloc(1));
        if (!h->rRays) {
            HIPCHK(h, h->rRays.alloc((size_t)width + height));
            sph_launch_column_rays(h->rp, h->rRays, h->compute);
            HIPCHK(h, hipGetLastError());
        }
    }
    h->rp.radius = (pointSize - 1) / 2;
    plain = plain_path("SPH_RENDER_PLAIN");
    return outbound_fence(h, h->frame.out); // the previous frame's copy still reads the device frame the compose is about to rewrite
}

// ... and after it: the counters, the frame (a field or column frame: and the range of its colour scale) on its way
// to pinned memory
int frame_finish(sph_handle *h, FrameKind kind) {
    h->frame.calls += 1;
    h->frame.valid = true;
    h->frameKind = kind;
    const OutboundCopy frame{h->frameHost.get(), h->rRgb.get(), (size_t)h->rp.width * h->rp.height * 3};
    if (kind == FrameKind::Flat) return outbound_send(h, h->frame.out, {frame});
    return outbound_send(h, h->frame.out, {frame, {h->rangeHost.get(), h->rRange.get(), 2 * sizeof(uint32_t)}});
}

} // namespace

extern "C" {

int sph_render_frame(sph_handle *h, const SphRenderOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphRenderOptions o{};
    bool plain = false;
    auto rest = [](const SphRenderOptions &o) -> const char * {
        return o.shade != SPH_SHADE_FLAT && o.shade != SPH_SHADE_COUNT ? "unknown shade" : nullptr;
    };
    int rc = frame_begin(h, opt, "SphRenderOptions.struct_size is not set", rest, FrameKind::Flat, o, plain);
    if (rc) return rc;
    h->rp.shade = o.shade;
    // The current state: after a step the rows the force sweep wrote, still in that step's cell-sorted order;
    // after setup / upload / load (and always with SPH_SWEEP_LINKED) in particle-id order.  A grid built
    // ahead for the next step only reads these rows.
    rc = timed_launch(h, &h->frame.seconds, [&] { sph_launch_render(h->rp, h->pos4[h->cur], h->n, plain, h->rDepth, h->rCount, h->rEdge, h->rRgb, h->compute); });
    return rc ? rc : frame_finish(h, FrameKind::Flat);
}

const uint8_t *sph_frame_host(sph_handle *h, int *width, int *height) {
    if (!h) return nullptr;
    if (!h->frame.valid) {
        h->err = "sph_render_frame must come first";
        return nullptr;
    }
    if (outbound_wait(h->frame.out) != hipSuccess) {
        h->err = "frame copy failed";
        return nullptr;
    }
    if (width) *width = h->rp.width;
    if (height) *height = h->rp.height;
    return h->frameHost;
}

int sph_download_frame_buffers(sph_handle *h, uint32_t *depth_bits, uint32_t *count, uint32_t *edge_depth_bits) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->frame.valid) return fail(h, SPH_ESTATE, "sph_render_frame must come first");
    if (h->frameKind == FrameKind::Column) return fail(h, SPH_ESTATE, "the last render was a column frame: it writes no depth or count (sph_download_column_buffer)");
    HIPCHK(h, hipStreamSynchronize(h->compute));
    const size_t bytes = (size_t)h->rp.width * h->rp.height * sizeof(uint32_t);
    if (depth_bits) HIPCHK(h, hipMemcpy(depth_bits, h->rDepth, bytes, hipMemcpyDeviceToHost));
    if (count) HIPCHK(h, hipMemcpy(count, h->rCount, bytes, hipMemcpyDeviceToHost));
    if (edge_depth_bits) HIPCHK(h, hipMemcpy(edge_depth_bits, h->rEdge, bytes, hipMemcpyDeviceToHost));
    return SPH_OK;
}

int sph_get_render_time(sph_handle *h, double *seconds, int64_t *frames, int reset) {
    if (!h) return SPH_EINVAL;
    return timed_total(h, &h->frame.seconds, &h->frame.calls, seconds, frames, reset);
}

int sph_render_field(sph_handle *h, const SphFieldFrameOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphFieldFrameOptions o{};
    bool plain = false;
    auto rest = [](const SphFieldFrameOptions &o) -> const char * {
        if (bad_field(o.field)) return "unknown field";
        if (!std::isfinite(o.value_lo) || !std::isfinite(o.value_hi)) return "value_lo / value_hi must be finite";
        return o.value_hi < o.value_lo ? "value_hi < value_lo" : nullptr;
    };
    int rc = frame_begin(h, opt, "SphFieldFrameOptions.struct_size is not set", rest, FrameKind::Field, o, plain);
    if (rc) return rc;
    const bool autoRange = o.value_lo == 0.f && o.value_hi == 0.f;
    // pos4[cur] / vel4[cur]: the rows sph_render_frame draws and the rows sph_download_state reads
    rc = timed_launch(h, &h->frame.seconds, [&] {
        sph_launch_render_field(h->rp, h->pos4[h->cur], h->vel4[h->cur], h->n, plain, o.field, autoRange, o.value_lo, o.value_hi,
                                h->rPacked, h->rDepth, h->rCount, h->rEdge, h->rRange, h->rRgb, h->compute);
    });
    return rc ? rc : frame_finish(h, FrameKind::Field);
}

int sph_download_field_buffer(sph_handle *h, uint32_t *value_bits) {
    if (!h || !value_bits) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->frame.valid || h->frameKind != FrameKind::Field) return fail(h, SPH_ESTATE, "the last render was not a field frame (sph_render_field)");
    HIPCHK(h, hipStreamSynchronize(h->compute));
    const size_t npix = (size_t)h->rp.width * h->rp.height;
    std::vector<unsigned long long> packed(npix);
    HIPCHK(h, hipMemcpy(packed.data(), h->rPacked, npix * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) value_bits[i] = (uint32_t)packed[i]; // the low words
    return SPH_OK;
}

int sph_field_range(sph_handle *h, float *lo, float *hi) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->frame.valid || h->frameKind != FrameKind::Field) return fail(h, SPH_ESTATE, "the last render was not a field frame (sph_render_field)");
    HIPCHK(h, outbound_wait(h->frame.out));
    if (lo) memcpy(lo, &h->rangeHost[0], sizeof(float));
    if (hi) memcpy(hi, &h->rangeHost[1], sizeof(float));
    return SPH_OK;
}

int sph_render_column(sph_handle *h, const SphColumnFrameOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphColumnFrameOptions o{};
    bool plain = false;
    auto rest = [](const SphColumnFrameOptions &o) -> const char * {
        if (!std::isfinite(o.value_lo) || !std::isfinite(o.value_hi)) return "value_lo / value_hi must be finite";
        return o.value_hi < o.value_lo ? "value_hi < value_lo" : nullptr;
    };
    int rc = frame_begin(h, opt, "SphColumnFrameOptions.struct_size is not set", rest, FrameKind::Column, o, plain);
    if (rc) return rc;
    const bool autoRange = o.value_lo == 0.f && o.value_hi == 0.f;
    // pos4[cur]: the rows sph_render_frame draws; h and the kernel coefficient: the handle's settings
    rc = timed_launch(h, &h->frame.seconds, [&] {
        sph_launch_render_column(h->rp, h->pos4[h->cur], h->n, plain, h->P.h, h->P.h2, h->P.dcoef, autoRange, o.value_lo, o.value_hi,
                                 h->rRays, h->rPacked, h->rColumnMax, h->rEdge, h->rRange, h->rRgb, h->compute);
    });
    return rc ? rc : frame_finish(h, FrameKind::Column);
}

int sph_download_column_buffer(sph_handle *h, uint64_t *column_words) {
    if (!h || !column_words) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->frame.valid || h->frameKind != FrameKind::Column) return fail(h, SPH_ESTATE, "the last render was not a column frame (sph_render_column)");
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipMemcpy(column_words, h->rPacked, (size_t)h->rp.width * h->rp.height * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SPH_OK;
}

int sph_column_range(sph_handle *h, float *lo, float *hi) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->frame.valid || h->frameKind != FrameKind::Column) return fail(h, SPH_ESTATE, "the last render was not a column frame (sph_render_column)");
    HIPCHK(h, outbound_wait(h->frame.out));
    if (lo) memcpy(lo, &h->rangeHost[0], sizeof(float));
    if (hi) memcpy(hi, &h->rangeHost[1], sizeof(float));
    return SPH_OK;
}

} // extern "C"
