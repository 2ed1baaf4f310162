// The visualiser's frame: sph_render_frame / sph_render_field / sph_render_column / sph_render_liquid / sph_render_view
// and what reads their results
// (kernels: render.hip; the view's: rays.hip).
#include "sph_handle.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace sph_host;

namespace {

// (re)allocate the frame buffers for a width x height image and draw the static edge layer
int render_resize(sph_handle *h, int width, int height) {
    FrameState &f = h->frame;
    if (f.rp.width == width && f.rp.height == height && f.depth) return SPH_OK;
    // the old buffers may still be read by a queued compose / frame copy
    int rc = pass_quiesce(h, f.pass);
    if (rc) return rc;
    f.packed.reset(); // (sized by the image: the next field or column frame allocates it again)
    f.rays.reset();
    f.smooth[0].reset();
    f.smooth[1].reset();
    f.normals.reset();
    f.smoothed = nullptr;
    f.kind = FrameKind::Flat;
    f.rp.width = f.rp.height = 0;
    const size_t npix = (size_t)width * (size_t)height;
    const size_t rgbBytes = (npix + 3) / 4 * 12; // whole groups of four pixels (k_render_compose)
    HIPCHK(h, f.depth.alloc(npix));
    HIPCHK(h, f.count.alloc(npix));
    HIPCHK(h, f.edge.alloc(npix));
    HIPCHK(h, f.rgb.alloc(rgbBytes / sizeof(uint32_t)));
    HIPCHK(h, f.host.alloc(rgbBytes));
    memset(f.host, 0, rgbBytes);
    RenderParams R = f.rp;
    R.width = width;
    R.height = height;
    R.Wf = (float)width;
    R.Hf = (float)height;
    sph_launch_render_edges(R, f.edge, h->compute);
    HIPCHK(h, hipGetLastError());
    f.rp = R;
    return SPH_OK;
}

// the frame's device buffers, as the launchers of render.hip take them
FrameView frame_view(const sph_handle *h) {
    const FrameState &f = h->frame;
    return {f.depth, f.count, f.edge, f.rgb, f.packed, f.range, f.maxWord, f.rays, {f.smooth[0], f.smooth[1]}, f.normals};
}

// the value range of the field and column options: a message or null
const char *bad_value_range(float lo, float hi) {
    if (!std::isfinite(lo) || !std::isfinite(hi)) return "value_lo / value_hi must be finite";
    return hi < lo ? "value_hi < value_lo" : nullptr;
}

// The renderers up to their launch: the state checks, the caller's options into `o`, the option checks (pointSize: the
// option in `o`, null for the column and liquid frames, which draw no points; `rest(o)`: the entry point's own, a message or null),
// the buffers, the wait for the previous frame's copy.
template <class Opt, class Rest>
int frame_begin(sph_handle *h, const Opt *opt, const char *unset, Opt &o, const int32_t *pointSize, Rest rest, FrameKind kind) {
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, ": multi-GPU frames are not rendered");
    if (!h->ready) return fail(h, SPH_ESTATE, "setup()/upload_state() must come first");
    int rc = copy_options(h, opt, o, unset);
    if (rc) return rc;
    FrameState &f = h->frame;
    const int width = o.width == 0 ? 800 : o.width, height = o.height == 0 ? 600 : o.height;
    const int points = pointSize && *pointSize ? *pointSize : 3;
    if (width < 1 || width > 4096 || height < 1 || height > 4096) return fail(h, SPH_EINVAL, "frame size must be 1..4096 x 1..4096");
    if (points < 1 || points > 9 || (points & 1) == 0) return fail(h, SPH_EINVAL, "point_size must be odd, 1..9");
    if (const char *bad = rest(o)) return fail(h, SPH_EINVAL, bad);
    if ((rc = render_resize(h, width, height))) return rc;
    if (kind != FrameKind::Flat) {
        if (!f.packed) HIPCHK(h, f.packed.alloc((size_t)width * height));
        if (!f.range) HIPCHK(h, f.range.alloc(2));
        if (!f.rangeHost) HIPCHK(h, f.rangeHost.alloc(2));
    }
    if (kind == FrameKind::Column || kind == FrameKind::Liquid) {
        if (!f.maxWord) HIPCHK(h, f.maxWord.alloc(1));
        if (!f.rays) {
            HIPCHK(h, f.rays.alloc((size_t)width + height));
            sph_launch_column_rays(f.rp, f.rays, h->compute);
            HIPCHK(h, hipGetLastError());
        }
    }
    if (kind == FrameKind::Liquid) {
        const size_t npix = (size_t)width * height;
        for (auto &plane : f.smooth)
            if (!plane) HIPCHK(h, plane.alloc(npix));
        if (!f.normals) HIPCHK(h, f.normals.alloc(npix));
    }
    f.rp.radius = (points - 1) / 2;
    return outbound_fence(h, f.pass.out); // the previous frame's copy still reads the device frame the compose is about to rewrite
}

// ... and after it: the timed launch, the counters, the frame (a field or column frame: and the range of its colour
// scale) on its way to pinned memory
template <class Launch>
int frame_finish(sph_handle *h, FrameKind kind, Launch launch) {
    FrameState &f = h->frame;
    int rc = timed_launch(h, &f.pass.seconds, launch);
    if (rc) return rc;
    f.pass.calls += 1;
    f.pass.valid = true;
    f.kind = kind;
    const OutboundCopy frame{f.host.get(), f.rgb.get(), (size_t)f.rp.width * f.rp.height * 3};
    if (kind == FrameKind::Flat || kind == FrameKind::Liquid || kind == FrameKind::View) return outbound_send(h, f.pass.out, {frame}); // (no colour scale to report)
    return outbound_send(h, f.pass.out, {frame, {f.rangeHost.get(), f.range.get(), 2 * sizeof(uint32_t)}});
}

// the last render exists and was of this kind, else SPH_ESTATE with this message
int last_frame_was(sph_handle *h, FrameKind kind) {
    SPH_ON_DEVICE(h);
    if (h->frame.pass.valid && h->frame.kind == kind) return SPH_OK;
    return fail(h, SPH_ESTATE, kind == FrameKind::Field    ? "the last render was not a field frame (sph_render_field)"
                               : kind == FrameKind::Column ? "the last render was not a column frame (sph_render_column)"
                               : kind == FrameKind::View   ? "the last render was not a view frame (sph_render_view)"
                                                           : "the last render was not a liquid frame (sph_render_liquid)");
}

// sph_field_range / sph_column_range
int frame_range(sph_handle *h, FrameKind kind, float *lo, float *hi) {
    if (!h) return SPH_EINVAL;
    if (int rc = last_frame_was(h, kind)) return rc;
    HIPCHK(h, outbound_wait(h->frame.pass.out));
    if (lo) memcpy(lo, &h->frame.rangeHost[0], sizeof(float));
    if (hi) memcpy(hi, &h->frame.rangeHost[1], sizeof(float));
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_render_frame(sph_handle *h, const SphRenderOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphRenderOptions o{};
    auto rest = [](const SphRenderOptions &o) { return o.shade != SPH_SHADE_FLAT && o.shade != SPH_SHADE_COUNT ? "unknown shade" : nullptr; };
    if (int rc = frame_begin(h, opt, "SphRenderOptions.struct_size is not set", o, &o.point_size, rest, FrameKind::Flat)) return rc;
    h->frame.rp.shade = o.shade;
    // The current state: after a step the rows the force sweep wrote, still in that step's cell-sorted order;
    // after setup / upload / load (and always with SPH_SWEEP_LINKED) in particle-id order.  A grid built
    // ahead for the next step only reads these rows.
    return frame_finish(h, FrameKind::Flat, [&] { sph_launch_render(h->frame.rp, frame_view(h), h->pos4[h->cur], h->n, plain_path("SPH_RENDER_PLAIN"), h->compute); });
}

const uint8_t *sph_frame_host(sph_handle *h, int *width, int *height) {
    if (!h) return nullptr;
    if (!h->frame.pass.valid) {
        h->err = "sph_render_frame must come first";
        return nullptr;
    }
    if (outbound_wait(h->frame.pass.out) != hipSuccess) {
        h->err = "frame copy failed";
        return nullptr;
    }
    if (width) *width = h->frame.rp.width;
    if (height) *height = h->frame.rp.height;
    return h->frame.host;
}

int sph_download_frame_buffers(sph_handle *h, uint32_t *depth_bits, uint32_t *count, uint32_t *edge_depth_bits) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    const FrameState &f = h->frame;
    if (!f.pass.valid) return fail(h, SPH_ESTATE, "sph_render_frame must come first");
    if (f.kind == FrameKind::Column) return fail(h, SPH_ESTATE, "the last render was a column frame: it writes no depth or count (sph_download_column_buffer)");
    if (f.kind == FrameKind::Liquid) return fail(h, SPH_ESTATE, "the last render was a liquid frame: it writes no point depth or count (sph_download_liquid_buffers)");
    if (f.kind == FrameKind::View) return fail(h, SPH_ESTATE, "the last render was a view frame: it writes no point depth or count (sph_download_view_buffer)");
    HIPCHK(h, hipStreamSynchronize(h->compute));
    const size_t bytes = (size_t)f.rp.width * f.rp.height * sizeof(uint32_t);
    if (depth_bits) HIPCHK(h, hipMemcpy(depth_bits, f.depth, bytes, hipMemcpyDeviceToHost));
    if (count) HIPCHK(h, hipMemcpy(count, f.count, bytes, hipMemcpyDeviceToHost));
    if (edge_depth_bits) HIPCHK(h, hipMemcpy(edge_depth_bits, f.edge, bytes, hipMemcpyDeviceToHost));
    return SPH_OK;
}

int sph_get_render_time(sph_handle *h, double *seconds, int64_t *frames, int reset) {
    if (!h) return SPH_EINVAL;
    return timed_total(h, &h->frame.pass.seconds, &h->frame.pass.calls, seconds, frames, reset);
}

int sph_render_field(sph_handle *h, const SphFieldFrameOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphFieldFrameOptions o{};
    auto rest = [](const SphFieldFrameOptions &o) { return bad_field(o.field) ? "unknown field" : bad_value_range(o.value_lo, o.value_hi); };
    if (int rc = frame_begin(h, opt, "SphFieldFrameOptions.struct_size is not set", o, &o.point_size, rest, FrameKind::Field)) return rc;
    const bool autoRange = o.value_lo == 0.f && o.value_hi == 0.f;
    // pos4[cur] / vel4[cur]: the rows sph_render_frame draws and the rows sph_download_state reads
    return frame_finish(h, FrameKind::Field, [&] {
        sph_launch_render_field(h->frame.rp, frame_view(h), h->pos4[h->cur], h->vel4[h->cur], h->n, plain_path("SPH_RENDER_PLAIN"), o.field,
                                autoRange,
                                o.value_lo, o.value_hi, h->compute);
    });
}

int sph_download_field_buffer(sph_handle *h, uint32_t *value_bits) {
    if (!h || !value_bits) return SPH_EINVAL;
    if (int rc = last_frame_was(h, FrameKind::Field)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->compute));
    const size_t npix = (size_t)h->frame.rp.width * h->frame.rp.height;
    std::vector<unsigned long long> packed(npix);
    HIPCHK(h, hipMemcpy(packed.data(), h->frame.packed, npix * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) value_bits[i] = (uint32_t)packed[i]; // the low words
    return SPH_OK;
}

int sph_field_range(sph_handle *h, float *lo, float *hi) { return frame_range(h, FrameKind::Field, lo, hi); }

int sph_render_column(sph_handle *h, const SphColumnFrameOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphColumnFrameOptions o{};
    auto rest = [](const SphColumnFrameOptions &o) { return bad_value_range(o.value_lo, o.value_hi); };
    if (int rc = frame_begin(h, opt, "SphColumnFrameOptions.struct_size is not set", o, nullptr, rest, FrameKind::Column)) return rc;
    const bool autoRange = o.value_lo == 0.f && o.value_hi == 0.f;
    // pos4[cur]: the rows sph_render_frame draws; h and the kernel coefficient: the handle's settings
    return frame_finish(h, FrameKind::Column, [&] {
        sph_launch_render_column(h->frame.rp, frame_view(h), h->pos4[h->cur], h->n, plain_path("SPH_RENDER_PLAIN"), h->P.h, h->P.h2, h->P.dcoef, autoRange,
                                 o.value_lo, o.value_hi, h->compute);
    });
}

int sph_download_column_buffer(sph_handle *h, uint64_t *column_words) {
    if (!h || !column_words) return SPH_EINVAL;
    if (int rc = last_frame_was(h, FrameKind::Column)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipMemcpy(column_words, h->frame.packed, (size_t)h->frame.rp.width * h->frame.rp.height * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SPH_OK;
}

int sph_column_range(sph_handle *h, float *lo, float *hi) { return frame_range(h, FrameKind::Column, lo, hi); }

int sph_render_liquid(sph_handle *h, const SphLiquidFrameOptions *opt) {
    if (!h) return SPH_EINVAL;
    SphLiquidFrameOptions o{};
    const float hh = h->P.h; // (read again behind frame_begin's state checks; a handle without state fails there)
    auto rest = [hh](const SphLiquidFrameOptions &o) -> const char * {
        if (!(o.radius == 0.f || (o.radius > 0.f && o.radius <= hh))) return "radius must be 0 (h) or 0 < radius <= h";
        if (o.smooth_iterations < -1 || o.smooth_iterations > 8) return "smooth_iterations must be -1..8";
        if (o.smooth_radius < -1 || o.smooth_radius > 7) return "smooth_radius must be -1..7";
        if (!(o.smooth_depth >= 0.f) || !std::isfinite(o.smooth_depth)) return "smooth_depth must be finite and > 0 (0: 2 radius)";
        for (float l : o.light)
            if (!std::isfinite(l)) return "light must be finite";
        if (!(o.thickness_scale >= 0.f) || !std::isfinite(o.thickness_scale)) return "thickness_scale must be finite and >= 0";
        return nullptr;
    };
    if (int rc = frame_begin(h, opt, "SphLiquidFrameOptions.struct_size is not set", o, nullptr, rest, FrameKind::Liquid)) return rc;
    LiquidParams Q{};
    Q.radius = o.radius == 0.f ? h->P.h : o.radius;
    Q.h = h->P.h, Q.h2 = h->P.h2, Q.dcoef = h->P.dcoef;
    Q.smoothIterations = o.smooth_iterations == 0 ? 3 : o.smooth_iterations < 0 ? 0 : o.smooth_iterations;
    Q.smoothRadius = o.smooth_radius == 0 ? 3 : o.smooth_radius < 0 ? 0 : o.smooth_radius;
    Q.smoothDepth = o.smooth_depth == 0.f ? 2.f * Q.radius : o.smooth_depth;
    const bool dark = o.light[0] == 0.f && o.light[1] == 0.f && o.light[2] == 0.f;
    const float sun[3] = {-0.35f, 0.8f, 0.5f};
    for (int k = 0; k < 3; ++k) Q.light[k] = dark ? sun[k] : o.light[k];
    Q.autoThickness = o.thickness_scale == 0.f;
    Q.thickness = o.thickness_scale;
    // pos4[cur]: the rows sph_render_frame draws
    return frame_finish(h, FrameKind::Liquid, [&] {
        h->frame.smoothed = sph_launch_render_liquid(h->frame.rp, frame_view(h), h->pos4[h->cur], h->n, plain_path("SPH_RENDER_PLAIN"), Q, h->compute);
    });
}

int sph_download_liquid_buffers(sph_handle *h, uint32_t *front_bits, uint32_t *smooth_depth_bits, float *normals_xyz,
                                uint64_t *column_words) {
    if (!h) return SPH_EINVAL;
    if (int rc = last_frame_was(h, FrameKind::Liquid)) return rc;
    const FrameState &f = h->frame;
    HIPCHK(h, hipStreamSynchronize(h->compute));
    const size_t npix = (size_t)f.rp.width * f.rp.height;
    if (front_bits) HIPCHK(h, hipMemcpy(front_bits, f.depth, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (smooth_depth_bits) HIPCHK(h, hipMemcpy(smooth_depth_bits, f.smoothed, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (column_words) HIPCHK(h, hipMemcpy(column_words, f.packed, npix * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (normals_xyz) {
        std::vector<float4> n4(npix);
        HIPCHK(h, hipMemcpy(n4.data(), f.normals, npix * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < npix; ++i) normals_xyz[3 * i] = n4[i].x, normals_xyz[3 * i + 1] = n4[i].y, normals_xyz[3 * i + 2] = n4[i].z;
    }
    return SPH_OK;
}

// the view's basis, fp32, every operation rounded on its own; false: g or s0 vanishes or is not finite
static bool view_basis(const SphViewOptions &o, ViewCamera &C) {
    const auto dot = [](const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    const auto usable = [&](const float (&a)[3]) {
        const float d = dot(a, a);
        return std::isfinite(d) && d > 0.f && std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]);
    };
    float g[3], s0[3];
    for (int a = 0; a < 3; ++a) g[a] = o.target[a] - o.eye[a];
    if (!usable(g)) return false;
    const float glen = sqrtf(dot(g, g));
    for (int a = 0; a < 3; ++a) C.fwd[a] = g[a] / glen;
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        s0[a] = C.fwd[b] * o.up[c] - C.fwd[c] * o.up[b];
    }
    if (!usable(s0)) return false;
    const float slen = sqrtf(dot(s0, s0));
    for (int a = 0; a < 3; ++a) C.s[a] = s0[a] / slen;
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        C.u[a] = C.s[b] * C.fwd[c] - C.s[c] * C.fwd[b];
    }
    for (int a = 0; a < 3; ++a) C.eye[a] = o.eye[a];
    return true;
}

int sph_render_view(sph_handle *h, const SphViewOptions *opt) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = analysis_begin(h, "the view frame", ": multi-GPU frames are not rendered");
    if (rc) return rc;
    const char *unset = "SphViewOptions.struct_size is not set";
    if (!opt) return fail(h, SPH_EINVAL, unset); // (no defaults: a camera has to be given)
    SphViewOptions o{};
    ViewCamera cam{};
    auto rest = [&](const SphViewOptions &o) -> const char * {
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(o.eye[a]) || !std::isfinite(o.target[a]) || !std::isfinite(o.up[a])) return "eye, target and up must be finite";
        if (!view_basis(o, cam)) return "target - eye and (target - eye) x up must not vanish";
        const bool noTan = o.tan_half_x == 0.f && o.tan_half_y == 0.f;
        if (!noTan && !(o.tan_half_x > 0.f && o.tan_half_x <= 1024.f && o.tan_half_y > 0.f && o.tan_half_y <= 1024.f))
            return "tan_half_x / tan_half_y must both be 0 or both in (0, 1024]";
        if (!(o.near >= 0.f) || !std::isfinite(o.near)) return "near must be finite and >= 0 (0: h)";
        if (!(o.far >= 0.f)) return "far must be >= 0 (0: +inf)";
        if (o.far != 0.f && o.far < (o.near == 0.f ? h->P.h : o.near)) return "far < near";
        if (const char *bad = bad_cast_radius(h, o.radius)) return bad;
        if (o.shade != SPH_VIEW_FLAT && bad_field(o.shade - SPH_VIEW_FIELD)) return "unknown shade";
        if (const char *bad = bad_value_range(o.value_lo, o.value_hi)) return bad;
        for (float l : o.light)
            if (!std::isfinite(l)) return "light must be finite";
        if (!std::isfinite(o.edge_radius)) return "edge_radius must be finite";
        return nullptr;
    };
    if ((rc = frame_begin(h, opt, unset, o, nullptr, rest, FrameKind::View))) return rc;
    FrameState &f = h->frame;
    cam.width = f.rp.width, cam.height = f.rp.height;
    cam.Wf = f.rp.Wf, cam.Hf = f.rp.Hf;
    cam.tanY = o.tan_half_y, cam.tanX = o.tan_half_x;
    if (o.tan_half_x == 0.f && o.tan_half_y == 0.f) {
        cam.tanY = 0.41421357f;
        cam.tanX = cam.tanY * (cam.Wf / cam.Hf);
    }
    cam.tNear = o.near == 0.f ? h->P.h : o.near;
    cam.tFar = o.far == 0.f ? INFINITY : o.far;
    bool plain;
    if ((rc = cast_path(h, (size_t)cam.width * cam.height, plain))) return rc;
    if ((rc = analysis_grid(h))) return rc;
    CastArgs A{};
    A.m = cam.width * cam.height;
    A.cam = cam;
    A.words = f.packed;
    A.rows = f.count;
    if ((rc = cast_prepare(h, A, o.radius, plain))) return rc;
    ViewShade V{};
    V.shade = o.shade;
    const bool dark = o.light[0] == 0.f && o.light[1] == 0.f && o.light[2] == 0.f;
    const float sun[3] = {-0.35f, 0.8f, 0.5f};
    for (int k = 0; k < 3; ++k) V.light[k] = dark ? sun[k] : o.light[k];
    V.edgeRadius = o.edge_radius == 0.f ? 0.002f * h->P.boxDim : o.edge_radius;
    V.range = f.range;
    const bool autoRange = o.value_lo == 0.f && o.value_hi == 0.f;
    // vel4[cur]: the rows sph_render_field reduces its range over
    rc = frame_finish(h, FrameKind::View, [&] {
        if (o.shade != SPH_VIEW_FLAT)
            sph_launch_field_range(h->vel4[h->cur], h->n, o.shade - SPH_VIEW_FIELD, autoRange, o.value_lo, o.value_hi, f.range, h->compute);
        sph_launch_cast(h->P, A, plain, h->compute);
        sph_launch_view_compose(h->P, A, V, f.rgb, h->compute);
    });
    if (rc) return rc;
    h->castViews += 1;
    cast_account(h, A, plain);
    return SPH_OK;
}

int sph_download_view_buffer(sph_handle *h, uint64_t *words) {
    if (!h || !words) return SPH_EINVAL;
    if (int rc = last_frame_was(h, FrameKind::View)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipMemcpy(words, h->frame.packed, (size_t)h->frame.rp.width * h->frame.rp.height * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SPH_OK;
}

} // extern "C"
