// The visualiser's frame (display.cpp:35-90), drawn on the device: clear, splat, compose and the
// one-off box-edge layer.  The image is defined exactly in DESIGN.md section 10; every operation
// below is fp32 and rounded on its own (-ffp-contract=off), in the order that section gives.
//
// The splat is a scatter with heavy contention: at 800 x 600 every particle covers 9 pixels of a
// 400 x 300 region, ~300 hits per pixel at n = 4 M and thousands on the rows the floor pile projects
// to.  The stream it reads is cell-sorted, so the 1024 consecutive particles of a workgroup cover a
// small screen rectangle: the workgroup accumulates them in an LDS tile over that rectangle (LDS
// atomics) and sends ONE global atomic per touched pixel and buffer.  A workgroup whose rectangle
// does not fit the tile (unsorted state right after an upload, very large images) issues the plain
// per-hit global atomics instead.  Minimum and sum commute, so every path gives the same buffers.
// The column frame (section 10h, further down) is the same scheme over footprints that vary with depth, with a
// 64-bit integer sum per pixel.
#include "sph_c_api.h"
#include "sph_device.h"

namespace {

constexpr int kSplatThreads = 256;
constexpr int kSplatPerThread = 4;
constexpr int kSplatBlock = kSplatThreads * kSplatPerThread; // particles per workgroup
constexpr int kTilePixels = 8192;                            // a count and a minimum each: 64 KB (flat) or 96 KB (field) of LDS

struct Pixel {
    int px, py;
    uint32_t wbits;
};

// window coordinates of a point (glFrustum(-2, 2, -2, 2, 1, 100) x glTranslatef(-5, -5, -15), viewport
// W x H): row 0 is the TOP of the window, as in the mouse coordinates of sph_apply_click
__device__ __forceinline__ Pixel project(float x, float y, float z, const RenderParams &R) {
    const float w = 15.f - z;
    const float xw = (((0.5f * (x - 5.f)) / w) + 1.f) * (0.5f * R.Wf);
    const float yw = (((0.5f * (y - 5.f)) / w) + 1.f) * (0.5f * R.Hf);
    Pixel p;
    // (clamped before the conversion: a float beyond the int range must not reach it; anything
    // that far out is outside every viewport either way)
    p.px = (int)fminf(fmaxf(floorf(xw), -65536.f), 65536.f);
    p.py = (R.height - 1) - (int)fminf(fmaxf(floorf(yw), -65536.f), 65536.f);
    p.wbits = __float_as_uint(w);
    return p;
}

// ---- the splat, once for two payloads ----
// The flat frame keeps the minimum of the depth bits per pixel.  The field frame ("The field
// frame") keeps the minimum of (bits(w) << 32) | bits(s), s >= +0 the scalar of the particle's vel4 row (xyz =
// velocity, w = density): the high word IS the depth buffer of the flat frame, the low word the value of the nearest
// particle (the smallest among several at that depth).  A payload gives the per-pixel word, its "empty", the word of
// particle i and the global buffer the minima go to.

// (field_bits, the scalar of a row: sph_device.h)
__device__ __forceinline__ unsigned long long field_word(uint32_t wbits, uint32_t sbits) {
    return ((unsigned long long)wbits << 32) | sbits;
}

struct FlatPayload {
    using Word = uint32_t;
    static constexpr Word kEmpty = 0xFFFFFFFFu;
    static constexpr bool kRange = false;
    Word *least; // depth
    __device__ __forceinline__ Word word(uint32_t wbits, int) const { return wbits; }
};

struct FieldPayload {
    using Word = unsigned long long;
    static constexpr Word kEmpty = 0xFFFFFFFFFFFFFFFFull;
    static constexpr bool kRange = true;
    Word *least; // packed
    const float4 *vel4;
    int field;
    __device__ __forceinline__ Word word(uint32_t wbits, int i) const { return field_word(wbits, field_bits(vel4[i], field)); }
};

// range[0] / range[1] (field frame only): the bits of lo / hi compose will read -- the fixed range, or the identities of the reduction
template <class Pay>
__global__ __launch_bounds__(256) void k_render_clear(typename Pay::Word *__restrict__ least, uint32_t *__restrict__ count, int npix,
                                                      uint32_t *__restrict__ range, uint32_t lo, uint32_t hi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npix) {
        least[i] = Pay::kEmpty;
        count[i] = 0u;
    }
    if (Pay::kRange && i == 0) {
        range[0] = lo;
        range[1] = hi;
    }
}

// one particle's hits: every pixel of its square, clipped to the viewport, counts one more and takes the minimum
// with `word`.  Pixel (x, y) is entry (y - y0) * pitch + (x - x0) of both targets: the global buffers (0, 0, width)
// or a tile over the rectangle that starts at (x0, y0) and is `pitch` wide.
template <class Word>
__device__ __forceinline__ void splat_hits(const RenderParams &R, int px, int py, Word word, uint32_t *count, Word *least,
                                           int x0, int y0, int pitch) {
    const int r = R.radius;
    for (int y = max(py - r, 0); y <= min(py + r, R.height - 1); ++y)
        for (int x = max(px - r, 0); x <= min(px + r, R.width - 1); ++x) {
            const int e = (y - y0) * pitch + (x - x0);
            atomicAdd(&count[e], 1u);
            atomicMin(&least[e], word);
        }
}

// the check path (SPH_RENDER_PLAIN=1): one thread per particle, one atomic per hit and buffer
template <class Pay>
__global__ __launch_bounds__(256) void k_splat_plain(const float4 *__restrict__ pos4, int n, RenderParams R, Pay pay,
                                                     uint32_t *__restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pos4[i];
    const Pixel q = project(p.x, p.y, p.z, R);
    splat_hits(R, q.px, q.py, pay.word(q.wbits, i), count, pay.least, 0, 0, R.width);
}

template <class Pay>
__global__ __launch_bounds__(kSplatThreads) void k_splat_tile(const float4 *__restrict__ pos4, int n, RenderParams R, Pay pay,
                                                              uint32_t *__restrict__ count) {
    using Word = typename Pay::Word;
    constexpr int kNowhere = -0x40000000; // px of no particle, or of one whose square misses the viewport: covers nothing
    __shared__ Word tLeast[kTilePixels];
    __shared__ uint32_t tCount[kTilePixels];
    __shared__ int box[4]; // min x, min y, max x, max y over the workgroup's particle centres
    const int t = threadIdx.x;
    const int base = blockIdx.x * kSplatBlock;
    const int r = R.radius;
    if (t < 2) box[t] = 0x7fffffff;
    else if (t < 4) box[t] = -0x7fffffff;

    int qx[kSplatPerThread], qy[kSplatPerThread];
    Word qw[kSplatPerThread];
    int lox = 0x7fffffff, loy = 0x7fffffff, hix = -0x7fffffff, hiy = -0x7fffffff;
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k) {
        const int i = base + k * kSplatThreads + t;
        qx[k] = qy[k] = kNowhere;
        qw[k] = Pay::kEmpty;
        if (i < n) {
            const float4 p = pos4[i];
            const Pixel q = project(p.x, p.y, p.z, R);
            // a centre whose square misses the viewport draws nothing and must not stretch the rectangle
            if (q.px + r >= 0 && q.px - r < R.width && q.py + r >= 0 && q.py - r < R.height) {
                qx[k] = q.px;
                qy[k] = q.py;
                qw[k] = pay.word(q.wbits, i);
                lox = min(lox, q.px);
                hix = max(hix, q.px);
                loy = min(loy, q.py);
                hiy = max(hiy, q.py);
            }
        }
    }
    lox = wave_min_i32(lox);
    loy = wave_min_i32(loy);
    hix = wave_max_i32(hix);
    hiy = wave_max_i32(hiy);
    __syncthreads();
    if ((t & 63) == 0) {
        atomicMin(&box[0], lox);
        atomicMin(&box[1], loy);
        atomicMax(&box[2], hix);
        atomicMax(&box[3], hiy);
    }
    __syncthreads();
    if (box[2] < box[0]) return; // nothing of this workgroup is on screen (uniform)
    const int x0 = max(box[0] - r, 0), y0 = max(box[1] - r, 0);
    const int x1 = min(box[2] + r, R.width - 1), y1 = min(box[3] + r, R.height - 1);
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    const long long area = (long long)bw * bh;

    if (area > kTilePixels) { // (uniform) the rectangle does not fit: per-hit global atomics
#pragma unroll
        for (int k = 0; k < kSplatPerThread; ++k)
            if (qx[k] != kNowhere) splat_hits(R, qx[k], qy[k], qw[k], count, pay.least, 0, 0, R.width);
        return;
    }

    const int tile = (int)area;
    for (int e = t; e < tile; e += kSplatThreads) {
        tCount[e] = 0u;
        tLeast[e] = Pay::kEmpty;
    }
    __syncthreads();
    // (every pixel of a clipped square lies inside [x0, x1] x [y0, y1] by construction)
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k)
        if (qx[k] != kNowhere) splat_hits(R, qx[k], qy[k], qw[k], tCount, tLeast, x0, y0, bw);
    __syncthreads();
    for (int e = t; e < tile; e += kSplatThreads) {
        const uint32_t c = tCount[e];
        if (c == 0u) continue;
        const int ey = e / bw;
        const int g = (y0 + ey) * R.width + x0 + (e - ey * bw);
        atomicAdd(&count[g], c);
        // The word only ever decreases during the splat, so whatever value a plain (aligned, single) load returns,
        // however stale, is >= the final one: if it is already <= ours, ours cannot change the result.
        const Word m = tLeast[e];
        if (pay.least[g] > m) atomicMin(&pay.least[g], m);
    }
}

// 12 edges x 4096 samples, each a 1-pixel point (built once per handle and image size)
__global__ __launch_bounds__(256) void k_render_edges(RenderParams R, uint32_t *__restrict__ edge) {
    const float V[8][3] = {{0.f, 0.f, 0.f},   {10.f, 0.f, 0.f},   {10.f, 10.f, 0.f},  {0.f, 10.f, 0.f},
                           {0.f, 0.f, 10.f},  {10.f, 0.f, 10.f},  {10.f, 10.f, 10.f}, {0.f, 10.f, 10.f}};
    const int E[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= 12 * 4096) return;
    const int e = gid >> 12, i = gid & 4095;
    const float s = (float)i / 4095.f;
    const float *a = V[E[e][0]], *b = V[E[e][1]];
    const float x = a[0] + s * (b[0] - a[0]);
    const float y = a[1] + s * (b[1] - a[1]);
    const float z = a[2] + s * (b[2] - a[2]);
    const Pixel q = project(x, y, z, R);
    if (q.px < 0 || q.px >= R.width || q.py < 0 || q.py >= R.height) return;
    atomicMin(&edge[q.py * R.width + q.px], q.wbits);
}

__device__ __forceinline__ uint32_t pixel_rgb(uint32_t d, uint32_t c, uint32_t e, int shade) {
    if (e != 0xFFFFFFFFu && e <= d) return 0xFFFFFFu; // GL_LESS, lines drawn first
    if (c == 0u) return 0u;
    if (shade == 0) return 0xFF0000u; // (r, g, b) = bytes 0, 1, 2
    const uint32_t L = min(7u, 31u - (uint32_t)__clz((int)c));
    return (32u * L) | ((32u * L) << 8) | 0xFF0000u;
}

// automatic range: minimum and maximum of the bit patterns of s over ALL n rows (s >= +0: bit order = value order);
// wave64 shuffles, one LDS step across the four waves, then at most one atomic per workgroup and word
__global__ __launch_bounds__(256) void k_field_range(const float4 *__restrict__ vel4, int n, int field,
                                                     uint32_t *__restrict__ range) {
    __shared__ uint32_t wlo[4], whi[4];
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t b = field_bits(vel4[i], field);
        lo = min(lo, b);
        hi = max(hi, b);
    }
    // (the helpers compare signed values: flip the top bit around them)
    lo = (uint32_t)wave_min_i32((int)(lo ^ 0x80000000u)) ^ 0x80000000u;
    hi = (uint32_t)wave_max_i32((int)(hi ^ 0x80000000u)) ^ 0x80000000u;
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = min(min(wlo[0], wlo[1]), min(wlo[2], wlo[3]));
        hi = max(max(whi[0], whi[1]), max(whi[2], whi[3]));
        // (lo only falls and hi only rises: a stale load that already is past ours settles it)
        if (range[0] > lo) atomicMin(&range[0], lo);
        if (range[1] < hi) atomicMax(&range[1], hi);
    }
}

// (r, g, b) = bytes 0, 1, 2: blue - cyan - green - yellow - red over q = 0..255, integers only
__device__ __forceinline__ uint32_t field_ramp(uint32_t q) {
    if (q < 64u) return ((4u * q) << 8) | 0xFF0000u;
    if (q < 128u) return 0x00FF00u | ((255u - 4u * (q - 64u)) << 16);
    if (q < 192u) return (4u * (q - 128u)) | 0x00FF00u;
    return 0xFFu | ((255u - 4u * (q - 192u)) << 8);
}

// the quantiser of the field and column frames: q = 0..255 of s on the scale lo..hi
__device__ __forceinline__ uint32_t field_quantise(float s, float lo, float hi) {
    uint32_t q = 0u;
    if (hi != lo) {
        const float u = ((s - lo) / (hi - lo)) * 256.f;
        if (u == u) q = (uint32_t)(int)fminf(fmaxf(floorf(u), 0.f), 255.f); // (NaN: q = 0)
    }
    return q;
}

__device__ __forceinline__ uint32_t field_rgb(unsigned long long m, uint32_t c, uint32_t e, float lo, float hi) {
    const uint32_t d = (uint32_t)(m >> 32);
    if (e != 0xFFFFFFFFu && e <= d) return 0xFFFFFFu; // GL_LESS, lines drawn first
    if (c == 0u) return 0u;
    return field_ramp(field_quantise(__uint_as_float((uint32_t)m), lo, hi));
}

// four pixels = 12 bytes = three dwords per thread (rgb is padded to a multiple of four pixels); colour(p) = 0xBBGGRR of pixel p
template <class Colour>
__device__ __forceinline__ void compose_quad(int npix, uint32_t *__restrict__ rgb, Colour colour) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int p0 = g * 4;
    if (p0 >= npix) return;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = (p0 + k < npix) ? colour(p0 + k) : 0u;
    rgb[g * 3 + 0] = c[0] | (c[1] << 24);
    rgb[g * 3 + 1] = (c[1] >> 8) | (c[2] << 16);
    rgb[g * 3 + 2] = (c[2] >> 16) | (c[3] << 8);
}

__global__ __launch_bounds__(256) void k_render_compose(const uint32_t *__restrict__ depth, const uint32_t *__restrict__ count,
                                                        const uint32_t *__restrict__ edge, int npix, int shade,
                                                        uint32_t *__restrict__ rgb) {
    compose_quad(npix, rgb, [&](int p) { return pixel_rgb(depth[p], count[p], edge[p], shade); });
}

// also leaves the high words in `depth`, the depth buffer sph_download_frame_buffers serves
__global__ __launch_bounds__(256) void k_field_compose(const unsigned long long *__restrict__ packed,
                                                       const uint32_t *__restrict__ count, const uint32_t *__restrict__ edge,
                                                       const uint32_t *__restrict__ range, int npix,
                                                       uint32_t *__restrict__ depth, uint32_t *__restrict__ rgb) {
    compose_quad(npix, rgb, [&](int p) {
        const unsigned long long m = packed[p];
        depth[p] = (uint32_t)(m >> 32);
        return field_rgb(m, count[p], edge[p], __uint_as_float(range[0]), __uint_as_float(range[1]));
    });
}

// ---- the column frame: per pixel the sum over ALL particles of a 64-bit integer term ----
// Through the centre of pixel (c, r) runs the ray (ax(c), ay(r), -1) from the eye; a particle within h of it adds the
// line integral of its poly6 kernel along the ray, MASS coeff (32/35) a^7, as the integer (uint64)(term 2^32).  Sums of
// integers commute: the tile, its fallback and the check path give the same words, whatever the order of the rows.
//
// Work split: one lane walks the whole footprint of its particle (9 to ~200 pixel tests).  The footprint's size is a
// function of the particle's depth w (and, weakly, of its angle off the axis); in the cell-sorted stream the 64 rows
// of a wave come from one cell or its neighbours in x, so their w differ by about h and their footprints by a pixel:
// the lanes' trip counts agree without splitting particles by footprint row, which would cost each piece the
// per-particle set-up again.  Id-ordered state (right after an upload, SPH_SWEEP_LINKED) diverges; it also misses the
// tile, and is not the case the frame is built for.
//
// ax and ay are read from a table built once per image size (sph_launch_column_rays) with the operations of the
// definition; inv, one IEEE divide, is recomputed per test.

struct ColumnParams {
    float h, h2, dcoef;
    const float *rays; // ax of column c at [c], ay of row r at [width + r]
};

__global__ __launch_bounds__(256) void k_column_rays(RenderParams R, float *__restrict__ rays) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < R.width) rays[i] = 2.f * ((((float)i + 0.5f) / (0.5f * R.Wf)) - 1.f);
    else if (i < R.width + R.height) rays[i] = 2.f * ((((float)(R.height - 1 - (i - R.width)) + 0.5f) / (0.5f * R.Hf)) - 1.f);
}

__global__ __launch_bounds__(256) void k_column_clear(unsigned long long *__restrict__ column, int npix,
                                                      unsigned long long *__restrict__ maxWord) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npix) column[i] = 0ull;
    if (i == 0) *maxWord = 0ull;
}

// the term of a pair with a2 = h h - b2 > 0
__device__ __forceinline__ unsigned long long column_term(float a2, float dcoef) {
    const float c = (SPH_MASS * (((dcoef * a2) * a2) * a2)) * ((32.f / 35.f) * sqrtf(a2));
    if (c >= 1048576.f) return 1ull << 52;
    if (!(c > 0.f)) return 0ull; // NaN, and a negative coefficient
    return (unsigned long long)(c * 4294967296.f);
}

// The pixels a particle can reach, clipped to the viewport (empty: c1 < c0).  On a ray b >= |e| / s, which bounds the
// footprint by 0.25 W h s_p / (w - h) columns and 0.25 H h s_p / (w - h) rows around the particle's own pixel (DESIGN.md
// section 10h); rounded up, plus one for the fp32 evaluation here.  A particle at or behind the eye's h (w <= h) may
// reach every pixel; a non-finite one reaches none (its b2 is NaN or infinite for every ray).
struct Footprint {
    float X, Y, w;
    int c0, c1, r0, r1;
};
__device__ __forceinline__ Footprint column_footprint(const float4 p, const RenderParams &R, float h) {
    Footprint f;
    f.X = p.x - 5.f;
    f.Y = p.y - 5.f;
    f.w = 15.f - p.z;
    f.c0 = f.r0 = 0;
    f.c1 = f.r1 = -1;
    if (!(fabsf(f.X) < INFINITY && fabsf(f.Y) < INFINITY && fabsf(f.w) < INFINITY)) return f;
    f.c1 = R.width - 1;
    f.r1 = R.height - 1;
    const float d = f.w - h;
    if (d > 0.f) {
        const Pixel q = project(p.x, p.y, p.z, R); // (clamped to +-65536)
        const float u = f.X / f.w, v = f.Y / f.w;
        const float k = (h * sqrtf((1.f + u * u) + v * v)) / d;
        // (fminf drops a NaN: the whole viewport then)
        const int hx = (int)fminf(ceilf((0.25f * R.Wf) * k) + 1.f, 131072.f);
        const int hy = (int)fminf(ceilf((0.25f * R.Hf) * k) + 1.f, 131072.f);
        f.c0 = max(q.px - hx, 0);
        f.c1 = min(q.px + hx, R.width - 1);
        f.r0 = max(q.py - hy, 0);
        f.r1 = min(q.py + hy, R.height - 1);
    }
    if (f.r1 < f.r0) f.c1 = f.c0 - 1; // one test for "empty"
    return f;
}

// every pixel of the footprint whose ray passes within h: sink(column, row, term)
template <class Sink>
__device__ __forceinline__ void column_hits(const Footprint &f, const RenderParams &R, const ColumnParams &C, Sink sink) {
    for (int r = f.r0; r <= f.r1; ++r) {
        const float ay = C.rays[R.width + r];
        const float ey = f.Y - ay * f.w;
        for (int c = f.c0; c <= f.c1; ++c) {
            const float ax = C.rays[c];
            const float inv = 1.f / ((1.f + ax * ax) + ay * ay);
            const float ex = f.X - ax * f.w;
            const float t = ex * ax + ey * ay;
            const float b2 = (ex * ex + ey * ey) - (t * t) * inv;
            const float a2 = C.h2 - b2;
            if (a2 > 0.f) { // (a NaN is not)
                const unsigned long long q = column_term(a2, C.dcoef);
                if (q) sink(c, r, q);
            }
        }
    }
}

// the check path (SPH_RENDER_PLAIN=1): one thread per particle, one global atomic per contributing pixel
__global__ __launch_bounds__(256) void k_column_plain(const float4 *__restrict__ pos4, int n, RenderParams R, ColumnParams C,
                                                      unsigned long long *__restrict__ column) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Footprint f = column_footprint(pos4[i], R, C.h);
    column_hits(f, R, C, [&](int c, int r, unsigned long long q) { atomicAdd(&column[r * R.width + c], q); });
}

// k_splat_tile's scheme over the hull of the workgroup's FOOTPRINTS: LDS atomics into a 64 KB tile of 64-bit sums,
// then one global atomic per touched pixel; a hull that does not fit the tile: per-hit global atomics
__global__ __launch_bounds__(kSplatThreads) void k_column_tile(const float4 *__restrict__ pos4, int n, RenderParams R, ColumnParams C,
                                                               unsigned long long *__restrict__ column) {
    __shared__ unsigned long long tile[kTilePixels];
    __shared__ int box[4]; // min column, min row, max column, max row over the workgroup's footprints
    const int t = threadIdx.x;
    const int base = blockIdx.x * kSplatBlock;
    if (t < 2) box[t] = 0x7fffffff;
    else if (t < 4) box[t] = -0x7fffffff;

    Footprint f[kSplatPerThread];
    int lox = 0x7fffffff, loy = 0x7fffffff, hix = -0x7fffffff, hiy = -0x7fffffff;
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k) {
        const int i = base + k * kSplatThreads + t;
        f[k].c0 = f[k].r0 = 0;
        f[k].c1 = f[k].r1 = -1;
        if (i < n) f[k] = column_footprint(pos4[i], R, C.h);
        if (f[k].c1 >= f[k].c0) {
            lox = min(lox, f[k].c0);
            hix = max(hix, f[k].c1);
            loy = min(loy, f[k].r0);
            hiy = max(hiy, f[k].r1);
        }
    }
    lox = wave_min_i32(lox);
    loy = wave_min_i32(loy);
    hix = wave_max_i32(hix);
    hiy = wave_max_i32(hiy);
    __syncthreads();
    if ((t & 63) == 0) {
        atomicMin(&box[0], lox);
        atomicMin(&box[1], loy);
        atomicMax(&box[2], hix);
        atomicMax(&box[3], hiy);
    }
    __syncthreads();
    if (box[2] < box[0]) return; // nothing of this workgroup is on screen (uniform)
    const int x0 = box[0], y0 = box[1];
    const int bw = box[2] - x0 + 1, bh = box[3] - y0 + 1;
    const long long area = (long long)bw * bh;

    if (area > kTilePixels) { // (uniform)
#pragma unroll
        for (int k = 0; k < kSplatPerThread; ++k)
            column_hits(f[k], R, C, [&](int c, int r, unsigned long long q) { atomicAdd(&column[r * R.width + c], q); });
        return;
    }

    const int area32 = (int)area;
    for (int e = t; e < area32; e += kSplatThreads) tile[e] = 0ull;
    __syncthreads();
    // (every footprint lies inside the hull [x0, x0 + bw) x [y0, y0 + bh) by construction)
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k)
        column_hits(f[k], R, C, [&](int c, int r, unsigned long long q) { atomicAdd(&tile[(r - y0) * bw + (c - x0)], q); });
    __syncthreads();
    for (int e = t; e < area32; e += kSplatThreads) {
        const unsigned long long v = tile[e];
        if (v == 0ull) continue;
        const int ey = e / bw;
        atomicAdd(&column[(y0 + ey) * R.width + x0 + (e - ey * bw)], v);
    }
}

// automatic range: the largest column word (the value is monotonic in the word); wave64 shuffles, one LDS step
// across the four waves, then at most one atomic per workgroup
__global__ __launch_bounds__(256) void k_column_max(const unsigned long long *__restrict__ column, int npix,
                                                    unsigned long long *__restrict__ maxWord) {
    __shared__ unsigned long long whi[4];
    unsigned long long hi = 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) hi = max(hi, column[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hi = max(hi, (unsigned long long)__shfl_xor(hi, off));
    if ((threadIdx.x & 63) == 0) whi[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        hi = max(max(whi[0], whi[1]), max(whi[2], whi[3]));
        if (*maxWord < hi) atomicMax(maxWord, hi); // (it only rises: a stale load that already is past ours settles it)
    }
}

// one round-to-nearest-even conversion of the 64-bit word, then an exact scaling by 2^-32
__device__ __forceinline__ float column_value(unsigned long long sum) { return (float)sum * 2.3283064365386963e-10f; }

// maxWord: the reduced maximum of an automatic range (then lo = +0, hi = its value), or null (lo, hi: the options');
// leaves the bits of the range it used in range[0..1]
__global__ __launch_bounds__(256) void k_column_compose(const unsigned long long *__restrict__ column, const uint32_t *__restrict__ edge,
                                                        const unsigned long long *__restrict__ maxWord, float lo, float hi, int npix,
                                                        uint32_t *__restrict__ range, uint32_t *__restrict__ rgb) {
    if (maxWord) {
        lo = 0.f;
        hi = column_value(*maxWord);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        range[0] = __float_as_uint(lo);
        range[1] = __float_as_uint(hi);
    }
    compose_quad(npix, rgb, [&](int p) -> uint32_t {
        if (edge[p] != 0xFFFFFFFFu) return 0xFFFFFFu; // the fluid is translucent: no depth test
        const unsigned long long sum = column[p];
        if (sum == 0ull) return 0u;
        const uint32_t q = field_quantise(column_value(sum), lo, hi);
        return (223u - ((7u * q) >> 3)) | ((239u - ((3u * q) >> 2)) << 8) | ((255u - (q >> 1)) << 16);
    });
}

template <class Pay>
void launch_splat(const RenderParams &R, const float4 *pos4, int n, bool plain, Pay pay, uint32_t *count, hipStream_t s) {
    if (n <= 0) return;
    if (plain) k_splat_plain<<<(n + 255) / 256, 256, 0, s>>>(pos4, n, R, pay, count);
    else k_splat_tile<<<(n + kSplatBlock - 1) / kSplatBlock, kSplatThreads, 0, s>>>(pos4, n, R, pay, count);
}

} // namespace

void sph_launch_render_edges(const RenderParams &R, uint32_t *edge, hipStream_t s) {
    const int npix = R.width * R.height;
    (void)hipMemsetAsync(edge, 0xFF, (size_t)npix * sizeof(uint32_t), s);
    k_render_edges<<<(12 * 4096) / 256, 256, 0, s>>>(R, edge);
}

void sph_launch_render(const RenderParams &R, const float4 *pos4, int n, bool plain, uint32_t *depth, uint32_t *count,
                       const uint32_t *edge, uint32_t *rgb, hipStream_t s) {
    const int npix = R.width * R.height;
    k_render_clear<FlatPayload><<<(npix + 255) / 256, 256, 0, s>>>(depth, count, npix, nullptr, 0u, 0u);
    launch_splat(R, pos4, n, plain, FlatPayload{depth}, count, s);
    const int quads = (npix + 3) / 4;
    k_render_compose<<<(quads + 255) / 256, 256, 0, s>>>(depth, count, edge, npix, R.shade, rgb);
}

void sph_launch_column_rays(const RenderParams &R, float *rays, hipStream_t s) {
    k_column_rays<<<(R.width + R.height + 255) / 256, 256, 0, s>>>(R, rays);
}

void sph_launch_render_column(const RenderParams &R, const float4 *pos4, int n, bool plain, float h, float h2, float dcoef,
                              bool autoRange, float lo, float hi, const float *rays, unsigned long long *column,
                              unsigned long long *maxWord, const uint32_t *edge, uint32_t *range, uint32_t *rgb, hipStream_t s) {
    const int npix = R.width * R.height;
    const ColumnParams C{h, h2, dcoef, rays};
    k_column_clear<<<(npix + 255) / 256, 256, 0, s>>>(column, npix, maxWord);
    if (n > 0) {
        if (plain) k_column_plain<<<(n + 255) / 256, 256, 0, s>>>(pos4, n, R, C, column);
        else k_column_tile<<<(n + kSplatBlock - 1) / kSplatBlock, kSplatThreads, 0, s>>>(pos4, n, R, C, column);
    }
    if (autoRange) k_column_max<<<min((npix + 255) / 256, 1024), 256, 0, s>>>(column, npix, maxWord);
    const int quads = (npix + 3) / 4;
    k_column_compose<<<(quads + 255) / 256, 256, 0, s>>>(column, edge, autoRange ? maxWord : nullptr, lo, hi, npix, range, rgb);
}

void sph_launch_render_field(const RenderParams &R, const float4 *pos4, const float4 *vel4, int n, bool plain, int field,
                            bool autoRange, float lo, float hi, unsigned long long *packed, uint32_t *depth, uint32_t *count,
                            const uint32_t *edge, uint32_t *range, uint32_t *rgb, hipStream_t s) {
    const int npix = R.width * R.height;
    const bool reduce = autoRange && n > 0;
    k_render_clear<FieldPayload><<<(npix + 255) / 256, 256, 0, s>>>(packed, count, npix, range,
                                                                   reduce ? 0xFFFFFFFFu : __builtin_bit_cast(uint32_t, lo),
                                                                   reduce ? 0u : __builtin_bit_cast(uint32_t, hi));
    if (reduce) k_field_range<<<min((n + 255) / 256, 1024), 256, 0, s>>>(vel4, n, field, range);
    launch_splat(R, pos4, n, plain, FieldPayload{packed, vel4, field}, count, s);
    const int quads = (npix + 3) / 4;
    k_field_compose<<<(quads + 255) / 256, 256, 0, s>>>(packed, count, edge, range, npix, depth, rgb);
}
