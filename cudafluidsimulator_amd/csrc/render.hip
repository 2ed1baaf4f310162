// The visualiser's frames (display.cpp:35-90), drawn on the device: clear, splat, compose and the one-off box-edge
// layer.  The images are defined exactly in DESIGN.md sections 10, 10a and 10h; every operation below is fp32 and
// rounded on its own (-ffp-contract=off), in the order those sections give.
//
// The splat is a scatter with heavy contention: at 800 x 600 every particle covers 9 pixels of a
// 400 x 300 region, ~300 hits per pixel at n = 4 M and thousands on the rows the floor pile projects
// to.  The stream it reads is cell-sorted, so the 1024 consecutive particles of a workgroup cover a
// small screen rectangle: the workgroup accumulates them in an LDS tile over that rectangle (LDS
// atomics) and sends ONE global atomic per touched pixel and buffer.  A workgroup whose rectangle
// does not fit the tile (unsorted state right after an upload, very large images) issues the plain
// per-hit global atomics instead.  Minimum and sum commute, so every path gives the same buffers.
// That scheme is written once (k_frame_tile, k_frame_plain) over a frame policy: SplatFrame, the squares of the flat
// and field frames, ColumnFrame (section 10h), footprints that vary with depth and a 64-bit integer sum per pixel, and
// SphereFrame (section 10i), the same footprints with the minimum of a ray-sphere entry depth per pixel.
#include "sph_c_api.h"
#include "sph_device.h"

namespace {

constexpr int kSplatThreads = 256;
constexpr int kSplatPerThread = 4;
constexpr int kSplatBlock = kSplatThreads * kSplatPerThread; // particles per workgroup
constexpr int kTilePixels = 8192;                            // 64 KB of LDS (flat, column) or 96 KB (field)

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

// ---- the splat of the flat and field frames, once for two payloads ----
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
    Word *least; // depth
    __device__ __forceinline__ Word word(uint32_t wbits, int) const { return wbits; }
};

struct FieldPayload {
    using Word = unsigned long long;
    static constexpr Word kEmpty = 0xFFFFFFFFFFFFFFFFull;
    Word *least; // packed
    const float4 *vel4;
    int field;
    __device__ __forceinline__ Word word(uint32_t wbits, int i) const { return field_word(wbits, field_bits(vel4[i], field)); }
};

// One clear for the three frames.  Per pixel: `least` (flat: the depth words) and `wide` (field: the packed words,
// column: the sums) are set to `empty`, `count` to 0, each where given.  range[0] / range[1] (field): the bits of lo / hi
// compose will read -- the fixed range, or the identities of the reduction; *maxWord (column): 0
__global__ __launch_bounds__(256) void k_frame_clear(uint32_t *__restrict__ least, unsigned long long *__restrict__ wide,
                                                     unsigned long long empty, uint32_t *__restrict__ count, int npix,
                                                     uint32_t *__restrict__ range, uint32_t lo, uint32_t hi,
                                                     unsigned long long *__restrict__ maxWord) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npix) {
        if (least) least[i] = (uint32_t)empty;
        if (wide) wide[i] = empty;
        if (count) count[i] = 0u;
    }
    if (i == 0) {
        if (range) {
            range[0] = lo;
            range[1] = hi;
        }
        if (maxWord) *maxWord = 0ull;
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

// A frame policy is what k_frame_tile / k_frame_plain need of a frame: the item of a row (one that covers nothing for
// a row off screen), its pixel box, the hit loop of an item into a target -- the global buffers (0, 0, width), or the
// workgroup's tile over the rectangle that starts at (x0, y0) and is `pitch` wide --, clear / touched / flush for one
// tile entry, and the check path's row.  kMargin: the hull of the boxes still has to be widened by the radius and clipped.
template <class Pay>
struct SplatFrame {
    using Word = typename Pay::Word;
    static constexpr int kNowhere = -0x40000000; // px of no particle, or of one whose square misses the viewport: covers nothing
    static constexpr bool kMargin = true;        // the boxes are the particles' centres
    struct Item {
        int px, py;
        Word word;
    };
    struct Target {
        uint32_t *count;
        Word *least;
    };
    struct Tile {
        Word least[kTilePixels];
        uint32_t count[kTilePixels];
        __device__ __forceinline__ Target target() { return {count, least}; }
    };
    Pay pay;
    uint32_t *count;

    __device__ __forceinline__ Target global() const { return {count, pay.least}; }
    __device__ __forceinline__ Item none() const { return {kNowhere, kNowhere, Pay::kEmpty}; }
    __device__ __forceinline__ Item item(const float4 p, int i, const RenderParams &R) const {
        const Pixel q = project(p.x, p.y, p.z, R);
        const int r = R.radius;
        Item it = none();
        // a centre whose square misses the viewport draws nothing and must not stretch the rectangle
        if (q.px + r >= 0 && q.px - r < R.width && q.py + r >= 0 && q.py - r < R.height) it = {q.px, q.py, pay.word(q.wbits, i)};
        return it;
    }
    __device__ __forceinline__ bool box(const Item &q, int &x0, int &y0, int &x1, int &y1) const {
        x0 = x1 = q.px;
        y0 = y1 = q.py;
        return q.px != kNowhere;
    }
    __device__ __forceinline__ void hits(const Item &q, const RenderParams &R, Target T, int x0, int y0, int pitch) const {
        if (q.px != kNowhere) splat_hits(R, q.px, q.py, q.word, T.count, T.least, x0, y0, pitch);
    }
    // the check path's row: no test against the viewport beside the clipping of the hit loop itself
    __device__ __forceinline__ void plain(const float4 p, int i, const RenderParams &R) const {
        const Pixel q = project(p.x, p.y, p.z, R);
        splat_hits(R, q.px, q.py, pay.word(q.wbits, i), count, pay.least, 0, 0, R.width);
    }
    __device__ __forceinline__ void clear(Target T, int e) const {
        T.count[e] = 0u;
        T.least[e] = Pay::kEmpty;
    }
    __device__ __forceinline__ bool touched(Target T, int e) const { return T.count[e] != 0u; }
    __device__ __forceinline__ void flush(Target T, int e, int g) const {
        atomicAdd(&count[g], T.count[e]);
        // The word only ever decreases during the splat, so whatever value a plain (aligned, single) load returns,
        // however stale, is >= the final one: if it is already <= ours, ours cannot change the result.
        const Word m = T.least[e];
        if (pay.least[g] > m) atomicMin(&pay.least[g], m);
    }
};

// Both kernels take a policy's two members -- its parameters and its global buffer -- as kernel arguments of their own
// and put the policy together again: the fields of one by-value argument are loaded where they are first used, which in
// the tile kernel is behind the barriers (the column frame: +1 %).
// The check path (SPH_RENDER_PLAIN=1): one thread per particle, one global atomic per hit and buffer
template <class Frame, class Part, class Word>
__global__ __launch_bounds__(256) void k_frame_plain(const float4 *__restrict__ pos4, int n, RenderParams R, Part part,
                                                     Word *__restrict__ buffer) {
    const Frame F{part, buffer};
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    F.plain(pos4[i], i, R);
}

template <class Frame, class Part, class Word>
__global__ __launch_bounds__(kSplatThreads) void k_frame_tile(const float4 *__restrict__ pos4, int n, RenderParams R, Part part,
                                                              Word *__restrict__ buffer) {
    const Frame F{part, buffer};
    __shared__ typename Frame::Tile tile;
    __shared__ int box[4]; // min x, min y, max x, max y over the boxes of the workgroup's items
    const int t = threadIdx.x;
    const int base = blockIdx.x * kSplatBlock;
    if (t < 2) box[t] = 0x7fffffff;
    else if (t < 4) box[t] = -0x7fffffff;

    typename Frame::Item q[kSplatPerThread];
    int lox = 0x7fffffff, loy = 0x7fffffff, hix = -0x7fffffff, hiy = -0x7fffffff;
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k) {
        const int i = base + k * kSplatThreads + t;
        q[k] = F.none();
        if (i < n) q[k] = F.item(pos4[i], i, R);
        int bx0, by0, bx1, by1;
        if (F.box(q[k], bx0, by0, bx1, by1)) {
            lox = min(lox, bx0);
            hix = max(hix, bx1);
            loy = min(loy, by0);
            hiy = max(hiy, by1);
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
    int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    if (Frame::kMargin) { // (a hull of footprints is clipped already)
        x0 = max(x0 - R.radius, 0), y0 = max(y0 - R.radius, 0);
        x1 = min(x1 + R.radius, R.width - 1), y1 = min(y1 + R.radius, R.height - 1);
    }
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    const long long area = (long long)bw * bh;

    if (area > kTilePixels) { // (uniform) the rectangle does not fit: per-hit global atomics
#pragma unroll
        for (int k = 0; k < kSplatPerThread; ++k) F.hits(q[k], R, F.global(), 0, 0, R.width);
        return;
    }

    const auto T = tile.target();
    const int entries = (int)area;
    for (int e = t; e < entries; e += kSplatThreads) F.clear(T, e);
    __syncthreads();
    // (every hit of an item lies inside its box, widened by the margin: inside [x0, x1] x [y0, y1] by construction)
#pragma unroll
    for (int k = 0; k < kSplatPerThread; ++k) F.hits(q[k], R, T, x0, y0, bw);
    __syncthreads();
    for (int e = t; e < entries; e += kSplatThreads) {
        if (!F.touched(T, e)) continue;
        const int ey = e / bw;
        F.flush(T, e, (y0 + ey) * R.width + x0 + (e - ey * bw));
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

// The range reductions.  block_fold: v over the workgroup -- wave64 shuffles, then one LDS step across the four waves --
// for thread 0; one call per instantiation and kernel (nothing keeps a second call's writes to `part` behind this one's
// reads).  settle: that value into *word with at most one atomic per workgroup: *word only moves one way while
// the kernel runs, so a plain load that already is past ours, however stale, settles it.
template <bool kMax, class T>
__device__ __forceinline__ T block_fold(T v) {
    __shared__ T part[4];
    auto pick = [](T a, T b) { return kMax ? max(a, b) : min(a, b); };
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = pick(v, (T)__shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return pick(pick(part[0], part[1]), pick(part[2], part[3]));
}
template <bool kMax, class T>
__device__ __forceinline__ void settle(T *word, T v) {
    if (kMax ? *word < v : *word > v) kMax ? atomicMax(word, v) : atomicMin(word, v);
}

// automatic range: minimum and maximum of the bit patterns of s over ALL n rows (s >= +0: bit order = value order)
__global__ __launch_bounds__(256) void k_field_range(const float4 *__restrict__ vel4, int n, int field,
                                                     uint32_t *__restrict__ range) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t b = field_bits(vel4[i], field);
        lo = min(lo, b);
        hi = max(hi, b);
    }
    lo = block_fold<false>(lo);
    hi = block_fold<true>(hi);
    if (threadIdx.x == 0) {
        settle<false>(&range[0], lo);
        settle<true>(&range[1], hi);
    }
}

// (field_ramp, field_quantise: sph_device.h)
__device__ __forceinline__ uint32_t field_rgb(unsigned long long m, uint32_t c, uint32_t e, float lo, float hi) {
    const uint32_t d = (uint32_t)(m >> 32);
    if (e != 0xFFFFFFFFu && e <= d) return 0xFFFFFFu; // GL_LESS, lines drawn first
    if (c == 0u) return 0u;
    return field_ramp(field_quantise(__uint_as_float((uint32_t)m), lo, hi));
}

// (compose_quad: sph_device.h)
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

struct ColumnFrame {
    static constexpr bool kMargin = false; // the boxes are the footprints, clipped already
    using Item = Footprint;
    using Target = unsigned long long *;
    struct Tile {
        unsigned long long sum[kTilePixels];
        __device__ __forceinline__ Target target() { return sum; }
    };
    ColumnParams C;
    unsigned long long *column;

    __device__ __forceinline__ Target global() const { return column; }
    __device__ __forceinline__ Item none() const {
        Footprint f;
        f.c0 = f.r0 = 0;
        f.c1 = f.r1 = -1;
        return f;
    }
    __device__ __forceinline__ Item item(const float4 p, int, const RenderParams &R) const { return column_footprint(p, R, C.h); }
    __device__ __forceinline__ bool box(const Item &f, int &x0, int &y0, int &x1, int &y1) const {
        x0 = f.c0, y0 = f.r0, x1 = f.c1, y1 = f.r1;
        return f.c1 >= f.c0;
    }
    __device__ __forceinline__ void hits(const Item &f, const RenderParams &R, Target T, int x0, int y0, int pitch) const {
        column_hits(f, R, C, [&](int c, int r, unsigned long long q) { atomicAdd(&T[(r - y0) * pitch + (c - x0)], q); });
    }
    __device__ __forceinline__ void plain(const float4 p, int i, const RenderParams &R) const { hits(item(p, i, R), R, column, 0, 0, R.width); }
    __device__ __forceinline__ void clear(Target T, int e) const { T[e] = 0ull; }
    __device__ __forceinline__ bool touched(Target T, int e) const { return T[e] != 0ull; }
    __device__ __forceinline__ void flush(Target T, int e, int g) const { atomicAdd(&column[g], T[e]); }
};

// automatic range: the largest column word (the value is monotonic in the word)
__global__ __launch_bounds__(256) void k_column_max(const unsigned long long *__restrict__ column, int npix,
                                                    unsigned long long *__restrict__ maxWord) {
    unsigned long long hi = 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) hi = max(hi, column[i]);
    hi = block_fold<true>(hi);
    if (threadIdx.x == 0) settle<true>(maxWord, hi);
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

// ---- the liquid frame: front surface, smoothing, normals, a lit picture ----
// Every particle is a sphere of radius r <= h.  On the ray of a pixel the sphere is entered at depth
// wf = (w + t inv) - sqrtf(a2 inv), a2 = r r - b2 > 0: closest approach minus half the chord, from the quantities of
// the column frame's test.  The front buffer keeps the minimum of the bits of wf >= 1 (the near plane) per pixel: a
// minimum of positive floats' bits, so tile, fallback and check path agree like the flat frame's.

struct SphereParams {
    float r, r2;
    const float *rays; // k_column_rays' table
};

struct SphereFrame {
    static constexpr bool kMargin = false; // the boxes are the footprints, clipped already
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    using Item = Footprint;
    using Target = uint32_t *;
    struct Tile {
        uint32_t least[kTilePixels];
        __device__ __forceinline__ Target target() { return least; }
    };
    SphereParams S;
    uint32_t *front;

    __device__ __forceinline__ Target global() const { return front; }
    __device__ __forceinline__ Item none() const {
        Footprint f;
        f.c0 = f.r0 = 0;
        f.c1 = f.r1 = -1;
        return f;
    }
    // (a2 > 0 needs b < r: the column frame's bound with r in the place of h)
    __device__ __forceinline__ Item item(const float4 p, int, const RenderParams &R) const { return column_footprint(p, R, S.r); }
    __device__ __forceinline__ bool box(const Item &f, int &x0, int &y0, int &x1, int &y1) const {
        x0 = f.c0, y0 = f.r0, x1 = f.c1, y1 = f.r1;
        return f.c1 >= f.c0;
    }
    // (column_hits' loop with t and inv kept for the depth; written out here so that the column frame's own kernels
    // compile from the lines they always did)
    __device__ __forceinline__ void hits(const Item &f, const RenderParams &R, Target T, int x0, int y0, int pitch) const {
        for (int r = f.r0; r <= f.r1; ++r) {
            const float ay = S.rays[R.width + r];
            const float ey = f.Y - ay * f.w;
            for (int c = f.c0; c <= f.c1; ++c) {
                const float ax = S.rays[c];
                const float inv = 1.f / ((1.f + ax * ax) + ay * ay);
                const float ex = f.X - ax * f.w;
                const float t = ex * ax + ey * ay;
                const float b2 = (ex * ex + ey * ey) - (t * t) * inv;
                const float a2 = S.r2 - b2;
                if (a2 > 0.f) { // (a NaN is not)
                    const float wf = (f.w + t * inv) - sqrtf(a2 * inv);
                    if (wf >= 1.f) atomicMin(&T[(r - y0) * pitch + (c - x0)], __float_as_uint(wf)); // (a NaN is not)
                }
            }
        }
    }
    __device__ __forceinline__ void plain(const float4 p, int i, const RenderParams &R) const { hits(item(p, i, R), R, front, 0, 0, R.width); }
    __device__ __forceinline__ void clear(Target T, int e) const { T[e] = kEmpty; }
    __device__ __forceinline__ bool touched(Target T, int e) const { return T[e] != kEmpty; }
    __device__ __forceinline__ void flush(Target T, int e, int g) const {
        const uint32_t m = T[e]; // (the flat frame's rule: a plain load that already shows a nearer word settles it)
        if (front[g] > m) atomicMin(&front[g], m);
    }
};

// One smoothing iteration: out = the bilateral filter of `in` (both: the bits of a depth per pixel, 0xFFFFFFFF =
// empty).  A workgroup owns kSmoothW x kSmoothH output pixels, one wave per row, and stages them with a halo of k
// into LDS once; pixels of the halo outside the viewport are staged as empty.  Every read of the window then has the
// 64 lanes of a wave on 64 consecutive dwords of one LDS row: lanes l and l + 32 share a bank, which is free, and no
// two lanes of a 32-lane half do, whatever the pitch 64 + 2k.
constexpr int kSmoothW = 64, kSmoothH = 4, kSmoothMaxRadius = 7;
constexpr uint32_t kNoDepth = 0xFFFFFFFFu;

__global__ __launch_bounds__(kSmoothW * kSmoothH) void k_liquid_smooth(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                                      int width, int height, int k, float delta) {
    __shared__ uint32_t win[(kSmoothW + 2 * kSmoothMaxRadius) * (kSmoothH + 2 * kSmoothMaxRadius)];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * kSmoothW, y0 = blockIdx.y * kSmoothH;
    const int lw = kSmoothW + 2 * k, lh = kSmoothH + 2 * k;
    for (int e = t; e < lw * lh; e += kSmoothW * kSmoothH) {
        const int ly = e / lw, lx = e - ly * lw;
        const int gx = x0 - k + lx, gy = y0 - k + ly;
        win[e] = (gx >= 0 && gx < width && gy >= 0 && gy < height) ? in[(size_t)gy * width + gx] : kNoDepth;
    }
    __syncthreads();
    const int lx = t & (kSmoothW - 1), ly = t / kSmoothW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= width || y >= height) return;
    const uint32_t *centre = &win[(ly + k) * lw + (lx + k)];
    const uint32_t zb = *centre;
    uint32_t result = zb;
    if (zb != kNoDepth) {
        const float zp = __uint_as_float(zb);
        const float norm = (float)(2 * k * k + 1);
        float num = 0.f, den = 1.f;
        for (int dy = -k; dy <= k; ++dy)
            for (int dx = -k; dx <= k; ++dx) {
                const uint32_t qb = centre[dy * lw + dx];
                if (qb == kNoDepth || (dx == 0 && dy == 0)) continue;
                const float d = __uint_as_float(qb) - zp;
                const float u = d / delta;
                const float g = 1.f - u * u;
                if (g > 0.f) { // (a NaN is not)
                    const float s = 1.f - (float)(dx * dx + dy * dy) / norm;
                    const float wgt = (s * s) * (g * g);
                    num = num + wgt * d;
                    den = den + wgt;
                }
            }
        result = __float_as_uint(zp + num / den);
    }
    out[(size_t)y * width + x] = result;
}

struct LiquidShade {
    float light[3];  // as given (compose normalises it)
    float thickness; // s_ref, used where maxWord is null
};

struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ float dot3(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Vec3 over_length(Vec3 a) {
    const float len = sqrtf(dot3(a, a));
    return {a.x / len, a.y / len, a.z / len};
}
__device__ __forceinline__ float at_least_zero(float v) { return v > 0.f ? v : 0.f; } // (a NaN: 0)

// the tangent along one screen axis at a pixel with view-space point P: `ahead` / `behind` are the neighbours' points
// in the forward and backward direction (valid: inside the viewport and non-empty)
__device__ __forceinline__ Vec3 liquid_tangent(Vec3 P, bool fwdOk, Vec3 ahead, bool backOk, Vec3 behind, Vec3 none) {
    const Vec3 fwd = {ahead.x - P.x, ahead.y - P.y, ahead.z - P.z};
    const Vec3 back = {P.x - behind.x, P.y - behind.y, P.z - behind.z};
    if (fwdOk && backOk) return fabsf(back.z) < fabsf(fwd.z) ? back : fwd; // (forward on a tie)
    if (fwdOk) return fwd;
    if (backOk) return back;
    return none;
}

// The lit picture.  depth: the raw front words (the edge test), z: the final smoothed plane, column: the column words;
// maxWord: the reduced largest word of an automatic thickness scale, or null (then S.thickness).  Also leaves the
// unit normal of every pixel in `normals` (w = 0; all zero where the pixel is empty).
__global__ __launch_bounds__(256) void k_liquid_compose(const uint32_t *__restrict__ depth, const uint32_t *__restrict__ z,
                                                        const unsigned long long *__restrict__ column,
                                                        const uint32_t *__restrict__ edge, const float *__restrict__ rays,
                                                        const unsigned long long *__restrict__ maxWord, LiquidShade S, int width,
                                                        int height, float4 *__restrict__ normals, uint32_t *__restrict__ rgb) {
    const float sref = maxWord ? column_value(*maxWord) : S.thickness;
    const Vec3 L = over_length({S.light[0], S.light[1], S.light[2]});
    auto point = [&](int c, int r, bool &ok) -> Vec3 {
        ok = c >= 0 && c < width && r >= 0 && r < height;
        uint32_t b = kNoDepth;
        if (ok) b = z[(size_t)r * width + c];
        ok = b != kNoDepth;
        if (!ok) return {0.f, 0.f, 0.f};
        const float d = __uint_as_float(b);
        return {rays[c] * d, rays[width + r] * d, -d};
    };
    compose_quad(width * height, rgb, [&](int p) -> uint32_t {
        const int r = p / width, c = p - r * width;
        bool here, e, w, n, s;
        const Vec3 P = point(c, r, here);
        const uint32_t eb = edge[p];
        if (!here) {
            normals[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            return eb != 0xFFFFFFFFu ? 0xFFFFFFu : 0u;
        }
        const Vec3 Pe = point(c + 1, r, e), Pw = point(c - 1, r, w), Pn = point(c, r - 1, n), Ps = point(c, r + 1, s);
        const Vec3 Tx = liquid_tangent(P, e, Pe, w, Pw, {1.f, 0.f, 0.f});
        const Vec3 Ty = liquid_tangent(P, n, Pn, s, Ps, {0.f, 1.f, 0.f});
        Vec3 N = {Tx.y * Ty.z - Tx.z * Ty.y, Tx.z * Ty.x - Tx.x * Ty.z, Tx.x * Ty.y - Tx.y * Ty.x};
        const float len2 = dot3(N, N);
        if (len2 > 0.f) { // (a NaN is not)
            const float len = sqrtf(len2);
            N = {N.x / len, N.y / len, N.z / len};
        } else N = {0.f, 0.f, 1.f};
        normals[p] = make_float4(N.x, N.y, N.z, 0.f);
        if (eb != 0xFFFFFFFFu && eb <= depth[p]) return 0xFFFFFFu; // GL_LESS, lines drawn first

        const float ax = rays[c], ay = rays[width + r];
        const float vlen = sqrtf((1.f + ax * ax) + ay * ay);
        const Vec3 V = {-ax / vlen, -ay / vlen, 1.f / vlen};
        const Vec3 Hh = over_length({L.x + V.x, L.y + V.y, L.z + V.z});
        const float nl = at_least_zero(dot3(N, L));
        float spec = at_least_zero(dot3(N, Hh));
#pragma unroll
        for (int k = 0; k < 6; ++k) spec = spec * spec;
        const float f = 1.f - at_least_zero(dot3(N, V));
        const float fres = 0.02f + 0.98f * (((f * f) * (f * f)) * f);
        const float tau = sref == 0.f ? 0.f : column_value(column[p]) / sref;
        const float lit = 0.25f + 0.75f * nl;
        const float kappa[3] = {6.f, 2.f, 0.75f}, sky[3] = {0.75f, 0.85f, 1.f};
        uint32_t out = 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float T = 1.f / (1.f + kappa[ch] * tau);
            float col = ((1.f - fres) * (T * lit) + fres * sky[ch]) + spec;
            col = at_least_zero(col);
            col = col < 1.f ? col : 1.f;
            out |= (uint32_t)(col * 255.f + 0.5f) << (8 * ch);
        }
        return out;
    });
}

template <class Frame>
void launch_splat(const RenderParams &R, const float4 *pos4, int n, bool plain, Frame F, hipStream_t s) {
    if (n <= 0) return;
    const auto [part, buffer] = F;
    if (plain) k_frame_plain<Frame><<<(n + 255) / 256, 256, 0, s>>>(pos4, n, R, part, buffer);
    else k_frame_tile<Frame><<<(n + kSplatBlock - 1) / kSplatBlock, kSplatThreads, 0, s>>>(pos4, n, R, part, buffer);
}

int blocks_of(int items) { return (items + 255) / 256; }

} // namespace

void sph_launch_render_edges(const RenderParams &R, uint32_t *edge, hipStream_t s) {
    const int npix = R.width * R.height;
    (void)hipMemsetAsync(edge, 0xFF, (size_t)npix * sizeof(uint32_t), s);
    k_render_edges<<<(12 * 4096) / 256, 256, 0, s>>>(R, edge);
}

void sph_launch_column_rays(const RenderParams &R, float *rays, hipStream_t s) {
    k_column_rays<<<blocks_of(R.width + R.height), 256, 0, s>>>(R, rays);
}

void sph_launch_render(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain, hipStream_t s) {
    const int npix = R.width * R.height;
    k_frame_clear<<<blocks_of(npix), 256, 0, s>>>(V.depth, nullptr, FlatPayload::kEmpty, V.count, npix, nullptr, 0u, 0u, nullptr);
    launch_splat(R, pos4, n, plain, SplatFrame<FlatPayload>{{V.depth}, V.count}, s);
    k_render_compose<<<blocks_of((npix + 3) / 4), 256, 0, s>>>(V.depth, V.count, V.edge, npix, R.shade, V.rgb);
}

void sph_launch_render_field(const RenderParams &R, const FrameView &V, const float4 *pos4, const float4 *vel4, int n, bool plain,
                             int field, bool autoRange, float lo, float hi, hipStream_t s) {
    const int npix = R.width * R.height;
    const bool reduce = autoRange && n > 0;
    k_frame_clear<<<blocks_of(npix), 256, 0, s>>>(nullptr, V.packed, FieldPayload::kEmpty, V.count, npix, V.range,
                                                  reduce ? 0xFFFFFFFFu : __builtin_bit_cast(uint32_t, lo),
                                                  reduce ? 0u : __builtin_bit_cast(uint32_t, hi), nullptr);
    if (reduce) k_field_range<<<min(blocks_of(n), 1024), 256, 0, s>>>(vel4, n, field, V.range);
    launch_splat(R, pos4, n, plain, SplatFrame<FieldPayload>{{V.packed, vel4, field}, V.count}, s);
    k_field_compose<<<blocks_of((npix + 3) / 4), 256, 0, s>>>(V.packed, V.count, V.edge, V.range, npix, V.depth, V.rgb);
}

void sph_launch_field_range(const float4 *vel4, int n, int field, bool autoRange, float lo, float hi, uint32_t *range, hipStream_t s) {
    const bool reduce = autoRange && n > 0;
    k_frame_clear<<<1, 256, 0, s>>>(nullptr, nullptr, 0ull, nullptr, 0, range, reduce ? 0xFFFFFFFFu : __builtin_bit_cast(uint32_t, lo),
                                    reduce ? 0u : __builtin_bit_cast(uint32_t, hi), nullptr);
    if (reduce) k_field_range<<<min(blocks_of(n), 1024), 256, 0, s>>>(vel4, n, field, range);
}

void sph_launch_render_column(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain, float h, float h2,
                              float dcoef, bool autoRange, float lo, float hi, hipStream_t s) {
    const int npix = R.width * R.height;
    k_frame_clear<<<blocks_of(npix), 256, 0, s>>>(nullptr, V.packed, 0ull, nullptr, npix, nullptr, 0u, 0u, V.maxWord);
    launch_splat(R, pos4, n, plain, ColumnFrame{{h, h2, dcoef, V.rays}, V.packed}, s);
    if (autoRange) k_column_max<<<min(blocks_of(npix), 1024), 256, 0, s>>>(V.packed, npix, V.maxWord);
    k_column_compose<<<blocks_of((npix + 3) / 4), 256, 0, s>>>(V.packed, V.edge, autoRange ? V.maxWord : nullptr, lo, hi, npix,
                                                             V.range, V.rgb);
}

const uint32_t *sph_launch_render_liquid(const RenderParams &R, const FrameView &V, const float4 *pos4, int n, bool plain,
                                         const LiquidParams &Q, hipStream_t s) {
    const int npix = R.width * R.height;
    k_frame_clear<<<blocks_of(npix), 256, 0, s>>>(V.depth, nullptr, SphereFrame::kEmpty, nullptr, npix, nullptr, 0u, 0u, nullptr);
    k_frame_clear<<<blocks_of(npix), 256, 0, s>>>(nullptr, V.packed, 0ull, nullptr, npix, nullptr, 0u, 0u, V.maxWord);
    launch_splat(R, pos4, n, plain, SphereFrame{{Q.radius, Q.radius * Q.radius, V.rays}, V.depth}, s);
    launch_splat(R, pos4, n, plain, ColumnFrame{{Q.h, Q.h2, Q.dcoef, V.rays}, V.packed}, s); // sph_launch_render_column's
    if (Q.autoThickness) k_column_max<<<min(blocks_of(npix), 1024), 256, 0, s>>>(V.packed, npix, V.maxWord);
    const uint32_t *z = V.depth;
    if (Q.smoothRadius > 0) {
        const dim3 grid((R.width + kSmoothW - 1) / kSmoothW, (R.height + kSmoothH - 1) / kSmoothH);
        for (int it = 0; it < Q.smoothIterations; ++it) {
            uint32_t *out = (it & 1) ? V.smooth[1] : V.smooth[0];
            k_liquid_smooth<<<grid, kSmoothW * kSmoothH, 0, s>>>(z, out, R.width, R.height, Q.smoothRadius, Q.smoothDepth);
            z = out;
        }
    }
    const LiquidShade S{{Q.light[0], Q.light[1], Q.light[2]}, Q.thickness};
    k_liquid_compose<<<blocks_of((npix + 3) / 4), 256, 0, s>>>(V.depth, z, V.packed, V.edge, V.rays, Q.autoThickness ? V.maxWord : nullptr, S,
                                                             R.width, R.height, V.normals, V.rgb);
    return z;
}
