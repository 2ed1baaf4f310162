// Ray casting: per ray the nearest entry into a particle's sphere, as the word
// (bits(t) << 32) | id, and the view frame built on it -- the pixel-centre rays of a pinhole camera, then a lit picture
// with the box's edges as cylinders.  Every operation below is fp32 and rounded on its own (-ffp-contract=off), in the
// order that section gives, whatever the handle's math mode.
//
// The ray's word is a minimum over particles, so a kernel may visit the pairs in any order and skip any pair that
// cannot be entered (a2 <= 0).  The default path walks the cell grid along the ray, one lane per ray, layer by layer
// along the ray's dominant axis m: the spheres centred in layer k (cells with index k on axis m) can only be entered
// where the ray's m-coordinate lies in [k h - R, (k + 1) h + R], R = r + pad; the bounding rectangle of that piece of
// the ray in the two other axes, widened by R, holds every such centre.  Layers partition the particles, so nothing is
// tested twice.  The layers are walked in the ray's direction and a lane stops when its best t lies below the t at
// which the ray enters the next WIDENED layer: a sphere centred further on cannot be entered sooner.  pad covers the
// fp32 error of the pair's b2 and t and of the walk's own arithmetic (section 10n derives 2^-17 E, E = max |o_a| + D h,
// for both together) and adds h / 16 on top.  No lane waits for another, every loop is bounded (at most D layers, the
// cells of a rectangle, the rows of a cell), every cell index is clamped into [0, D - 1] before it indexes, and a
// float becomes an int only behind a range test.  No atomics: the two counters leave as one pair of words per wave.
//
// A view gives every wave an 8 x 8 tile of pixels, so that its lanes walk the same cells.
// The check path (SPH_CAST_PLAIN=1): one thread per ray, every row of the stream, nothing shared with the walk.
#include "walk_common.h"

namespace {

constexpr unsigned long long kMiss = SPH_CAST_MISS;

struct Ray {
    float o[3], d[3];
    float tmin, tmax;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; } // (false for a NaN)

__device__ __forceinline__ Ray batch_ray(const SphRay *__restrict__ rays, int g) {
    const float4 *r4 = reinterpret_cast<const float4 *>(rays);
    const float4 a = r4[2 * (size_t)g], b = r4[2 * (size_t)g + 1];
    return {{a.x, a.y, a.z}, {b.x, b.y, b.z}, a.w, b.w};
}

// the ray through the centre of pixel (c, row), row 0 on top
__device__ __forceinline__ Ray view_ray(const ViewCamera &C, int c, int row) {
    const float ax = C.tanX * ((((float)c + 0.5f) / (0.5f * C.Wf)) - 1.f);
    const float ay = C.tanY * ((((float)(C.height - 1 - row) + 0.5f) / (0.5f * C.Hf)) - 1.f);
    Ray q;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q.o[a] = C.eye[a];
        q.d[a] = (C.fwd[a] + ax * C.s[a]) + ay * C.u[a];
    }
    q.tmin = C.tNear;
    q.tmax = C.tFar;
    return q;
}

__device__ __forceinline__ float ray_dd(const Ray &q) { return (q.d[0] * q.d[0] + q.d[1] * q.d[1]) + q.d[2] * q.d[2]; }

__device__ __forceinline__ bool ray_valid(const DevParams &P, const Ray &q, float dd) {
    const float reach = 64.f * ((float)P.D * P.h);
    bool ok = q.tmin >= 0.f && q.tmin <= q.tmax && dd >= 0x1p-40f && dd <= 0x1p40f; // (a NaN fails)
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && finite_f(q.d[a]) && fabsf(q.o[a]) <= reach;
    return ok;
}

// the word of a pair: c = (x, y, z, id)
__device__ __forceinline__ unsigned long long pair_word(const DevParams &P, const Ray &q, float dd, float r2, const float4 c) {
    const float Df = (float)P.D;
    // (point_cell's tests: rows outside the grid sit in clamped cells, where a walk would find them)
    const bool visible = c.x >= 0.f && c.x / P.h < Df && c.y >= 0.f && c.y / P.h < Df && c.z >= 0.f && c.z / P.h < Df;
    const float ex = c.x - q.o[0], ey = c.y - q.o[1], ez = c.z - q.o[2];
    const float b = (ex * q.d[0] + ey * q.d[1]) + ez * q.d[2];
    const float tc = b / dd;
    const float fx = ex - tc * q.d[0], fy = ey - tc * q.d[1], fz = ez - tc * q.d[2];
    const float b2 = (fx * fx + fy * fy) + fz * fz;
    const float a2 = r2 - b2;
    if (!(visible && a2 > 0.f)) return kMiss; // (a NaN is not)
    float t = tc - sqrtf(a2 / dd);
    if (!(t >= q.tmin && t <= q.tmax)) return kMiss;
    t = t == 0.f ? 0.f : t; // -0 is stored as +0
    return ((unsigned long long)__float_as_uint(t) << 32) | __float_as_uint(c.w);
}

// the cells lo .. hi of a stretch [a, b] of coordinates, clamped to the grid; false: the stretch misses the grid
__device__ __forceinline__ bool cell_span(const DevParams &P, float a, float b, int &lo, int &hi) {
    const float Df = (float)P.D, top = (float)(P.D - 1);
    const float fa = a / P.h, fb = b / P.h;
    if (!(fb >= 0.f && fa < Df)) return false; // (a NaN: nothing)
    lo = (int)fminf(fmaxf(fa, 0.f), top);
    hi = (int)fminf(fmaxf(fb, 0.f), top);
    return true;
}

// ray g of the launch: its number in the words, whether it exists, the ray
template <bool kView>
__device__ __forceinline__ Ray wave_ray(const CastArgs &A, int lane, int &g, bool &live) {
    if (kView) {
        const int tilesX = (A.cam.width + 7) >> 3;
        const int c = (blockIdx.x % tilesX) * 8 + (lane & 7), row = (blockIdx.x / tilesX) * 8 + (lane >> 3);
        live = c < A.cam.width && row < A.cam.height;
        g = row * A.cam.width + c;
        return view_ray(A.cam, c, row);
    }
    g = blockIdx.x * 64 + lane;
    live = g < A.m;
    return live ? batch_ray(A.rays, g) : Ray{};
}

template <bool kView>
__global__ __launch_bounds__(64) void k_cast_walk(DevParams P, CastArgs A) {
    const int lane = threadIdx.x;
    int g;
    bool live;
    const Ray q = wave_ray<kView>(A, lane, g, live);
    const float dd = ray_dd(q);
    unsigned long long best = kMiss;
    uint32_t bestRow = 0u;
    unsigned long long layers = 0ull, tests = 0ull;
    if (live && A.S.n > 0 && ray_valid(P, q, dd)) {
        const float adx = fabsf(q.d[0]), ady = fabsf(q.d[1]), adz = fabsf(q.d[2]);
        const int m = (adx >= ady && adx >= adz) ? 0 : (ady >= adz ? 1 : 2);
        // u is the faster key axis of the two others (x unless m is x), v the slower
        const float om = m == 0 ? q.o[0] : m == 1 ? q.o[1] : q.o[2], dm = m == 0 ? q.d[0] : m == 1 ? q.d[1] : q.d[2];
        const float ou = m == 0 ? q.o[1] : q.o[0], du = m == 0 ? q.d[1] : q.d[0];
        const float ov = m == 2 ? q.o[1] : q.o[2], dv = m == 2 ? q.d[1] : q.d[2];
        const int D2 = P.D * P.D;
        const int sm = m == 0 ? 1 : m == 1 ? P.D : D2, su = m == 0 ? P.D : 1, sv = m == 2 ? P.D : D2;
        const float extent = (float)P.D * P.h;
        const float R = A.r + (0.0625f * P.h + 0x1p-17f * (fmaxf(fmaxf(fabsf(q.o[0]), fabsf(q.o[1])), fabsf(q.o[2])) + extent));
        // the layers the ray can reach inside its window, one more on either side (t_max may be +inf)
        const float ma = om + q.tmin * dm, mb = om + q.tmax * dm;
        int k0, k1;
        if (cell_span(P, (fminf(ma, mb) - R) - P.h, (fmaxf(ma, mb) + R) + P.h, k0, k1)) {
            const bool up = dm > 0.f;
            for (int i = 0; i <= k1 - k0; ++i) {
                const int k = up ? k0 + i : k1 - i;
                const float ta = (((float)k * P.h - R) - om) / dm, tb = (((float)(k + 1) * P.h + R) - om) / dm;
                const float tin = fminf(ta, tb), tout = fmaxf(ta, tb);
                if (__uint_as_float((uint32_t)(best >> 32)) < tin) break; // (a miss: the high word is a NaN, never below)
                const float ts = fmaxf(tin, q.tmin), te = fminf(tout, q.tmax);
                if (!(ts <= te)) continue;
                const float ua = ou + ts * du, ub = ou + te * du, va = ov + ts * dv, vb = ov + te * dv;
                int u0, u1, v0, v1;
                if (!cell_span(P, fminf(ua, ub) - R, fmaxf(ua, ub) + R, u0, u1)) continue;
                if (!cell_span(P, fminf(va, vb) - R, fmaxf(va, vb) + R, v0, v1)) continue;
                layers += 1ull;
                for (int cv = v0; cv <= v1; ++cv)
                    for (int cu = u0; cu <= u1; ++cu) {
                        const int2 run = A.S.cellRange[k * sm + cu * su + cv * sv];
                        for (int j = max(run.x, 0); j < min(run.y, A.S.n); ++j) {
                            const unsigned long long w = pair_word(P, q, dd, A.r2, A.S.position(j));
                            tests += 1ull;
                            if (w < best) best = w, bestRow = (uint32_t)j;
                        }
                    }
            }
        }
    }
    if (live) {
        A.words[g] = best;
        if (kView) A.rows[g] = bestRow;
    }
    layers = wave_sum_u64(layers);
    tests = wave_sum_u64(tests);
    if (lane == 0) {
        A.partials[2 * (size_t)blockIdx.x] = layers;
        A.partials[2 * (size_t)blockIdx.x + 1] = tests;
    }
}

// the waves' pairs of words into the two counters: one workgroup, queued behind the walk
__global__ __launch_bounds__(256) void k_cast_count(const unsigned long long *__restrict__ partials, int waves,
                                                    unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long part[2][4];
    unsigned long long layers = 0ull, tests = 0ull;
    for (int w = threadIdx.x; w < waves; w += 256) {
        layers += partials[2 * (size_t)w];
        tests += partials[2 * (size_t)w + 1];
    }
    layers = wave_sum_u64(layers);
    tests = wave_sum_u64(tests);
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = layers, part[1][threadIdx.x >> 6] = tests;
    __syncthreads();
    if (threadIdx.x == 0) {
        counters[0] += (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        counters[1] += (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    }
}

template <bool kView>
__global__ __launch_bounds__(256) void k_cast_plain(DevParams P, CastArgs A) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= A.m) return;
    const Ray q = kView ? view_ray(A.cam, g % A.cam.width, g / A.cam.width) : batch_ray(A.rays, g);
    const float dd = ray_dd(q);
    unsigned long long best = kMiss;
    uint32_t bestRow = 0u;
    if (ray_valid(P, q, dd))
        for (int j = 0; j < A.S.n; ++j) {
            const unsigned long long w = pair_word(P, q, dd, A.r2, A.S.position(j));
            if (w < best) best = w, bestRow = (uint32_t)j;
        }
    A.words[g] = best;
    if (kView) A.rows[g] = bestRow;
}

struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ float dot3(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the smallest entry into one of the box's twelve edges inside the ray's window, +inf where there is none: the
// sphere formula in the two axes across the edge
__device__ __forceinline__ float edge_entry(const Ray &q, float box, float rho) {
    const float rho2 = rho * rho;
    float least = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
        const float dd2 = q.d[b] * q.d[b] + q.d[c] * q.d[c];
        if (!(dd2 > 0.f)) continue;
#pragma unroll
        for (int corner = 0; corner < 4; ++corner) {
            const float eb = ((corner & 1) ? box : 0.f) - q.o[b], ec = ((corner & 2) ? box : 0.f) - q.o[c];
            const float tc = (eb * q.d[b] + ec * q.d[c]) / dd2;
            const float fb = eb - tc * q.d[b], fc = ec - tc * q.d[c];
            const float a2 = rho2 - (fb * fb + fc * fc);
            if (!(a2 > 0.f)) continue;
            const float te = tc - sqrtf(a2 / dd2);
            const float along = q.o[a] + te * q.d[a];
            if (te >= q.tmin && te <= q.tmax && along >= 0.f && along <= box && te < least) least = te;
        }
    }
    return least;
}

__device__ __forceinline__ uint32_t view_byte(float col) {
    col = col > 0.f ? col : 0.f; // (a NaN: 0)
    col = col < 1.f ? col : 1.f;
    return (uint32_t)(col * 255.f + 0.5f);
}

__global__ __launch_bounds__(256) void k_view_compose(DevParams P, CastArgs A, ViewShade V, uint32_t *__restrict__ rgb) {
    const Vec3 l0 = {V.light[0], V.light[1], V.light[2]};
    const float llen = sqrtf(dot3(l0, l0));
    const Vec3 L = {l0.x / llen, l0.y / llen, l0.z / llen};
    compose_quad(A.m, rgb, [&](int p) -> uint32_t {
        const int row = p / A.cam.width, c = p - row * A.cam.width;
        const Ray q = view_ray(A.cam, c, row);
        const unsigned long long w = A.words[p];
        const bool hit = w != kMiss;
        const float t = __uint_as_float((uint32_t)(w >> 32));
        if (V.edgeRadius >= 0.f) {
            const float te = edge_entry(q, P.boxDim, V.edgeRadius);
            if (te < INFINITY && (!hit || te <= t)) return 0xFFFFFFu;
        }
        if (!hit) return 0u;
        const uint32_t j = A.rows[p];
        const float4 c4 = A.S.position((int)j);
        const Vec3 n0 = {(q.o[0] + t * q.d[0]) - c4.x, (q.o[1] + t * q.d[1]) - c4.y, (q.o[2] + t * q.d[2]) - c4.z};
        const float len2 = dot3(n0, n0);
        Vec3 N = {-A.cam.fwd[0], -A.cam.fwd[1], -A.cam.fwd[2]};
        if (len2 > 0.f) { // (a NaN is not)
            const float len = sqrtf(len2);
            N = {n0.x / len, n0.y / len, n0.z / len};
        }
        const float nl0 = dot3(N, L);
        const float nl = nl0 > 0.f ? nl0 : 0.f;
        const float lit = 0.25f + 0.75f * nl;
        float base[3] = {0.1f, 0.35f, 0.9f};
        if (V.shade != SPH_VIEW_FLAT) {
            const float s = __uint_as_float(field_bits(A.S.velocity((int)j), V.shade - SPH_VIEW_FIELD));
            const uint32_t ramp = field_ramp(field_quantise(s, __uint_as_float(V.range[0]), __uint_as_float(V.range[1])));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) base[ch] = (float)((ramp >> (8 * ch)) & 0xFFu) / 255.f;
        }
        uint32_t out = 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out |= view_byte(base[ch] * lit) << (8 * ch);
        return out;
    });
}

} // namespace

int sph_cast_waves(const CastArgs &A) {
    if (A.rays) return (A.m + 63) / 64;
    return ((A.cam.width + 7) / 8) * ((A.cam.height + 7) / 8);
}

void sph_launch_cast(const DevParams &P, const CastArgs &A, bool plain, hipStream_t s) {
    if (A.m <= 0) return;
    const bool view = A.rays == nullptr;
    if (plain) {
        const int blocks = (A.m + 255) / 256;
        if (view) k_cast_plain<true><<<blocks, 256, 0, s>>>(P, A);
        else k_cast_plain<false><<<blocks, 256, 0, s>>>(P, A);
        return;
    }
    const int waves = sph_cast_waves(A); // <= 2^18
    if (view) k_cast_walk<true><<<waves, 64, 0, s>>>(P, A);
    else k_cast_walk<false><<<waves, 64, 0, s>>>(P, A);
    k_cast_count<<<1, 256, 0, s>>>(A.partials, waves, A.counters);
}

void sph_launch_view_compose(const DevParams &P, const CastArgs &A, const ViewShade &V, uint32_t *rgb, hipStream_t s) {
    k_view_compose<<<((A.m + 3) / 4 + 255) / 256, 256, 0, s>>>(P, A, V, rgb);
}
