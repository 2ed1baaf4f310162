// C-ABI implementation (include/sph_c_api.h) of the MI355X SPH step path.
// Host logic only; the kernels live in sort.hip / grid.hip / sweeps.hip.
// This unit: settings and initialisers, the handle's life cycle, uploads, downloads and counters; the step is
// in sph_step.hip, the rest in sph_readback / sph_slab / sph_snapshot / sph_frame / sph_sample / sph_surface.hip (shared: sph_handle.h).
// Compile with -ffp-contract=off (host initialisers must round like the
// reference's g++ -O3 x86-64 build, Makefile:22-23).
#include "sph_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sph_host;

namespace {

thread_local std::string g_create_error;

// Largest dist2 for which pressureKernel (dist2 <= h*h) or viscosityKernel
// (sqrtf(dist2) <= h) can be non-zero (simulator.cu:105,125).
float force_cut2(float h) {
    float h2 = h * h;
    float x = h2;
    for (int k = 0; k < 64; ++k) {
        float nx = std::nextafterf(x, INFINITY);
        if (sqrtf(nx) <= h) x = nx;
        else break;
    }
    return x;
}

// every SPH_* knob read at create (the list: sph_handle.h, above Knobs)
Knobs read_knobs() {
    Knobs k;
    if (const char *e = getenv("SPH_SLIM_DIV")) k.slimDiv = atoi(e);
    if (const char *e = getenv("SPH_PIPELINE")) k.pipeline = atoi(e) != 0;
    if (const char *e = getenv("SPH_MASK_POOL_WORDS")) k.maskPoolSet = true, k.maskPoolQuads = strtoull(e, nullptr, 10) / 4;
    if (const char *e = getenv("SPH_ZERO_PAIR_FILTER")) k.zeroPairFilter = atoi(e) != 0;
    if (const char *e = getenv("SPH_PREWARM_COPIES")) k.prewarmCopies = atoi(e);
    if (const char *e = getenv("SPH_TILE_CHUNK")) k.tileChunk = atoi(e); // tuning studies
    if (const char *e = getenv("SPH_XCD_ROTATE")) k.xcdRotate = atoi(e);
    if (const char *e = getenv("SPH_STEP_TRACE")) k.stepTrace = atoi(e) != 0;
    if (const char *e = getenv("SPH_READBACK_SDMA")) k.readbackSdma = atoi(e) != 0;
    return k;
}

void fill_params(sph_handle *h) {
    const SphSettings &s = h->settings;
    DevParams &P = h->P;
    P.h = s.h;
    P.h2 = s.h * s.h;
    P.vcoef = s.v_kernel_coeff;
    P.dcoef = s.d_kernel_coeff;
    P.boxDim = s.boxDim;
    P.boxHi = s.boxDim - s.h;
    P.dt = s.timestep;
    P.cut2 = force_cut2(s.h);
    P.D = (int)s.numCellsPerDim;
    P.morton = h->opt.key_order == SPH_KEY_MORTON ? 1 : 0;
    {
        // The pair body's short divide / square-root chains are proven for the reference's constants
        // only (sweep_common.h): any other h or kernel coefficient selects the full IEEE expansions.
        // SPH_SLIM_DIV=0 forces the full expansions (A/B; same bits).
        SphSettings ref{};
        sph_default_settings(&ref, s.numParticles, s.randomInit);
        P.slimDiv = (s.h == ref.h && s.v_kernel_coeff == ref.v_kernel_coeff && s.d_kernel_coeff == ref.d_kernel_coeff) ? 1 : 0;
        if (h->knobs.slimDiv == 0) P.slimDiv = 0;
    }
    if (P.morton) {
        int b = 0;
        while ((1 << b) < P.D) ++b;
        P.numCells = 1 << (3 * b);
    } else {
        P.numCells = P.D * P.D * P.D;
    }
}

// Simulator::setup's initialisers (simulator.cu:430-453).
int init_positions_reference(const SphSettings &s, float *pos) {
    int n = s.numParticles;
    if (s.randomInit) {
        srand(1); // the state of a process that never called srand (the reference)
        for (int i = 0; i < n; i++) {
            float x = rand() / (float)RAND_MAX * (s.boxDim - 2.f) + 1.f;
            float y = rand() / (float)RAND_MAX * (s.boxDim - 2.f) + 1.f;
            float z = rand() / (float)RAND_MAX * (s.boxDim - 2.f) + 1.f;
            pos[3 * i + 0] = x;
            pos[3 * i + 1] = y;
            pos[3 * i + 2] = z;
        }
        return n;
    }
    float spacing = 0.9f * s.h;
    int nx = (int)(floor((s.boxDim - 2 * s.h) / spacing) + 1);
    int ny = nx, nz = nx;
    int count = 0;
    for (int x = 0; x < nx && count < n; x++)
        for (int y = 0; y < ny && count < n; y++)
            for (int z = 0; z < nz && count < n; z++) {
                pos[3 * count + 0] = s.h + spacing * x;
                pos[3 * count + 1] = s.h + spacing * y;
                pos[3 * count + 2] = s.h + spacing * z;
                count++;
            }
    return count;
}

// Extension for n beyond the reference lattice's 109^3 capacity.
void init_positions_dense(const SphSettings &s, float *pos) {
    int n = s.numParticles;
    int nx = (int)ceil(cbrt((double)n));
    while ((long long)nx * nx * nx < n) nx++;
    while (nx > 1 && (long long)(nx - 1) * (nx - 1) * (nx - 1) >= n) nx--;
    float spacing = nx > 1 ? (s.boxDim - 2 * s.h) / (float)(nx - 1) : 0.f;
    int count = 0;
    for (int x = 0; x < nx && count < n; x++)
        for (int y = 0; y < nx && count < n; y++)
            for (int z = 0; z < nx && count < n; z++) {
                pos[3 * count + 0] = s.h + spacing * x;
                pos[3 * count + 1] = s.h + spacing * y;
                pos[3 * count + 2] = s.h + spacing * z;
                count++;
            }
}

int alloc_device(sph_handle *h) {
    const size_t cap = (size_t)(h->cap > 0 ? h->cap : 1);
    h->external = (h->opt.flags & SPH_FLAG_EXTERNAL_STATE) != 0;
    const size_t posCap = h->external ? 1 : cap; // id-ordered read-back is single-domain only
    for (int b = 0; b < 2; ++b) {
        if (!h->external) {
            HIPCHK(h, h->posBuf[b].alloc(cap));
            HIPCHK(h, h->velBuf[b].alloc(cap));
            h->pos4[b] = h->posBuf[b];
            h->vel4[b] = h->velBuf[b];
            // never hand uninitialised indices to a gather, whatever happens upstream
            HIPCHK(h, hipMemset(h->pos4[b], 0, cap * sizeof(float4)));
            HIPCHK(h, hipMemset(h->vel4[b], 0, cap * sizeof(float4)));
        }
        HIPCHK(h, h->sortKeys[b].alloc(cap));
        HIPCHK(h, h->sortVals[b].alloc(cap));
        h->ws.keys[b] = h->sortKeys[b];
        h->ws.vals[b] = h->sortVals[b];
        if (!(h->opt.flags & SPH_FLAG_MAPPED_POSITIONS)) {
            HIPCHK(h, h->devPosBuf[b].alloc(posCap * 3));
            h->devPos[b] = h->devPosBuf[b];
        }
        HIPCHK(h, hipMemset(h->ws.keys[b], 0, cap * sizeof(uint32_t)));
        HIPCHK(h, hipMemset(h->ws.vals[b], 0, cap * sizeof(uint32_t)));
        HIPCHK(h, h->computeDone[b].create(hipEventDisableTiming));
        HIPCHK(h, h->copyDone[b].create(hipEventDisableTiming));
    }
    h->ws.capacity = (int)cap;
    h->ws.maxBlocks = (int)sph_sort_workspace_blocks((int)cap);
    HIPCHK(h, h->sortBlockHist.alloc((size_t)1024 * (size_t)(h->ws.maxBlocks > 0 ? h->ws.maxBlocks : 1)));
    HIPCHK(h, h->sortDigitTotal.alloc(1024));
    h->ws.blockHist = h->sortBlockHist;
    h->ws.digitTotal = h->sortDigitTotal;
    for (int b = 0; b < 2; ++b) {
        HIPCHK(h, h->cellTable[b].alloc((size_t)h->P.numCells));
        HIPCHK(h, hipMemset(h->cellTable[b], 0, (size_t)h->P.numCells * sizeof(int2)));
    }
    h->cellRange = h->cellTable[0];
    // measured (profiles/r03_experiments.md): n = 262,144: 0.170 -> 0.149 ms per step; n = 4,194,304: nothing
    // (the early steps are bound by the read-back, and beside more GPU work its blit kernel slows down)
    h->aheadEnabled = h->n < (3 << 19);
    if (h->knobs.pipeline >= 0) h->aheadEnabled = h->knobs.pipeline != 0;
    if (h->opt.flags & SPH_FLAG_MAPPED_POSITIONS) {
        // zero-copy: the force sweep's id-ordered scatter goes over PCIe into this buffer
        HIPCHK(h, h->hostPos.alloc(posCap * 3, hipHostMallocMapped));
        void *dp = nullptr;
        HIPCHK(h, hipHostGetDevicePointer(&dp, h->hostPos, 0));
        h->devPos[0] = h->devPos[1] = static_cast<float *>(dp);
        h->mappedPos = true;
    } else {
        // (measured, round 3: a non-coherent buffer changes nothing for the runtime's copy)
        HIPCHK(h, h->hostPos.alloc(posCap * 3));
    }
    memset(h->hostPos, 0, posCap * 3 * sizeof(float));
    if (h->opt.sweep == SPH_SWEEP_LIST) {
        // Hit-stream pool (sweeps_list.hip): a wave reserves Q quads (16 B = two (first
        // candidate, mask) pairs) for each of its 64 lanes, Q = half the largest number
        // of 32-candidate words any of its lanes can fill.  Candidates per particle =
        // 27 x particles per cell (about half the cells of the box hold particles with
        // the reference initialisers) and grow ~4.7x as the fluid settles (measured at
        // n = 4,194,304: 217 at step 1, 1011 at step 100, i.e. 9 -> 36 words per lane
        // plus up to two partly filled words per run).  The pool is sized for 5x the
        // initial fill + the per-run slack, never more than 40 % of the device memory
        // that is free now; a wave that finds it exhausted falls back to testing every
        // candidate again in the force sweep (k_force_fallback: same results, slower).
        const double ppc = (double)cap / (0.5 * (double)h->P.numCells);
        const double wordsPerLane = 5.0 * (27.0 * ppc / 32.0) + 24.0;
        unsigned long long quads = (unsigned long long)((double)cap * wordsPerLane * 0.5 * 1.25);
        if (quads < (1ull << 20)) quads = 1ull << 20;
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
            const unsigned long long lim = (unsigned long long)(0.4 * (double)freeB) / sizeof(uint4);
            if (quads > lim) quads = lim;
        }
        if (h->knobs.maskPoolSet) quads = h->knobs.maskPoolQuads;
        if (quads > 0xFFFFFFF0ull) quads = 0xFFFFFFF0ull; // wave bases are 32-bit quad indices
        h->maskCapacity = quads;
        HIPCHK(h, h->maskPool.alloc((size_t)(quads ? quads : 1) * 4)); // (a quad: four words)
        HIPCHK(h, h->pv8.alloc(cap * 2));
        // per 64-particle wave: {base of its quads or ~0u, quads per lane}
        const size_t hdrWords = 2 * ((cap + 63) / 64 + 1);
        HIPCHK(h, h->maskOff.alloc(hdrWords));
        HIPCHK(h, hipMemset(h->maskOff, 0xFF, hdrWords * sizeof(uint32_t)));
        HIPCHK(h, h->noneList.alloc(hdrWords)); // (>= one entry per wave)
        HIPCHK(h, h->maskCursor.alloc(kCursorBytes / sizeof(unsigned long long)));
        HIPCHK(h, hipMemset(h->maskCursor, 0, kCursorBytes));
        HIPCHK(h, h->hitCount.alloc(cap + 64));
        HIPCHK(h, hipMemset(h->hitCount, 0, (cap + 64) * sizeof(uint32_t)));
        // one bit per sorted row + the word a 32-row window may reach into
        const size_t quietWords = 2 * ((cap + 63) / 64) + 2;
        HIPCHK(h, h->quiet.alloc(quietWords));
        HIPCHK(h, hipMemset(h->quiet, 0, quietWords * sizeof(uint32_t)));
        HIPCHK(h, h->quietVref.alloc(2)); // [0] the reference velocity, [1].x the all-quiet word, [1].y the halo rows'
        HIPCHK(h, hipMemset(h->quietVref, 0, 2 * sizeof(float4)));
        HIPCHK(h, h->calm.alloc((cap + 63) / 64 + 1));
        HIPCHK(h, hipMemset(h->calm, 0, ((cap + 63) / 64 + 1) * sizeof(unsigned long long)));
    }
    HIPCHK(h, h->oobHost.alloc(1, hipHostMallocMapped));
    memset(h->oobHost, 0, sizeof(SphOobLog));
    {
        void *dp = nullptr;
        HIPCHK(h, hipHostGetDevicePointer(&dp, h->oobHost, 0));
        h->ws.oob = static_cast<SphOobLog *>(dp);
    }
    HIPCHK(h, h->boundsDev.alloc(16));
    HIPCHK(h, h->partTiles.alloc(sph_partition_tiles((int)cap) * 9));
    HIPCHK(h, h->boundsHost.alloc(8));
    for (auto &pe : h->pairs) {
        HIPCHK(h, pe.a.create());
        HIPCHK(h, pe.b.create());
    }
    if (h->opt.flags & SPH_FLAG_STORE_FORCE)
        HIPCHK(h, h->force4.alloc(cap));
    HIPCHK(h, h->pairCounter.alloc(kCounterWords));
    HIPCHK(h, hipMemset(h->pairCounter, 0, kCounterWords * sizeof(unsigned long long)));
    HIPCHK(h, h->pairHost.alloc(kCounterWords));
    *h->pairHost = 0;
    for (auto &se : h->ring) {
        for (auto &e : se.e) HIPCHK(h, e.create());
        for (auto &e : se.c) HIPCHK(h, e.create());
    }
    // Read-back pre-warm.  The runtime sets up its device-to-host copy path on the first copies
    // of a process: a one-off ~7 ms stall, which otherwise lands in the first steps of a run
    // (scripts/studies/early_stall.py).  A few small copies through the same stream and buffers here.
    if (h->hostPos && h->devPos[0] && !h->mappedPos) {
        const int warm = h->knobs.prewarmCopies;
        const size_t bytes = std::min<size_t>(posCap * 3 * sizeof(float), (size_t)1 << 20);
        for (int k = 0; k < warm; ++k) {
            HIPCHK(h, hipMemcpyAsync(h->hostPos, h->devPos[k & 1], bytes, hipMemcpyDeviceToHost, h->copy));
            HIPCHK(h, hipStreamSynchronize(h->copy));
        }
        memset(h->hostPos, 0, bytes);
    }
    HIPCHK(h, hipDeviceSynchronize()); // memsets above ran on the null stream
    sdma_init(h);
    return SPH_OK;
}

int upload_common(sph_handle *h, const float *pos, const float *vel, int n) {
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, "");
    if (n != h->n) return fail(h, SPH_EINVAL, "particle count differs from settings");
    const float hh = h->settings.h;
    const int D = h->P.D;
    std::vector<float4> p4((size_t)n), v4((size_t)n);
    int zmin = D, zmax = -1;
    for (int i = 0; i < n; ++i) {
        float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
        // (the range test comes BEFORE the conversion: float -> int of a NaN or of a value beyond INT_MAX is
        // undefined behaviour on the host -- found by the UBSan build under the fuzz tests' NaN upload)
        const float qx = x / hh, qy = y / hh, qz = z / hh, Df = (float)D;
        if (!(qx >= 0.f && qx < Df && qy >= 0.f && qy < Df && qz >= 0.f && qz < Df && x >= 0.f && y >= 0.f && z >= 0.f))
            return fail(h, SPH_EINVAL, "position outside the simulation box");
        const int cz = (int)qz;
        zmin = cz < zmin ? cz : zmin;
        zmax = cz > zmax ? cz : zmax;
        uint32_t id = (uint32_t)i;
        float idbits;
        memcpy(&idbits, &id, 4);
        p4[i] = make_float4(x, y, z, idbits);
        v4[i] = vel ? make_float4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], 0.f)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->cur = 0;
    if (n > 0) {
        int rc = staged_upload(h, h->pos4[0], (size_t)n,
                               [&](size_t k, float4 *dst, size_t cnt) { memcpy(dst, p4.data() + k, cnt * sizeof(float4)); });
        if (!rc)
            rc = staged_upload(h, h->vel4[0], (size_t)n,
                               [&](size_t k, float4 *dst, size_t cnt) { memcpy(dst, v4.data() + k, cnt * sizeof(float4)); });
        if (rc) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    h->zLayers = zmax >= zmin ? zmax - zmin + 1 : 0;
    state_replaced(h);
    // getPosition() right after an upload shows the uploaded state (like setup(): simulator.cu:430-456 fills the
    // host array it hands out)
    h->hostPosIsInit = false;
    if (h->hostPos && n > 0) memcpy(h->hostPos, pos, (size_t)n * 3 * sizeof(float));
    return SPH_OK;
}

} // namespace

namespace sph_host {

int fail(sph_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}

// "this entry point is for the single domain": `hint` ends the message
int reject_slab_mode(sph_handle *h, const char *hint) {
    return fail(h, SPH_ESTATE, std::string("handle is in slab mode (external state)") + hint);
}

} // namespace sph_host

extern "C" {

const char *sph_build_info(void) {
    return "libsph_hip gfx950 (MI355X/CDNA4), api v2, strict-fp32 sweeps, 8/10-bit LSD radix grid build";
}

int sph_default_settings(SphSettings *out, int numParticles, int randomInit) {
    if (!out) return SPH_EINVAL;
    // main.cpp:57-63
    float h = .1f;
    float h_pow_6 = (float)pow((double)h, 6.0);
    float h_pow_9 = (float)pow((double)h, 9.0);
    float v_kernel_coeff = 45.f / (3.14159265f * h_pow_6);
    float d_kernel_coeff = 315.f / (64.f * 3.14159265f * h_pow_9);
    memset(out, 0, sizeof(*out));
    out->randomInit = randomInit ? 1 : 0;
    out->numParticles = numParticles;
    out->h = h;
    out->v_kernel_coeff = v_kernel_coeff;
    out->d_kernel_coeff = d_kernel_coeff;
    out->boxDim = 10.f;
    out->numCellsPerDim = 100;
    out->timestep = (float).01;
    return SPH_OK;
}

int sph_initial_positions(const SphSettings *settings, float *pos_xyz) {
    if (!settings || (!pos_xyz && settings->numParticles > 0) || settings->numParticles < 0)
        return SPH_EINVAL;
    int written = init_positions_reference(*settings, pos_xyz);
    if (written < settings->numParticles) {
        fprintf(stderr,
                "sph: -i grid holds at most %d lattice points in the reference "
                "(simulator.cu:439-452); n=%d uses the dense-lattice EXTENSION\n",
                written, settings->numParticles);
        init_positions_dense(*settings, pos_xyz);
    }
    return SPH_OK;
}

int sph_create(const SphSettings *settings, const SphOptions *options, sph_handle **out) {
    if (!settings || !out) return fail(nullptr, SPH_EINVAL, "null argument");
    *out = nullptr;
    if (settings->numParticles < 0) return fail(nullptr, SPH_EINVAL, "numParticles < 0");
    if (!(settings->h > 0.f) || !(settings->numCellsPerDim >= 1.f) ||
        settings->numCellsPerDim > 1024.f)
        return fail(nullptr, SPH_EINVAL, "bad h / numCellsPerDim");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, SPH_ENODEV,
                    "no HIP device: libsph_hip has no CPU fallback by design");
    sph_handle *h = new (std::nothrow) sph_handle();
    if (!h) return fail(nullptr, SPH_ENOMEM, "out of host memory");
    h->knobs = read_knobs();
    h->settings = *settings;
    if (options) {
        size_t sz = options->struct_size > 0 ? (size_t)options->struct_size : sizeof(SphOptions);
        memcpy(&h->opt, options, sz < sizeof(SphOptions) ? sz : sizeof(SphOptions));
    } else {
        h->opt.device = -1;
    }
    h->opt.struct_size = (int32_t)sizeof(SphOptions);
    const SphOptions &o = h->opt;
    const char *bad = nullptr; // (the first of these that applies)
    if (o.math_mode != SPH_MATH_STRICT && o.math_mode != SPH_MATH_FAST) bad = "unknown math_mode";
    else if (o.sweep < SPH_SWEEP_LIST || o.sweep > SPH_SWEEP_LINKED) bad = "unknown sweep variant";
    else if (o.math_mode == SPH_MATH_FAST && (o.sweep == SPH_SWEEP_DIRECT || o.sweep == SPH_SWEEP_LINKED))
        bad = "SPH_MATH_FAST does not exist for SPH_SWEEP_DIRECT/LINKED";
    else if (o.key_order != SPH_KEY_FLATTENED && o.key_order != SPH_KEY_MORTON) bad = "unknown key_order";
    else if (o.key_order == SPH_KEY_MORTON && (o.sweep != SPH_SWEEP_DIRECT || (o.flags & SPH_FLAG_EXTERNAL_STATE)))
        bad = "SPH_KEY_MORTON is served by SPH_SWEEP_DIRECT, single domain, only";
    else if (o.sweep == SPH_SWEEP_LINKED && (o.flags & SPH_FLAG_EXTERNAL_STATE)) bad = "SPH_SWEEP_LINKED is single-domain only";
    if (bad) {
        delete h;
        return fail(nullptr, SPH_EINVAL, bad);
    }
    h->n = settings->numParticles;
    // a slab handle (caller-owned streams) is sized by its capacity alone: a GPU of an N-GPU run
    // holds ~1/N of the numParticles its settings name
    if ((h->opt.flags & SPH_FLAG_EXTERNAL_STATE) && h->opt.capacity > 0) h->cap = h->opt.capacity;
    else h->cap = h->opt.capacity > h->n ? h->opt.capacity : h->n;
    fill_params(h);
    int rc = SPH_OK;
    do {
        if (h->opt.device >= 0) {
            if (h->opt.device >= count) { rc = fail(nullptr, SPH_EINVAL, "device ordinal out of range"); break; }
            if (hipSetDevice(h->opt.device) != hipSuccess) { rc = fail(nullptr, SPH_EHIP, "hipSetDevice failed"); break; }
        }
        if (hipGetDevice(&h->device) != hipSuccess) { rc = fail(nullptr, SPH_EHIP, "hipGetDevice failed"); break; }
        if (hipStreamCreateWithFlags(&h->compute, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking) != hipSuccess) {
            rc = fail(nullptr, SPH_EHIP, "hipStreamCreate failed");
            break;
        }
        rc = alloc_device(h);
        if (rc) g_create_error = h->err;
    } while (0);
    if (rc) {
        sph_destroy(h);
        return rc;
    }
    *out = h;
    return SPH_OK;
}

void sph_destroy(sph_handle *h) {
    if (!h) return;
    if (h->knobs.stepTrace && h->trSteps > 0)
        fprintf(stderr, "sph step trace (host, us per timed step over %lld steps): enqueue %.1f | wait for the compute stream %.1f | "
                        "after the wait %.1f | caller between two steps %.1f\n", h->trSteps, h->trEnqueue / h->trSteps * 1e6,
                h->trSync / h->trSteps * 1e6, h->trPost / h->trSteps * 1e6, h->trBetween / (h->trSteps > 1 ? h->trSteps - 1 : 1) * 1e6),
        fprintf(stderr, "  enqueue split: events %.1f | grid %.1f | density %.1f | force %.1f | read-back %.1f\n", h->trPh[0] / h->trSteps * 1e6,
                h->trPh[1] / h->trSteps * 1e6, h->trPh[2] / h->trSteps * 1e6, h->trPh[3] / h->trSteps * 1e6, h->trPh[4] / h->trSteps * 1e6);
    if (h->knobs.stepTrace && h->sampleTileCalls + h->samplePlainCalls > 0)
        fprintf(stderr, "sph sample trace: %lld samples by k_sample_tile, %lld by k_sample_plain\n", h->sampleTileCalls, h->samplePlainCalls);
    if (h->knobs.stepTrace && h->surfWaveCalls + h->surfPlainCalls > 0)
        fprintf(stderr, "sph surface trace: %lld extractions by the lane-exchange path, %lld by the plain path\n", h->surfWaveCalls, h->surfPlainCalls);
    if (h->compute) (void)hipStreamSynchronize(h->compute);
    if (h->copy) (void)hipStreamSynchronize(h->copy);
    sdma_destroy(h);
    if (h->ownCompute) h->compute = h->ownCompute;
    const hipStream_t compute = h->compute, copy = h->copy;
    delete h; // every buffer and event, before the streams they were used on
    if (compute) (void)hipStreamDestroy(compute);
    if (copy) (void)hipStreamDestroy(copy);
}

int sph_setup(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    const int n = h->n;
    SPH_ON_DEVICE(h);
    if (h->initPos4 && !h->external) {
        // setup() again on the same handle (bench.py and the tests go back to the initial condition
        // after their warm-up steps): the initial streams are restored from a device-resident copy
        // instead of 12.6 M rand() calls, a validation pass and 134 MB over PCIe -- ~150 ms during
        // which the GPU idles and after which its clocks need ~20 steps to come back
        // (scripts/studies/clock_ramp.py: density sweep 0.63 -> 0.52 -> 0.47 ms over steps 1..40
        // right after an upload, 0.48 flat behind a busy GPU).
        HIPCHK(h, hipStreamSynchronize(h->compute));
        HIPCHK(h, hipStreamSynchronize(h->copy));
        HIPCHK(h, hipMemcpyAsync(h->pos4[0], h->initPos4, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, h->compute));
        HIPCHK(h, hipMemsetAsync(h->vel4[0], 0, (size_t)n * sizeof(float4), h->compute));
        HIPCHK(h, hipStreamSynchronize(h->compute));
        h->zLayers = h->initZLayers;
        state_replaced(h);
        h->hostPosIsInit = true; // (getPosition() before the next step: sph_positions_host copies them then)
        return SPH_OK;
    }
    std::vector<float> pos((size_t)(n > 0 ? n : 1) * 3, 0.f);
    int rc = sph_initial_positions(&h->settings, pos.data());
    if (rc) return fail(h, rc, "sph_initial_positions failed");
    rc = upload_common(h, pos.data(), nullptr, n);
    if (rc || n <= 0 || h->external) return rc;
    // keep the initial streams (best effort: without the copy the next setup() recomputes them)
    if (h->initPos4.alloc((size_t)n) == hipSuccess) {
        if (hipMemcpy(h->initPos4, h->pos4[0], (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice) == hipSuccess) h->initZLayers = h->zLayers;
        else h->initPos4.reset();
    }
    (void)hipGetLastError();
    return SPH_OK;
}

int sph_upload_state(sph_handle *h, const float *pos_xyz, const float *vel_xyz, int n) {
    if (!h || (!pos_xyz && n > 0)) return fail(h, SPH_EINVAL, "null argument");
    return upload_common(h, pos_xyz, vel_xyz, n);
}

int sph_sync(sph_handle *h) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    int rc = sdma_wait(h, 0);
    if (!rc) rc = sdma_wait(h, 1);
    if (rc) return rc;
    report_oob(h);
    return SPH_OK;
}

int sph_num_particles(const sph_handle *h) { return h ? h->n : SPH_EINVAL; }
int sph_num_table_cells(const sph_handle *h) { return h ? h->P.numCells : SPH_EINVAL; }

int sph_download_state(sph_handle *h, float *pos, float *vel, float *rho, float *prs) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h);
    if (!h->ready) return fail(h, SPH_ESTATE, "no state");
    int rc = sph_sync(h);
    if (rc) return rc;
    const int n = h->n;
    std::vector<float4> p4((size_t)(n > 0 ? n : 1)), v4((size_t)(n > 0 ? n : 1));
    if (n > 0) {
        HIPCHK(h, hipMemcpy(p4.data(), h->pos4[h->cur], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(v4.data(), h->vel4[h->cur], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) {
        uint32_t id;
        memcpy(&id, &p4[i].w, 4);
        if (id >= (uint32_t)n) return fail(h, SPH_EHIP, "corrupt particle id in device state");
        if (pos) { pos[3 * id] = p4[i].x; pos[3 * id + 1] = p4[i].y; pos[3 * id + 2] = p4[i].z; }
        if (vel) { vel[3 * id] = v4[i].x; vel[3 * id + 1] = v4[i].y; vel[3 * id + 2] = v4[i].z; }
        float r = v4[i].w;
        if (rho) rho[id] = r;
        // same expression as simulator.cu:188-189
        if (prs) prs[id] = fmaxf(0.f, SPH_GAS_CONSTANT * (r - SPH_REST_DENSITY));
    }
    return SPH_OK;
}

int sph_download_force(sph_handle *h, float *force_xyz) {
    if (!h || !force_xyz) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h);
    if (!h->force4) return fail(h, SPH_ESTATE, "create with SPH_FLAG_STORE_FORCE");
    int rc = sph_sync(h);
    if (rc) return rc;
    const int n = h->n;
    std::vector<float4> f4((size_t)(n > 0 ? n : 1)), p4((size_t)(n > 0 ? n : 1));
    if (n > 0) {
        HIPCHK(h, hipMemcpy(f4.data(), h->force4, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(p4.data(), h->pos4[h->cur], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) {
        uint32_t id;
        memcpy(&id, &p4[i].w, 4);
        if (id >= (uint32_t)n) return fail(h, SPH_EHIP, "corrupt particle id in device state");
        force_xyz[3 * id] = f4[i].x;
        force_xyz[3 * id + 1] = f4[i].y;
        force_xyz[3 * id + 2] = f4[i].z;
    }
    return SPH_OK;
}

int sph_download_grid(sph_handle *h, uint32_t *ids, uint32_t *keys, int32_t *cell_ranges) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h);
    if (!h->gridValid) return fail(h, SPH_ESTATE, "no grid built yet");
    int rc = sph_sync(h);
    if (rc) return rc;
    const int n = h->n;
    if (ids && n > 0) {
        std::vector<float4> p4((size_t)n);
        HIPCHK(h, hipMemcpy(p4.data(), h->pos4[h->sorted], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) memcpy(&ids[i], &p4[i].w, 4);
    }
    if (keys && n > 0)
        HIPCHK(h, hipMemcpy(keys, h->ws.keys[h->sortedKeyBuf], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (cell_ranges)
        HIPCHK(h, hipMemcpy(cell_ranges, h->cellRange, (size_t)h->P.numCells * sizeof(int2), hipMemcpyDeviceToHost));
    return SPH_OK;
}

int sph_get_kernel_times(sph_handle *h, SphKernelTimes *out, int reset) {
    if (!h || !out) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = sph_sync(h);
    if (rc) return rc;
    for (auto &se : h->ring) {
        if (h->gridAhead && &se == h->aheadEv) continue; // a grid built ahead: its step has not run yet
        if ((rc = resolve_events(h, se))) return rc;
    }
    for (auto &pe : h->pairs)
        if ((rc = resolve_pair(h, pe))) return rc;
    if (h->opt.flags & SPH_FLAG_COUNT_PAIRS) {
        HIPCHK(h, hipMemcpy(h->pairHost, h->pairCounter, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        h->kt.pair_tests = h->pairHost[0];
        h->kt.pair_hits = 0;
        h->hitsRecorded = 0;
        for (int sh = 0; sh < 256; ++sh) { // sharded counters (one address would serialise the waves)
            h->kt.pair_tests += h->pairHost[16 + sh * 16];
            h->kt.pair_hits += h->pairHost[16 + sh * 16 + 14];   // bodies evaluated (after the zero-pair filter)
            h->hitsRecorded += h->pairHost[16 + sh * 16 + 15];   // hits in the stream
        }
    }
    *out = h->kt;
    if (reset) {
        h->kt = SphKernelTimes{};
        // (not hipMemset: the first use of the null stream makes the runtime create another
        // hardware queue, and that stalled the GPU's queues for ~7 ms a step or two later)
        HIPCHK(h, hipMemsetAsync(h->pairCounter, 0, kCounterWords * sizeof(unsigned long long), h->compute));
        HIPCHK(h, hipStreamSynchronize(h->compute));
    }
    return SPH_OK;
}

int sph_debug_counters(sph_handle *h, uint64_t *out16) {
    if (!h || !out16) return SPH_EINVAL;
    int rc = sph_sync(h);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(h->pairHost, h->pairCounter, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out16[k] = h->pairHost[k];
    for (int sh = 0; sh < 256; ++sh)
        for (int k = 0; k < 16; ++k) out16[k] += h->pairHost[16 + sh * 16 + k];
    return SPH_OK;
}

int sph_api_version(void) { return SPH_API_VERSION; }

const char *sph_last_error(const sph_handle *h) {
    return h ? h->err.c_str() : g_create_error.c_str();
}

int sph_sort_check(int device, const uint32_t *keys, int n, int key_bits_, uint32_t *perm_out,
                   uint32_t *sorted_keys_out) {
    if (n < 0 || (n > 0 && !keys)) return SPH_EINVAL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SPH_ENODEV;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return SPH_EHIP;
    if (n == 0) return SPH_OK;
    std::vector<uint32_t> iota((size_t)n);
    for (int i = 0; i < n; ++i) iota[i] = (uint32_t)i;
    const size_t nb = sph_sort_workspace_blocks(n);
    DeviceBuf<uint32_t> dk[2], dv[2], blockHist, digitTotal; // (released on every way out)
#define SORT_TRY(call) do { if ((call) != hipSuccess) return SPH_EHIP; } while (0)
    for (int b = 0; b < 2; ++b) {
        SORT_TRY(dk[b].alloc((size_t)n));
        SORT_TRY(dv[b].alloc((size_t)n));
    }
    SORT_TRY(blockHist.alloc(1024 * nb));
    SORT_TRY(digitTotal.alloc(1024));
    SortWorkspace ws{};
    for (int b = 0; b < 2; ++b) {
        ws.keys[b] = dk[b];
        ws.vals[b] = dv[b];
        SORT_TRY(hipMemset(ws.keys[b], 0, (size_t)n * 4));
        SORT_TRY(hipMemset(ws.vals[b], 0, (size_t)n * 4));
    }
    ws.blockHist = blockHist;
    ws.digitTotal = digitTotal;
    ws.capacity = n;
    ws.maxBlocks = (int)nb;
    SORT_TRY(hipMemcpy(ws.keys[0], keys, (size_t)n * 4, hipMemcpyHostToDevice));
    SORT_TRY(hipMemcpy(ws.vals[0], iota.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    const int res = sph_sort_pairs(ws, n, key_bits_, nullptr);
    SORT_TRY(hipDeviceSynchronize());
    if (perm_out) SORT_TRY(hipMemcpy(perm_out, ws.vals[res], (size_t)n * 4, hipMemcpyDeviceToHost));
    if (sorted_keys_out) SORT_TRY(hipMemcpy(sorted_keys_out, ws.keys[res], (size_t)n * 4, hipMemcpyDeviceToHost));
#undef SORT_TRY
    return SPH_OK;
}

} // extern "C"
