// `class Simulator` (include/simulator.h) over the C-ABI in sph_c_api.h.
// Mirrors the method semantics of the reference's Simulator
// (simulator.cu:370-546): void methods, caller-owned Settings kept by pointer,
// getPosition() stable for the simulator's lifetime and coherent as soon as
// simulate()/simulateAndTime() has returned.  The reference checks no CUDA
// status; here a failing call aborts with the library's message.
#include "simulator.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "sph_c_api.h"
#include "sph_mgpu.h"

// Defined by the front end (display.cpp:19-20) or by headless.cpp.
extern bool mouseClicked;
extern int2 clickCoords;

static_assert(sizeof(Settings) == sizeof(SphSettings), "Settings layout");
static_assert(offsetof(Settings, numParticles) == offsetof(SphSettings, numParticles), "Settings layout");
static_assert(offsetof(Settings, h) == offsetof(SphSettings, h), "Settings layout");
static_assert(offsetof(Settings, timestep) == offsetof(SphSettings, timestep), "Settings layout");
static_assert(sizeof(Times) == sizeof(SphTimes), "Times layout");
static_assert(offsetof(Times, iters) == offsetof(SphTimes, iters), "Times layout");
static_assert(sizeof(float3) == 12, "float3 must be 12 bytes");

static void check(sph_handle *h, int rc, const char *what) {
    if (rc == SPH_OK) return;
    fprintf(stderr, "sph: %s failed (%d): %s\n", what, rc, sph_last_error(h));
    abort();
}

static void mcheck(sph_mgpu *m, int rc, const char *what) {
    if (rc == SPH_OK) return;
    fprintf(stderr, "sph: %s failed (%d): %s\n", what, rc, sph_mgpu_last_error(m));
    abort();
}

Simulator::Simulator(Settings *settings) : impl(NULL), multi(NULL), settings(settings) {}

Simulator::~Simulator() {
    if (impl) sph_destroy(impl);
    if (multi) sph_mgpu_destroy(multi);
}

void Simulator::setup() {
    if (impl) {
        sph_destroy(impl);
        impl = NULL;
    }
    SphSettings s;
    memcpy(&s, settings, sizeof s);
    s.randomInit = settings->randomInit ? 1 : 0;
    SphOptions o;
    memset(&o, 0, sizeof o);
    o.struct_size = (int32_t)sizeof o;
    o.device = -1;
    if (const char *e = getenv("SPH_SWEEP"))
        o.sweep = strcmp(e, "direct") == 0   ? SPH_SWEEP_DIRECT
                  : strcmp(e, "lds") == 0    ? SPH_SWEEP_LDS
                  : strcmp(e, "linked") == 0 ? SPH_SWEEP_LINKED
                                             : SPH_SWEEP_LIST;
    // SPH_GPUS=N (N > 1): the same step over N z-slabs, one per GPU, halo layers by RCCL
    // send/recv, all driven from this thread (include/sph_mgpu.h).  SPH_TRANSPORT=loopback
    // runs the N slabs on one GPU (rehearsal on a one-GPU machine).
    int gpus = getenv("SPH_GPUS") ? atoi(getenv("SPH_GPUS")) : 1;
    if (multi) {
        sph_mgpu_destroy(multi);
        multi = NULL;
    }
    if (gpus > 1) {
        SphMgpuOptions mo;
        memset(&mo, 0, sizeof mo);
        mo.struct_size = (int32_t)sizeof mo;
        mo.world = gpus;
        mo.rank_begin = 0;
        mo.rank_count = gpus;
        const char *tr = getenv("SPH_TRANSPORT");
        mo.transport = (tr && strcmp(tr, "loopback") == 0) ? SPH_TRANSPORT_LOOPBACK
                       : (tr && strcmp(tr, "rccl_self") == 0) ? SPH_TRANSPORT_RCCL_SELF
                       : (tr && strcmp(tr, "streams") == 0)   ? SPH_TRANSPORT_STREAMS
                                                               : SPH_TRANSPORT_RCCL;
        for (int k = 0; k < SPH_MGPU_MAX_LOCAL; ++k) mo.devices[k] = mo.transport == SPH_TRANSPORT_RCCL ? k : 0;
        mo.sweep = o.sweep;
        if (const char *e = getenv("SPH_RECUT_EVERY")) mo.recut_every = atoi(e);
        int rc = sph_mgpu_create(&s, &mo, NULL, &multi);
        mcheck(NULL, rc, "sph_mgpu_create");
        mcheck(multi, sph_mgpu_setup(multi), "sph_mgpu_setup");
        return;
    }
    int rc = sph_create(&s, &o, &impl);
    check(NULL, rc, "sph_create");
    check(impl, sph_setup(impl), "sph_setup");
}

const float3 *Simulator::getPosition() {
    if (multi) return reinterpret_cast<const float3 *>(sph_mgpu_positions_host(multi));
    if (!impl) return NULL;
    return reinterpret_cast<const float3 *>(sph_positions_host(impl));
}

void Simulator::simulate() {
    if (multi) { // every slab applies the impulse to the layers it owns, after its force sweep
        if (mouseClicked) mcheck(multi, sph_mgpu_queue_click(multi, clickCoords.x, clickCoords.y), "sph_mgpu_queue_click");
        mcheck(multi, sph_mgpu_step(multi, NULL), "sph_mgpu_step");
        mouseClicked = false;
        return;
    }
    check(impl, sph_step(impl, NULL), "sph_step");
    if (mouseClicked) { // simulator.cu:482-489
        check(impl, sph_apply_click(impl, clickCoords.x, clickCoords.y), "sph_apply_click");
        mouseClicked = false;
    }
}

void Simulator::simulateAndTime(Times *times) {
    if (multi) {
        mcheck(multi, sph_mgpu_step(multi, reinterpret_cast<SphTimes *>(times)), "sph_mgpu_step");
        return;
    }
    check(impl, sph_step(impl, reinterpret_cast<SphTimes *>(times)), "sph_step");
}

// what the three render* methods share: `render` queues the frame on the single-domain handle; the frame in pinned memory
template <class Render>
static const unsigned char *rendered(const char *method, bool multi, sph_handle *impl, int *width, int *height, const char *call,
                                     Render render) {
    if (multi) {
        fprintf(stderr, "sph: %s: frames of a multi-GPU run (SPH_GPUS > 1) are not rendered\n", method);
        return NULL;
    }
    if (!impl) return NULL;
    check(impl, render(), call);
    const unsigned char *f = sph_frame_host(impl, width, height);
    if (!f) check(impl, SPH_EHIP, "sph_frame_host");
    return f;
}

const unsigned char *Simulator::renderFrame(int *width, int *height) {
    return rendered("renderFrame", multi, impl, width, height, "sph_render_frame", [&] { return sph_render_frame(impl, NULL); });
}

const unsigned char *Simulator::renderField(int field, int *width, int *height) {
    SphFieldFrameOptions o{};
    o.struct_size = (int32_t)sizeof o;
    o.field = field;
    return rendered("renderField", multi, impl, width, height, "sph_render_field", [&] { return sph_render_field(impl, &o); });
}

const unsigned char *Simulator::renderColumn(int *width, int *height) {
    return rendered("renderColumn", multi, impl, width, height, "sph_render_column", [&] { return sph_render_column(impl, NULL); });
}

const unsigned char *Simulator::renderLiquid(int *width, int *height) {
    return rendered("renderLiquid", multi, impl, width, height, "sph_render_liquid", [&] { return sph_render_liquid(impl, NULL); });
}

const float *Simulator::sampleField(int field, const float origin[3], const float spacing[3], int nx, int ny, int nz) {
    if (multi) {
        fprintf(stderr, "sph: sampleField: a multi-GPU run (SPH_GPUS > 1) is not sampled\n");
        return NULL;
    }
    if (!impl) return NULL;
    SphSampleLattice l{};
    l.struct_size = (int32_t)sizeof l;
    l.nx = nx, l.ny = ny, l.nz = nz;
    for (int k = 0; k < 3; ++k) l.origin[k] = origin[k], l.spacing[k] = spacing[k];
    l.field = field;
    const int rc = sph_sample_field(impl, &l);
    if (rc == SPH_ESTATE) { // (SPH_SWEEP=linked, a step split into phases, ...): nothing to sample, nothing broken
        fprintf(stderr, "sph: sampleField: %s\n", sph_last_error(impl));
        return NULL;
    }
    check(impl, rc, "sph_sample_field");
    const float *v = sph_sample_host(impl, NULL, NULL, NULL);
    if (!v) check(impl, SPH_EHIP, "sph_sample_host");
    return v;
}

bool Simulator::extractSurface(float iso, const float origin[3], const float spacing[3], int nx, int ny, int nz,
                               const float **vertices, long long *numVertices, const unsigned **triangles, long long *numTriangles) {
    if (multi) {
        fprintf(stderr, "sph: extractSurface: a multi-GPU run (SPH_GPUS > 1) is not meshed\n");
        return false;
    }
    if (!impl) return false;
    SphSurfaceOptions o{};
    o.struct_size = (int32_t)sizeof o;
    o.nx = nx, o.ny = ny, o.nz = nz;
    for (int k = 0; k < 3; ++k) o.origin[k] = origin[k], o.spacing[k] = spacing[k];
    o.iso = iso;
    const int rc = sph_extract_surface(impl, &o);
    if (rc == SPH_ESTATE) { // (SPH_SWEEP=linked, a step split into phases, ...): nothing to mesh, nothing broken
        fprintf(stderr, "sph: extractSurface: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_extract_surface");
    const float *v = NULL;
    const uint32_t *t = NULL;
    int64_t nv = 0, nt = 0;
    check(impl, sph_surface_host(impl, &v, &nv, &t, &nt), "sph_surface_host");
    if (vertices) *vertices = v;
    if (numVertices) *numVertices = nv;
    if (triangles) *triangles = t;
    if (numTriangles) *numTriangles = nt;
    return true;
}

// the tracer calls share their way out: a multi-GPU run and SPH_ESTATE are reported, anything else is fatal
static bool tracer_call(sph_handle *impl, sph_mgpu *multi, int rc, const char *what) {
    if (multi) {
        fprintf(stderr, "sph: %s: a multi-GPU run (SPH_GPUS > 1) carries no tracers\n", what);
        return false;
    }
    if (!impl) return false;
    if (rc == SPH_ESTATE) { // (SPH_SWEEP=linked, a step split into phases, ...): nothing moved, nothing broken
        fprintf(stderr, "sph: %s: %s\n", what, sph_last_error(impl));
        return false;
    }
    check(impl, rc, what);
    return true;
}

bool Simulator::setTracers(const float *pos_xyz, int m) {
    return tracer_call(impl, multi, (multi || !impl) ? SPH_OK : sph_tracers_set(impl, pos_xyz, m), "setTracers");
}

bool Simulator::advectTracers(float dt) {
    return tracer_call(impl, multi, (multi || !impl) ? SPH_OK : sph_tracers_advect(impl, dt), "advectTracers");
}

bool Simulator::getTracers(const float **posDen, const float **vel, int *m) {
    return tracer_call(impl, multi, (multi || !impl) ? SPH_OK : sph_tracers_host(impl, posDen, vel, m), "getTracers");
}

bool Simulator::deriveFlow(const float **vortDiv, const float **gradRho, const uint32_t **neighbours) {
    if (multi) {
        fprintf(stderr, "sph: deriveFlow: a multi-GPU run (SPH_GPUS > 1) derives no fields\n");
        return false;
    }
    if (!impl) return false;
    const int rc = sph_derive(impl);
    if (rc == SPH_ESTATE) { // (SPH_SWEEP=linked, a step split into phases, ...): nothing computed, nothing broken
        fprintf(stderr, "sph: deriveFlow: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_derive");
    check(impl, sph_derived_host(impl, vortDiv, gradRho, neighbours, NULL), "sph_derived_host");
    return true;
}

bool Simulator::labelBodies(float link, const uint32_t **labels, const uint32_t **table, int *numBodies, uint32_t *largest) {
    if (multi) {
        fprintf(stderr, "sph: labelBodies: a multi-GPU run (SPH_GPUS > 1) labels no bodies\n");
        return false;
    }
    if (!impl) return false;
    SphBodyOptions o;
    o.struct_size = (int32_t)sizeof o;
    o.link = link;
    const int rc = sph_label_bodies(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL) { // (SPH_SWEEP=linked, a link longer than h, ...): nothing computed, nothing broken
        fprintf(stderr, "sph: labelBodies: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_label_bodies");
    check(impl, sph_bodies_host(impl, labels, NULL, table, numBodies, largest), "sph_bodies_host");
    return true;
}

bool Simulator::measureBodies(float link, const SphBodyMomentsRaw **rows, int *numBodies, const uint32_t **sizeHist) {
    if (multi) {
        fprintf(stderr, "sph: measureBodies: a multi-GPU run (SPH_GPUS > 1) labels no bodies\n");
        return false;
    }
    if (!impl) return false;
    SphBodyMeasureOptions o = {};
    o.struct_size = (int32_t)sizeof o;
    o.link = link;
    const int rc = sph_measure_bodies(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL || rc == SPH_ENOMEM) { // (SPH_SWEEP=linked, a link longer than h, ...): nothing computed, nothing broken
        fprintf(stderr, "sph: measureBodies: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_measure_bodies");
    check(impl, sph_body_moments_host(impl, rows, numBodies, sizeHist), "sph_body_moments_host");
    return true;
}

bool Simulator::trackBodies(float link, const uint32_t **table, const SphBodyTrack **tracks, int *numBodies, const SphBodyFate **previous,
                            int *numPrevious, const SphBodyEdge **edges, int *numEdges, SphBodyTrackSummary *summary) {
    if (multi) {
        fprintf(stderr, "sph: trackBodies: a multi-GPU run (SPH_GPUS > 1) labels no bodies\n");
        return false;
    }
    if (!impl) return false;
    SphBodyTrackOptions o = {};
    o.struct_size = (int32_t)sizeof o;
    o.link = link;
    const int rc = sph_track_bodies(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL || rc == SPH_ENOMEM) { // (SPH_SWEEP=linked, a link longer than h, ...): nothing computed, nothing broken
        fprintf(stderr, "sph: trackBodies: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_track_bodies");
    check(impl, sph_bodies_host(impl, NULL, NULL, table, NULL, NULL), "sph_bodies_host");
    check(impl, sph_body_tracks_host(impl, tracks, numBodies, previous, numPrevious, edges, numEdges, summary), "sph_body_tracks_host");
    return true;
}

bool Simulator::resetTracks() {
    if (multi || !impl) return false;
    check(impl, sph_track_reset(impl), "sph_track_reset");
    return true;
}

bool Simulator::neighbourLists(float radius, const uint64_t **offsets, const uint32_t **neighbours, uint64_t *entries) {
    if (multi) {
        fprintf(stderr, "sph: neighbourLists: a multi-GPU run (SPH_GPUS > 1) lists no neighbours\n");
        return false;
    }
    if (!impl) return false;
    SphNeighbourOptions o = {};
    o.struct_size = (int32_t)sizeof o;
    o.radius = radius;
    const int rc = sph_neighbour_lists(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL || rc == SPH_ENOMEM) { // (SPH_SWEEP=linked, a radius longer than h, more ids than
                                                                    // max_entries, ...): no lists, nothing broken
        fprintf(stderr, "sph: neighbourLists: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_neighbour_lists");
    check(impl, sph_neighbours_host(impl, offsets, neighbours, NULL, entries), "sph_neighbours_host");
    return true;
}

bool Simulator::pairStatistics(int bins, float radius, const SphPairBinRaw **rows, const float **edges2, int *numBins) {
    if (multi) {
        fprintf(stderr, "sph: pairStatistics: a multi-GPU run (SPH_GPUS > 1) gathers no pair statistics\n");
        return false;
    }
    if (!impl) return false;
    SphPairOptions o = {};
    o.struct_size = (int32_t)sizeof o;
    o.radius = radius;
    o.bins = bins;
    const int rc = sph_pair_statistics(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL) { // (SPH_SWEEP=linked, a radius longer than h, ...): no table, nothing broken
        fprintf(stderr, "sph: pairStatistics: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_pair_statistics");
    check(impl, sph_pair_statistics_host(impl, rows, edges2, numBins), "sph_pair_statistics_host");
    return true;
}

bool Simulator::castRays(const SphRay *rays, int m, float radius, const uint64_t **words) {
    if (multi) {
        fprintf(stderr, "sph: castRays: a multi-GPU run (SPH_GPUS > 1) casts no rays\n");
        return false;
    }
    if (!impl) return false;
    SphCastOptions o = {};
    o.struct_size = (int32_t)sizeof o;
    o.radius = radius;
    const int rc = sph_cast_rays(impl, rays, m, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL) { // (SPH_SWEEP=linked, a radius longer than h, ...): no words, nothing broken
        fprintf(stderr, "sph: castRays: %s\n", sph_last_error(impl));
        return false;
    }
    check(impl, rc, "sph_cast_rays");
    check(impl, sph_cast_host(impl, words, NULL), "sph_cast_host");
    return true;
}

const unsigned char *Simulator::renderView(const SphViewOptions &view, int *width, int *height) {
    if (multi) {
        fprintf(stderr, "sph: renderView: frames of a multi-GPU run (SPH_GPUS > 1) are not rendered\n");
        return NULL;
    }
    if (!impl) return NULL;
    SphViewOptions o = view;
    o.struct_size = (int32_t)sizeof o;
    const int rc = sph_render_view(impl, &o);
    if (rc == SPH_ESTATE || rc == SPH_EINVAL) { // (SPH_SWEEP=linked, a camera that looks along `up`, ...): no frame, nothing broken
        fprintf(stderr, "sph: renderView: %s\n", sph_last_error(impl));
        return NULL;
    }
    check(impl, rc, "sph_render_view");
    const unsigned char *f = sph_frame_host(impl, width, height);
    if (!f) check(impl, SPH_EHIP, "sph_frame_host");
    return f;
}

bool Simulator::getVelocity(float *vel_xyz) {
    if (multi || !impl || !vel_xyz) return false;
    check(impl, sph_download_state(impl, NULL, vel_xyz, NULL, NULL), "sph_download_state");
    return true;
}

bool Simulator::diagnostics(SphDiagnostics *out, SphDiagnosticsRaw *raw) {
    if (!out || (!impl && !multi)) {
        fprintf(stderr, "sph: diagnostics: setup() must come first\n");
        return false;
    }
    SphDiagnosticsRaw r;
    if (multi) {
        mcheck(multi, sph_mgpu_diagnostics(multi, NULL, &r), "sph_mgpu_diagnostics");
    } else {
        check(impl, sph_diagnose(impl, NULL), "sph_diagnose");
        check(impl, sph_diagnostics_host(impl, &r), "sph_diagnostics_host");
    }
    SphSettings s;
    memcpy(&s, settings, sizeof s);
    check(impl, sph_diagnostics_values(&r, &s, out), "sph_diagnostics_values");
    if (raw) *raw = r;
    return true;
}

void Simulator::moveParticles(int2 mouse_pos) {
    if (multi) { // multi-GPU: the impulse needs the slabs' grids of a step: it rides on the next simulate()
        mcheck(multi, sph_mgpu_queue_click(multi, mouse_pos.x, mouse_pos.y), "sph_mgpu_queue_click");
        return;
    }
    if (!impl) return;
    check(impl, sph_apply_click(impl, mouse_pos.x, mouse_pos.y), "sph_apply_click");
}
