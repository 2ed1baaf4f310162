/*
 * reference_driver.cpp -- a C ABI over the reference's own Simulator, run on the host.
 * TEST INFRASTRUCTURE ONLY (oracle/reference.py, tests/test_reference_pin_cpu.py).
 *
 * Linked with the reference's simulator.cu compiled as C++ against ref_host/cuda_runtime.h
 * (oracle/Makefile, target ref).  Compiled against the reference's simulator.h with
 * -fno-access-control, so that particles[] can be written and read.  This file defines what
 * that translation unit declares extern: the index variables, the build schedule, and the two
 * mouse globals of the reference's display code.
 *
 * Hazards, all inherited from the reference's text:
 *  - no bounds check: a particle outside the grid is a wild write into the cell table.  The
 *    caller keeps every state inside the grid (tests assert it before every step);
 *  - setup() with randomInit consumes the process's rand();
 *  - setup() leaks its staging array (a malloc it never frees);
 *  - the destructor walks the lists and frees nodes that live inside the particle block, and
 *    pairs malloc with delete[]: ref_destroy() frees the four blocks itself and clears the
 *    pointers first, so that the destructor finds nothing to do.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simulator.h"

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
const int *ref_build_schedule = nullptr;
long ref_build_schedule_len = 0;
bool mouseClicked = false;
int2 clickCoords = {0, 0};

extern Settings deviceSettings;   /* the reference's __constant__ copy, one per process */

namespace {
struct RefSim {
    Settings settings;
    Simulator *sim = nullptr;
    bool is_setup = false;
    std::vector<int> schedule;     /* thread indices, first to run first; empty: the default */
};
}  // namespace

static void release_blocks(RefSim *r) {
    if (!r->is_setup) return;
    std::free(r->sim->neighborGrid);
    std::free(r->sim->particles);
    std::free(r->sim->devicePosition);
    std::free(r->sim->position);
    r->sim->neighborGrid = nullptr;
    r->sim->particles = nullptr;
    r->sim->position = nullptr;
    r->is_setup = false;
}

extern "C" {

int ref_sizeof_settings(void) { return static_cast<int>(sizeof(Settings)); }
int ref_sizeof_particle(void) { return static_cast<int>(sizeof(Particle)); }

void *ref_create(const void *settings, int bytes) {
    if (bytes != static_cast<int>(sizeof(Settings))) return nullptr;
    RefSim *r = new RefSim;
    std::memcpy(&r->settings, settings, sizeof(Settings));
    r->sim = new Simulator(&r->settings);
    return r;
}

/* the reference's own setup(): allocation and its initialiser */
void ref_setup(void *h) {
    RefSim *r = static_cast<RefSim *>(h);
    release_blocks(r);            /* setup() allocates anew every time */
    r->sim->setup();
    r->is_setup = true;
    r->schedule.clear();
}

/* a new state, particle-id order; vel may be null (at rest).  Needs setup(). */
int ref_upload(void *h, const float *pos, const float *vel) {
    RefSim *r = static_cast<RefSim *>(h);
    if (!r->is_setup) return -1;
    const int n = r->settings.numParticles;
    for (int i = 0; i < n; ++i) {
        Particle p(make_float3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]));
        if (vel) p.velocity = make_float3(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]);
        r->sim->particles[i] = p;
    }
    r->schedule.clear();
    return 0;
}

/* order: the n particle ids in the order every cell's list must READ for the next step (null or
 * n == 0: back to the default).  kernelBuildGrid's threads then run in the reverse of it. */
int ref_set_schedule(void *h, const int32_t *order, int n) {
    RefSim *r = static_cast<RefSim *>(h);
    r->schedule.clear();
    if (!order || n == 0) return 0;
    if (n != r->settings.numParticles) return -1;
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || seen[order[i]]) return -2;
        seen[order[i]] = 1;
    }
    r->schedule.assign(order, order + n);
    for (int i = 0, j = n - 1; i < j; ++i, --j) std::swap(r->schedule[i], r->schedule[j]);
    return 0;
}

/* one simulate(); with click != 0 the reference's own click: the two globals, then simulate() */
int ref_step(void *h, int click, int mouse_x, int mouse_y) {
    RefSim *r = static_cast<RefSim *>(h);
    if (!r->is_setup) return -1;
    deviceSettings = r->settings;
    ref_build_schedule = r->schedule.empty() ? nullptr : r->schedule.data();
    ref_build_schedule_len = static_cast<long>(r->schedule.size());
    mouseClicked = click != 0;
    clickCoords = {mouse_x, mouse_y};
    r->sim->simulate();
    mouseClicked = false;
    ref_build_schedule = nullptr;
    ref_build_schedule_len = 0;
    r->schedule.clear();          /* a schedule serves one step */
    return 0;
}

/* by particle id (particles[] is never permuted).  Any pointer may be null. */
void ref_download(void *h, float *pos, float *vel, float *rho, float *prs, float *force) {
    RefSim *r = static_cast<RefSim *>(h);
    const int n = r->settings.numParticles;
    for (int i = 0; i < n; ++i) {
        const Particle &p = r->sim->particles[i];
        if (pos) { pos[3 * i] = p.position.x; pos[3 * i + 1] = p.position.y; pos[3 * i + 2] = p.position.z; }
        if (vel) { vel[3 * i] = p.velocity.x; vel[3 * i + 1] = p.velocity.y; vel[3 * i + 2] = p.velocity.z; }
        if (force) { force[3 * i] = p.force.x; force[3 * i + 1] = p.force.y; force[3 * i + 2] = p.force.z; }
        if (rho) rho[i] = p.density;
        if (prs) prs[i] = p.pressure;
    }
}

/* the reference's getPosition(): the host copy its last simulate() left */
void ref_get_position(void *h, float *out) {
    RefSim *r = static_cast<RefSim *>(h);
    const float3 *p = r->sim->getPosition();
    for (int i = 0; i < r->settings.numParticles; ++i) {
        out[3 * i] = p[i].x; out[3 * i + 1] = p[i].y; out[3 * i + 2] = p[i].z;
    }
}

/* The four blocks by name, then the destructor over cleared pointers (see the head of this file). */
void ref_destroy(void *h) {
    RefSim *r = static_cast<RefSim *>(h);
    if (!r) return;
    release_blocks(r);
    delete r->sim;
    delete r;
}

}  // extern "C"
