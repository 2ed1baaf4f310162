// Public C++ surface of the MI355X SPH simulator.
//
// Field-for-field / method-for-method the same surface as the reference's
// src/simulator.h:6-74 so its front ends (src/main.cpp, src/display.cpp) build
// against this header unchanged: the physics and click-box macros, `Settings`
// (positional brace-init in main.cpp:62-63 depends on the field order),
// `Particle`, and `class Simulator`.  What differs is private: the reference
// keeps CUDA device pointers here, this class keeps one opaque handle of the
// C-ABI in sph_c_api.h, behind which the hand-written gfx950 kernels live.
#ifndef SPH_SIMULATOR_H
#define SPH_SIMULATOR_H

#include <stdint.h>
#include <stdio.h>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_vector_types.h> // float3, int2, make_int2 (types only)

#include "times.h"

#define PI 3.14159265f
#define MASS 0.02f
#define GAS_CONSTANT 1.f
#define REST_DENSITY 1000.f
#define VISCOSITY 1.f
#define GRAVITY -9.8f
#define ELASTICITY 0.5f

// window-pixel box inside which a left click pushes the fluid (display.cpp:22-32)
#define BOX_MAX_X (600)
#define BOX_MIN_X (200)
#define BOX_MAX_Y (450)
#define BOX_MIN_Y (150)

struct Settings {
    bool randomInit;
    int numParticles;
    float h;

    // Pre-computed constants
    float v_kernel_coeff;
    float d_kernel_coeff;

    float boxDim;
    float numCellsPerDim;
    float timestep;
};

// Legacy per-particle record of the reference's AoS layout.  The simulator no
// longer stores particles this way (state is two key-sorted float4 streams on
// the device); the type is kept so code that names it still compiles.
struct Particle {
    float3 position, velocity, force;
    float density, pressure;
    struct Particle *next;

    Particle(float3 pos)
        : position(pos), velocity{0.f, 0.f, 0.f}, force{0.f, 0.f, 0.f}, density(0.f),
          pressure(0.f), next(NULL) {}

    void display() { printf("(%f, %f, %f)\n", position.x, position.y, position.z); }
};

struct sph_handle;
struct sph_mgpu;
struct SphDiagnostics;    // include/sph_c_api.h
struct SphDiagnosticsRaw;
struct SphBodyMomentsRaw;
struct SphBodyTrack;
struct SphBodyFate;
struct SphBodyEdge;
struct SphBodyTrackSummary;
struct SphPairBinRaw;
struct SphRay;
struct SphViewOptions;

class Simulator {
  private:
    struct sph_handle *impl; // one GPU (include/sph_c_api.h)
    struct sph_mgpu *multi;  // SPH_GPUS=N: z-slabs over N GPUs (include/sph_mgpu.h)

  public:
    const Settings *settings;

    Simulator(Settings *settings);
    virtual ~Simulator();

    void setup();

    const float3 *getPosition();

    void simulate();
    void simulateAndTime(Times *times);
    void moveParticles(int2 mouse_pos);

    // Not in the reference: the frame display.cpp would draw of the current state -- 800 x 600, RGB8,
    // row 0 = top of the window -- rendered on the GPU (sph_render_frame in sph_c_api.h).  Owned by the
    // simulator, valid until the next call.  NULL (with a message on stderr) with SPH_GPUS > 1.
    const unsigned char *renderFrame(int *width, int *height);
    // The same frame with the particles coloured by a field of the nearest one: field = SPH_FIELD_SPEED (0),
    // SPH_FIELD_DENSITY (1) or SPH_FIELD_PRESSURE (2), the colour scale over the frame's own minimum and maximum
    // (sph_render_field in sph_c_api.h).
    const unsigned char *renderField(int field, int *width, int *height);
    // The column-density frame of the same camera: how much fluid lies behind each pixel, the colour scale from 0 to
    // the frame's largest column (sph_render_column in sph_c_api.h).
    const unsigned char *renderColumn(int *width, int *height);
    // The liquid frame of the same camera: the fluid as a smoothed, lit water surface, every option at its default
    // (sph_render_liquid in sph_c_api.h).
    const unsigned char *renderLiquid(int *width, int *height);
    // The SPH-interpolated field on a regular lattice (sph_sample_field in sph_c_api.h): nx x ny x nz floats, point
    // (ix, iy, iz) = origin + i * spacing per axis at index (iz ny + iy) nx + ix.  Owned by the simulator, valid
    // until the next call.  NULL (with a message on stderr) with SPH_GPUS > 1 and where the library answers
    // SPH_ESTATE (SPH_SWEEP=linked has no cell table to walk).
    const float *sampleField(int field, const float origin[3], const float spacing[3], int nx, int ny, int nz);
    // The surface density == iso over the same kind of lattice as an indexed triangle mesh (sph_extract_surface in
    // sph_c_api.h): 3 floats per vertex, 3 indices per triangle, owned by the simulator, valid until the next call;
    // the pointers may be NULL for an empty mesh.  false (with a message on stderr) with SPH_GPUS > 1 and where
    // the library answers SPH_ESTATE.
    bool extractSurface(float iso, const float origin[3], const float spacing[3], int nx, int ny, int nz,
                        const float **vertices, long long *numVertices, const unsigned **triangles, long long *numTriangles);
    // Passive tracers (sph_tracers_* in sph_c_api.h): m points (x, y, z interleaved) that the caller seeds and that
    // advectTracers carries through the velocity field of the current state, one explicit Euler move of `dt` per call
    // (dt == 0: sample without moving).  getTracers: m x 4 floats each, (x, y, z, den) and (ux, uy, uz, 0), owned by
    // the simulator, valid until the next advectTracers or setTracers.  false (with a message on stderr) with
    // SPH_GPUS > 1 and where the library answers SPH_ESTATE.
    bool setTracers(const float *pos_xyz, int m);
    bool advectTracers(float dt);
    bool getTracers(const float **posDen, const float **vel, int *m);
    // Derived per-particle fields of the current state (sph_derive in sph_c_api.h), in particle-id order: n x 4
    // floats each, (wx, wy, wz, divergence) and (gx, gy, gz, rho), and n neighbour counts, owned by the simulator,
    // valid until the next deriveFlow.  Any out-pointer may be NULL.  false (with a message on stderr) with
    // SPH_GPUS > 1 and where the library answers SPH_ESTATE.
    bool deriveFlow(const float **vortDiv, const float **gradRho, const uint32_t **neighbours);
    // The bodies of the current state (sph_label_bodies in sph_c_api.h): the connected pieces of fluid at link length
    // `link` (0: h; else 0 < link <= h).  n labels in particle-id order, numBodies table rows of 8 words (label,
    // count, bounding box), owned by the simulator, valid until the next labelBodies; *largest is the label of the
    // body with the most particles.  Any out-pointer may be NULL.  false (with a message on stderr) with SPH_GPUS > 1
    // and where the library answers SPH_ESTATE or SPH_EINVAL.
    bool labelBodies(float link, const uint32_t **labels, const uint32_t **table, int *numBodies, uint32_t *largest);
    // The moments of the bodies of the current state (sph_measure_bodies in sph_c_api.h): labels them as labelBodies
    // does, then numBodies raw rows in the table's order -- label, count, the exact sums; sph_body_values derives
    // mass, centre, momentum, energies, covariance and angular momentum from them -- and the 32 bins of the size
    // distribution, owned by the simulator, valid until the next measureBodies.  Any out-pointer may be NULL.  false
    // (with a message on stderr) with SPH_GPUS > 1 and where the library answers SPH_ESTATE, SPH_EINVAL or SPH_ENOMEM.
    bool measureBodies(float link, const SphBodyMomentsRaw **rows, int *numBodies, const uint32_t **sizeHist);
    // The tracks of the bodies of the current state (sph_track_bodies in sph_c_api.h): labels them as labelBodies does
    // and joins the labelling with that of the last successful trackBodies -- numBodies SphBodyTrack beside the
    // numBodies rows of `table` (8 words each: label, count, bounding box), numPrevious SphBodyFate for the bodies of
    // the last call, numEdges SphBodyEdge in ascending (cur, prev) order and the summary, owned by the simulator, valid
    // until the next trackBodies.  Any out-pointer may be NULL.  resetTracks forgets the last call's labelling: the
    // next trackBodies finds no previous bodies and numbers its tracks from 0.  false (with a message on stderr) with
    // SPH_GPUS > 1 and where the library answers SPH_ESTATE, SPH_EINVAL or SPH_ENOMEM.
    bool trackBodies(float link, const uint32_t **table, const SphBodyTrack **tracks, int *numBodies, const SphBodyFate **previous,
                     int *numPrevious, const SphBodyEdge **edges, int *numEdges, SphBodyTrackSummary *summary);
    bool resetTracks();
    // The neighbour lists of the current state (sph_neighbour_lists in sph_c_api.h) as CSR in particle-id order: the
    // neighbours of particle i -- the particles within `radius` of it (0: h; else 0 < radius <= h), in ascending id
    // order -- are neighbours[offsets[i]] .. neighbours[offsets[i + 1] - 1]; n + 1 offsets, *entries ids, owned by the
    // simulator, valid until the next neighbourLists.  Any out-pointer may be NULL.  false (with a message on stderr)
    // with SPH_GPUS > 1 and where the library answers an error (SPH_ENOMEM: more than 1 << 28 ids).
    bool neighbourLists(float radius, const uint64_t **offsets, const uint32_t **neighbours, uint64_t *entries);
    // The pair statistics of the current state (sph_pair_statistics in sph_c_api.h): per bin of separation -- `bins`
    // bins (0: 32; at most 128) of equal width up to `radius` (0: h; else 0 < radius <= h) -- the number of pairs and
    // the exact sums behind g(r) and the velocity structure functions; *numBins rows and squared edges, owned by the
    // simulator, valid until the next pairStatistics; sph_pair_values turns them into floats.  Any out-pointer may be
    // NULL.  false (with a message on stderr) with SPH_GPUS > 1 and where the library answers SPH_ESTATE or SPH_EINVAL.
    bool pairStatistics(int bins, float radius, const SphPairBinRaw **rows, const float **edges2, int *numBins);
    // What lines of sight hit first (sph_cast_rays in sph_c_api.h): m rays against the particles as spheres of `radius`
    // (0: 0.5 h; else 0 < radius <= h); m words (bits(t) << 32) | id in the caller's order, SPH_CAST_MISS for a miss,
    // owned by the simulator, valid until the next castRays.  false (with a message on stderr) with SPH_GPUS > 1 and
    // where the library answers SPH_ESTATE or SPH_EINVAL.
    bool castRays(const SphRay *rays, int m, float radius, const uint64_t **words);
    // A lit frame of the current state from any pinhole camera (sph_render_view in sph_c_api.h), owned by the simulator,
    // valid until the next render.  NULL (with a message on stderr) with SPH_GPUS > 1 and where the library answers
    // SPH_ESTATE or SPH_EINVAL.
    const unsigned char *renderView(const SphViewOptions &view, int *width, int *height);
    // The velocities of the current state (sph_download_state), n x 3 floats in particle-id order, into the caller's
    // buffer.  false with SPH_GPUS > 1 and before setup().
    bool getVelocity(float *vel_xyz);
    // Run diagnostics of the current state, reduced on the GPU (sph_diagnose in sph_c_api.h): total kinetic and
    // potential energy, momentum, centre of mass, the fastest particle, the CFL number, the spread of density.
    // *raw, if given, receives the exact words behind them.  With SPH_GPUS > 1 through the multi-GPU driver
    // (sph_mgpu_diagnostics): the same words.  False (with a message on stderr) before setup().
    bool diagnostics(SphDiagnostics *out, SphDiagnosticsRaw *raw = nullptr);
};

#endif
