/*
 * sph_c_api.h -- C-ABI drop-in boundary of the MI355X SPH step path.
 *
 * Plain C types only (no HIP, no torch).  This is what a host program in any
 * language binds (cgo / JNI / ctypes / the C++ `Simulator` class in
 * include/simulator.h).  The reference has no FFI of its own -- its boundary is
 * the C++ class in src/simulator.h:53-74 -- so each entry point cites the
 * reference method or code it replaces.  All functions return 0 on success and
 * a negative SPH_E* code on failure; sph_last_error() gives the message.
 *
 * Threading: a handle is used from one host thread at a time (the reference is
 * single-threaded, simulator.cu:462-546).  Work is queued on the handle's own
 * HIP streams; sph_positions_host()/sph_download_state()/sph_sync() block until
 * the data they expose is complete, so callers observe the reference's
 * "synchronous on return" behaviour.
 */
#ifndef SPH_C_API_H
#define SPH_C_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_API_VERSION 3 /* 2: + sph_slab_apply_click, sph_slab_records; 3: + sph_render_frame, sph_frame_host,
                             sph_download_frame_buffers, sph_get_render_time, sph_api_version (additive; every
                             earlier entry point unchanged) */

#define SPH_OK 0
#define SPH_EINVAL (-1)  /* bad argument / state outside the box       */
#define SPH_EHIP (-2)    /* a HIP runtime call failed                   */
#define SPH_ENOMEM (-3)  /* host or device allocation failed            */
#define SPH_ESTATE (-4)  /* call order violated (e.g. step before setup) */
#define SPH_ENODEV (-5)  /* no usable GPU                               */

/* Layout-identical to the reference's `struct Settings` (simulator.h:19-31):
 * bool, int, 6 floats = 32 bytes.  numCellsPerDim is a float there too.
 *
 * Grids: sph_create accepts 1 <= numCellsPerDim <= 1024 and any h > 0.  The library flattens cell
 * coordinates in integers, key = cx + cy D + cz D^2.  The reference (and the CPU oracle) flatten in
 * fp32, which is exact only while every key formed stays below 2^24: D <= 256, or D = 257 with every
 * particle below z-layer 253.  Up to there the library equals the reference's arithmetic bit for bit
 * (tests/test_gpu_grids.py); above it the reference's own keys collide and the integer keys are the
 * definition.  D = 1 is accepted, but its wall planes sit at h and boxDim - h = 0: the first step
 * clamps every particle to h, outside the one-cell grid. */
typedef struct SphSettings {
    uint8_t randomInit;
    uint8_t pad_[3];
    int32_t numParticles;
    float h;
    float v_kernel_coeff;
    float d_kernel_coeff;
    float boxDim;
    float numCellsPerDim;
    float timestep;
} SphSettings;

/* Layout-identical to the reference's `struct Times` (times.h:5-10). */
typedef struct SphTimes {
    double buildGrid;
    double sphUpdate;
    double memcpy;
    int32_t iters;
} SphTimes;

enum {
    SPH_MATH_STRICT = 0, /* every op individually rounded; bit-identical to oracle */
    SPH_MATH_FAST = 1    /* FMA contraction + approximate rcp/sqrt (tolerance-checked) */
};
enum {
    SPH_SWEEP_LIST = 0,   /* production: LDS-staged density sweep records one hit bit per
                             candidate, the force sweep walks the recorded hits */
    SPH_SWEEP_DIRECT = 1, /* check path: one thread per particle, direct global loads */
    SPH_SWEEP_LDS = 2,    /* LDS-staged window in both sweeps, hit FIFO in the force sweep */
    SPH_SWEEP_LINKED = 3  /* the reference's own neighbour structure: no sort, one atomically
                             built linked list per cell (simulator.cu:44-55,133-147), walked
                             as in :163-189/:207-251.  Summation order is a race, so results
                             match the oracle to rounding only, and differ run to run.  Kept to
                             time "the reference's algorithm on MI355X"; strict math, single
                             domain only; sph_apply_click / sph_download_grid / the slab entry
                             points return SPH_ESTATE. */
};
enum {
    SPH_FLAG_COUNT_PAIRS = 1, /* accumulate the candidate pair-test count per step */
    SPH_FLAG_STORE_FORCE = 2, /* keep per-particle force of the last step (tests)  */
    SPH_FLAG_NO_READBACK = 4, /* skip the per-step D2H of positions (kernel studies) */
    SPH_FLAG_EXTERNAL_STATE = 8, /* particle streams are caller-owned device buffers
                                   (sph_bind_buffers); used by the multi-GPU slab
                                   driver so halo send/recv is zero-copy */
    SPH_FLAG_MAPPED_POSITIONS = 16 /* the id-ordered positions of getPosition() are written by
                                   the force sweep STRAIGHT into host-mapped pinned memory
                                   (zero-copy: no per-step device->host copy); SURVEY.md 8f
                                   rank 3.  Measured slower than the overlapped copy at
                                   n = 4 M: kept as an option, not the default */
};

enum {
    SPH_KEY_FLATTENED = 0, /* x + y D + z D^2 (simulator.cu:78-82): the 27-cell walk is nine
                              contiguous runs of the sorted stream -- what every sweep is built on */
    SPH_KEY_MORTON = 1     /* bits of x, y, z interleaved (the ordering the reference's README.md:5
                              names for its z_index_sort branch; BASELINE config 3).  For the A/B of
                              the two orderings: SPH_SWEEP_DIRECT, strict math, single domain only */
};

typedef struct SphOptions {
    int32_t struct_size; /* = sizeof(SphOptions) */
    int32_t device;      /* HIP device ordinal; -1 = current */
    int32_t math_mode;   /* SPH_MATH_* */
    int32_t sweep;       /* SPH_SWEEP_* */
    int32_t flags;       /* SPH_FLAG_* */
    int32_t capacity;    /* particle slots to allocate (0 = numParticles); slabs
                            need room for halo + migrants */
    int32_t key_order;   /* SPH_KEY_* (callers built against the 24-byte struct get FLATTENED) */
} SphOptions;

/* Per-kernel GPU time, accumulated from HIP events recorded on the handle's
 * compute stream (seconds).  `steps` = number of steps accumulated. */
typedef struct SphKernelTimes {
    double hash, sort, gather, density, force, readback;
    uint64_t pair_tests; /* candidate pair tests (see "What the pair counters report" below) */
    int64_t steps;
    uint64_t pair_hits;  /* pair bodies the force sweep evaluated (SPH_SWEEP_LIST; 0 for the other sweeps) */
} SphKernelTimes;

typedef struct sph_handle sph_handle;

/* main.cpp:57-63 -- the constants main() derives before constructing Settings. */
int sph_default_settings(SphSettings *out, int numParticles, int randomInit);

/* The host half of Simulator::setup (simulator.cu:430-453) on its own: fills
 * numParticles x (x,y,z) with the reference initial condition.  Needs no GPU
 * (the slab driver splits this array across ranks). */
int sph_initial_positions(const SphSettings *settings, float *pos_xyz);

/* Simulator::Simulator (simulator.cu:370-375).  Copies *settings.  SPH_EINVAL unless h > 0 and
 * 1 <= numCellsPerDim <= 1024 (see SphSettings for what D > 256 and D = 1 mean). */
int sph_create(const SphSettings *settings, const SphOptions *options,
               sph_handle **out);
/* Simulator::~Simulator (simulator.cu:377-405). */
void sph_destroy(sph_handle *h);

/* Simulator::setup (simulator.cu:411-460): allocate, reference initial
 * conditions (random: glibc rand() as if never seeded; grid: 0.09 lattice),
 * upload.  n > 109^3 in grid mode is outside the reference's domain and uses
 * the labelled "dense lattice" extension. */
int sph_setup(sph_handle *h);
/* Replaces setup()'s initialiser with caller state in particle-id order
 * (xyz interleaved; vel may be NULL = zero).  Positions must lie in the box. */
int sph_upload_state(sph_handle *h, const float *pos_xyz, const float *vel_xyz,
                     int n);

/* Simulator::simulate (times == NULL, simulator.cu:462-497) and
 * Simulator::simulateAndTime (times != NULL, simulator.cu:499-546). */
int sph_step(sph_handle *h, SphTimes *times);
/* kernelMoveParticles (simulator.cu:329-367) on the last step's grid; this is
 * what simulate() runs when `mouseClicked` is set (simulator.cu:482-489). */
int sph_apply_click(sph_handle *h, int mouse_x, int mouse_y);

/* Simulator::getPosition (simulator.cu:407-409): numParticles x (x,y,z),
 * original particle-id order, owned by the handle, valid until the next step.
 * Blocks until the last step's device->host copy has landed. */
const float *sph_positions_host(sph_handle *h);
/* Full state in particle-id order; any pointer may be NULL. rho/prs are the
 * values kernelUpdatePressureAndDensity produced in the last step. */
int sph_download_state(sph_handle *h, float *pos_xyz, float *vel_xyz,
                       float *rho, float *prs);
int sph_download_force(sph_handle *h, float *force_xyz); /* SPH_FLAG_STORE_FORCE */
/* Sorted-order view of the last grid build: ids, flattened cell keys
 * (pre-integration), and the {start,end} cell table (numCells x 2 ints). */
int sph_download_grid(sph_handle *h, uint32_t *ids, uint32_t *keys,
                      int32_t *cell_ranges);

/* Checkpoint / resume (no reference counterpart).  The file
 * is a raw snapshot of the two cell-sorted float4 streams (ids included) plus a
 * 64-byte header, so a resumed run continues BIT-IDENTICALLY (the canonical
 * summation order depends on the stored order, not only on positions). */
int sph_save_state(sph_handle *h, const char *path);
int sph_load_state(sph_handle *h, const char *path);

int sph_sync(sph_handle *h);
int sph_num_particles(const sph_handle *h);
/* entries of the cell table sph_download_grid fills: D^3, or 8^ceil(log2 D) with Morton keys */
int sph_num_table_cells(const sph_handle *h);
int sph_get_kernel_times(sph_handle *h, SphKernelTimes *out, int reset);
const char *sph_last_error(const sph_handle *h); /* h may be NULL: create errors */
/* ---- What the pair counters report (SPH_FLAG_COUNT_PAIRS; without the flag all of them stay 0) ----
 * Three integers, exact and reproducible, held to a CPU count by tests/test_gpu_pair_counts.py.  All three are sums
 * over the steps since the handle was created or since the last sph_get_kernel_times(reset = 1); reading does not
 * consume them, and a new state (sph_setup / sph_upload_state / sph_load_state) or a click neither resets them nor
 * adds to them.  A step counts the same whether it is timed or not and whether or not it runs on a grid built ahead
 * (SPH_PIPELINE=1).
 *
 * pair_tests (= word 0 of sph_debug_counters): for every particle, the occupancy of its existing neighbour cells
 *   -- up to 27, fewer at the walls, the own cell and the particle itself included -- summed over the particles:
 *   the candidates ONE 27-cell sweep tests (a step runs two such sweeps; the number is not doubled).  The cell of a
 *   position is (int)(x / h) per axis in fp32.  A property of the state: every sweep (LIST, LDS, DIRECT, LINKED,
 *   either key order) reports the same number, whatever it stages, shares or walks to get there.
 * hits (word 15 of sph_debug_counters; SPH_SWEEP_LIST, 0 for the other sweeps): the ordered candidate pairs (i, j),
 *   i == j included, that the density sweep records in its hit masks.  Strict mode, fp32, every operation rounded
 *   on its own: dx = xi - xj, ..., d2 = (dx dx + dy dy) + dz dz; the pair is a hit when d2 <= h h OR sqrtf(d2) <= h
 *   (the force terms test r^2 and r, simulator.cu:105,125; the union is "d2 <= the largest float whose sqrtf is <=
 *   h").  For h = 0.1f and 0.2f the two conditions coincide; for h = 0.25f the second admits d2 = h h + 1 ulp.
 * pair_hits (= word 14 of sph_debug_counters; SPH_SWEEP_LIST, 0 for the other sweeps): hits minus the pairs the
 *   zero-pair filter drops.  The filter drops the pair (i, j) when BOTH rows are "quiet": pressure
 *   fmaxf(0, GAS_CONSTANT (rho - REST_DENSITY)) == 0 with this step's rho, and velocity equal (three float
 *   compares) to the step's reference velocity.  The reference velocity is the most common bit pattern among the
 *   velocities of the 64 rows floor(k n / 64), k = 0..63, of the order the step's grid build starts from (particle-id
 *   order after sph_setup / sph_upload_state; otherwise the previous step's cell-sorted order, which a snapshot
 *   keeps); ties go to the lowest k.  This is NARROWER than "neither row under pressure, same velocity": such a
 *   pair adds exactly +-0 whatever the common velocity is, but only pairs moving with the reference velocity are
 *   dropped.  When every row of a single domain is quiet the force sweep skips its hit stream, and pair_hits
 *   counts 0 for that step by the same rule (every hit is a pair of two quiet rows).
 *   With SPH_ZERO_PAIR_FILTER=0 nothing is dropped: pair_hits == hits.
 * Pool exhaustion: the hit-stream pool is cut into 64 equal sub-pools.  Wave w -- rows [64 w, 64 w + 64) of the
 *   cell-sorted order -- reserves 64 Q quads (16 bytes) from sub-pool w mod 64, Q = ceil(W / 2), W = the largest
 *   over its rows of the sum over the row's nine runs (the three x-adjacent cells of one (y, z)) of
 *   ceil(candidates / 32).  Reservations are served in arrival order and every arrival advances the sub-pool's
 *   cursor, whether it fits or not; when a sub-pool is too small for all its waves, WHICH of them fit is not
 *   determined.  A wave that does not fit records no stream: it adds 0 to hits and 0 to pair_hits (its rows are
 *   swept by the fallback, which tests every candidate again), and its candidates still count in pair_tests.
 *   With the default pool size no wave of the reference's runs falls back, and the three numbers are exact.
 * Slabs (sph_slab_density / sph_slab_force*): each handle counts its OWNED rows [i_begin, i_end); halo rows are
 *   candidates only.  pair_tests and hits therefore sum over the slabs to the single domain's numbers.  Each slab
 *   draws its own reference velocity, by the rule above, from the n_all rows sph_slab_sort starts from (halo rows
 *   included), and only OWNED rows can be quiet: a halo row's density arrives after the sweep.  pair_hits of a
 *   slab is therefore its hits minus the pairs of two of its owned quiet rows; a quiet row's pairs with halo rows
 *   are counted.  That also holds while the slab driver's "every row is quiet" shortcut (owned and halo rows)
 *   skips the hit stream: pair_hits is what the rule counts, not 0, although no body is evaluated in such a step.
 *   Summed over the slabs, hits - (pairs of two quiet rows) <= pair_hits <= hits, with equality on the right
 *   when the filter is off.
 *   include/sph_mgpu.h's driver does not expose the counters.
 * sph_debug_counters: [0] = pair_tests, [1..13] reserved, always zero, [14] = pair_hits, [15] = hits. */
int sph_debug_counters(sph_handle *h, uint64_t *out16);

/* ---- the step split into its phases (tests, profiling, slab driver) ---- */
int sph_phase_grid(sph_handle *h);     /* kernelBuildGrid + kernelResetGrid */
int sph_phase_density(sph_handle *h);  /* kernelUpdatePressureAndDensity    */
int sph_phase_force(sph_handle *h);    /* kernelUpdateForces + UpdatePositions */
int sph_phase_readback(sph_handle *h); /* the per-step D2H (simulator.cu:479) */

/* Stand-alone check of the radix sort used by the grid build: stable sort of
 * n (key, index) pairs; writes the permutation (host pointers). */
int sph_sort_check(int device, const uint32_t *keys, int n, int key_bits,
                   uint32_t *perm_out, uint32_t *sorted_keys_out);

/* ---- z-slab decomposition (one handle per GPU; cudafluidsimulator_amd/slab.py) ----
 * No reference counterpart: the reference is single-GPU.  The slab
 * driver owns four float4 device buffers per rank -- pos4[2], vel4[2], `capacity`
 * particles each -- and exchanges halo / migrant ranges of them with RCCL
 * send/recv; the library only runs kernels on ranges of those buffers, on the
 * caller's stream (so it is stream-ordered with the collectives). */
int sph_set_stream(sph_handle *h, void *hip_stream); /* a hipStream_t; NULL = HIP's default stream */
int sph_bind_buffers(sph_handle *h, void *pos4_a, void *vel4_a, void *pos4_b,
                     void *vel4_b, int capacity);
/* Hash + stable radix sort + gather of particles [src_offset, src_offset+count)
 * of buffer pair `src_buf` into [0, count) of the other pair, and the cell table
 * over the result.  bounds_out[k] = number of sorted keys < thresholds[k]
 * (k < nthr <= 8); blocks until those counts are on the host. */
int sph_slab_sort(sph_handle *h, int src_buf, int src_offset, int count,
                  const uint32_t *thresholds, int nthr, int32_t *bounds_out);
/* Stable PARTITION of particles [src_offset, src_offset+count) of buffer pair
 * `src_buf` into [0, count) of the other pair by key class (class = number of
 * thresholds <= the particle's new cell key; previous order kept inside a class).
 * What a rank needs before the exchange: [migrants down | lower boundary layer |
 * interior | upper boundary layer | migrants up] as contiguous ranges, at a third of
 * the launches of a full sort.  bounds_out[k] = number of particles with key <
 * thresholds[k].  Builds no cell table (sph_slab_sort of the combined array does).
 * bounds_dev_out (may be NULL): DEVICE pointer that receives nthr+1 int32 -- the
 * bounds, then `count` -- stream-ordered, so the driver can send them to the
 * neighbours as a message header without a round trip through the host. */
int sph_slab_partition(sph_handle *h, int src_buf, int src_offset, int count,
                       const uint32_t *thresholds, int nthr, int32_t *bounds_out,
                       void *bounds_dev_out);
/* Assemble the combined array: copy nseg <= 8 row ranges -- src_pos[k]/src_vel[k] are
 * DEVICE pointers to counts[k] float4 rows each (ranges of the bound buffers or of the
 * driver's receive buffers) -- to rows dst_offsets[k].. of buffer pair `dst_buf`, in one
 * kernel launch on the handle's stream. */
int sph_slab_copy_segments(sph_handle *h, int dst_buf, int nseg, const void *const *src_pos,
                           const void *const *src_vel, const int32_t *counts,
                           const int32_t *dst_offsets);
/* kernelUpdatePressureAndDensity for particles [i_begin, i_end) of the n_all
 * sorted particles in buffer pair `buf` (halo particles are candidates only). */
int sph_slab_density(sph_handle *h, int buf, int i_begin, int i_end, int n_all);
/* kernelUpdateForces + kernelUpdatePositions for [i_begin, i_end); new state is
 * written to the same indices of the other buffer pair. */
int sph_slab_force(sph_handle *h, int buf, int i_begin, int i_end, int n_all);

/* ---- the same phases WITHOUT a host round trip (include/sph_mgpu.h's in-process driver) ----
 * Everything is queued on the handle's stream (sph_get_stream: a hipStream_t) and
 * nothing blocks: the bounds are only written to DEVICE memory (bounds_dev_out:
 * nthr+1 int32 = the bounds, then `count`), from where the driver sends them to the
 * neighbours / copies them to pinned memory.  sph_slab_force_ranges runs the force +
 * integration sweep for row ranges of the owned range whose hit stream was recorded
 * by sph_slab_density(buf, i_origin, ...): the interior rows can run while the halo
 * densities are still in flight, the two boundary layers after sph_slab_patch_halo.
 * Every launch before the one flagged last_launch_of_the_step must hold INTERIOR rows only
 * (every neighbour an owned row): the last one also tests the halo rows for the zero-pair
 * filter's "every row is quiet" shortcut, the earlier ones rely on the owned rows alone. */
void *sph_get_stream(sph_handle *h);
int sph_slab_partition_async(sph_handle *h, int src_buf, int src_offset, int count,
                             const uint32_t *thresholds, int nthr, void *bounds_dev_out);
int sph_slab_sort_async(sph_handle *h, int src_buf, int src_offset, int count,
                        const uint32_t *thresholds, int nthr, void *bounds_dev_out);
int sph_slab_patch_halo(sph_handle *h, int buf, int i_begin, int i_end, int n_all, void *hip_stream);
/* SPH_SWEEP_LIST: the interleaved (pos4, vel4) records of the sorted rows (32 bytes per row, row r at
 * byte 32 r; device pointer, NULL for the other sweeps).  The density sweep leaves rho in the record, so
 * the driver can send a boundary layer's records straight into the neighbour's halo rows (exchange B)
 * instead of sending vel4 rows and patching them in (sph_slab_patch_halo). */
void *sph_slab_records(sph_handle *h);
/* kernelMoveParticles (simulator.cu:329-367) for one slab: the impulse of sph_apply_click on the
 * z-layers [z_lo, z_hi) this slab owns, applied to the NEW state (buffer `buf`: the rows the last
 * sph_slab_force* launch wrote, still in that step's sorted order) through the cell table of that
 * step's sort -- the pre-integration grid, like the reference (simulator.cu:482-489). */
int sph_slab_apply_click(sph_handle *h, int buf, int mouse_x, int mouse_y, int z_lo, int z_hi);
/* rows [a0, b0) and [a1, b1) (either may be empty; a1 >= b0) of the owned range, in ONE
 * launch; hip_stream NULL = the handle's stream. */
int sph_slab_force_ranges(sph_handle *h, int buf, int i_origin, int a0, int b0, int a1, int b1,
                          int n_all, int last_launch_of_the_step, void *hip_stream);

/* ---- the visualiser's frame (display.cpp:35-90), drawn on the device ----
 * The scene is display.cpp's: glFrustum(-2, 2, -2, 2, 1, 100) x glTranslatef(-5, -5, -15), identity
 * model-view, the 12 edges of the box [0, 10]^3 in white, the particles as square points.  GL leaves
 * rasterisation to the implementation; this one is fixed to the bit: all fp32,
 * w = 15 - z, xw = ((0.5 (x - 5)) / w + 1) (0.5 W), column floor(xw), row (H - 1) - floor(yw) -- row 0
 * is the TOP of the window, so sph_apply_click(h, x, y) addresses pixel (x, y) of this image.  Per pixel
 * the library keeps the minimum depth (the bits of w) and the number of covering particles; the frame
 * is RGB8, row 0 first: white where a box edge is not behind the nearest particle, else the particle
 * colour, else black. */
enum {
    SPH_SHADE_FLAT = 0, /* the reference's: every particle pixel (0, 0, 255) */
    SPH_SHADE_COUNT = 1 /* (32 L, 32 L, 255), L = min(7, floor(log2(covering particles))) */
};
typedef struct SphRenderOptions {
    int32_t struct_size;   /* = sizeof(SphRenderOptions) */
    int32_t width, height; /* 0 = 800 x 600; at most 4096 x 4096 */
    int32_t point_size;    /* 0 = 3; odd, 1..9 */
    int32_t shade;         /* SPH_SHADE_* */
} SphRenderOptions;
/* Draws the state the handle holds NOW (after sph_step the positions sph_positions_host would return;
 * sph_apply_click changes velocities only; after sph_setup / sph_upload_state / sph_load_state the
 * uploaded state) and queues the copy of the frame to pinned host memory.  opt == NULL: display.cpp's
 * 800 x 600, points of size 3, flat blue.  Reads the device-resident particle stream, never the
 * id-ordered read-back: works with SPH_FLAG_NO_READBACK.  Queued on the handle's streams; does not
 * block.  Before any state, and for SPH_FLAG_EXTERNAL_STATE handles (slabs): SPH_ESTATE.  Bad sizes,
 * an even point_size, an unknown shade: SPH_EINVAL.  With SPH_SWEEP_LINKED the frame is drawn from the
 * particle-id-ordered state array that backend keeps (same image, no cell-sorted stream to exploit).
 * SPH_RENDER_PLAIN=1 in the environment selects the check path of the splat (one global atomic per
 * covered pixel and particle; identical buffers). */
int sph_render_frame(sph_handle *h, const SphRenderOptions *opt);
/* width x height x 3 bytes of the last sph_render_frame, owned by the handle, valid until the next
 * render.  Blocks until the copy has landed.  NULL before the first render. */
const uint8_t *sph_frame_host(sph_handle *h, int *width, int *height);
/* The buffers behind the last frame, width x height each, row 0 first; any pointer may be NULL.
 * depth_bits: minimum over covering particles of the bit pattern of w (0xFFFFFFFF = empty); count:
 * covering particles; edge_depth_bits: the static box-edge layer (0xFFFFFFFF = no edge). */
int sph_download_frame_buffers(sph_handle *h, uint32_t *depth_bits, uint32_t *count, uint32_t *edge_depth_bits);
/* GPU time of clear + splat + compose (HIP events on the compute stream), summed over `frames` renders. */
int sph_get_render_time(sph_handle *h, double *seconds, int64_t *frames, int reset);
/* SPH_API_VERSION of the library that is actually loaded. */
int sph_api_version(void);

/* ---- the field frame: the same picture, the particles coloured by a field of the nearest one ----
 * Additive to version 3: test for SPH_HAS_FIELD_FRAME.  Defined to the bit in DESIGN.md section 10 ("The field
 * frame").  The scalar s of a particle comes from the values sph_download_state returns for it, all fp32, every
 * operation rounded on its own: SPEED sqrtf((vx vx + vy vy) + vz vz), DENSITY rho, PRESSURE
 * fmaxf(0, GAS_CONSTANT (rho - REST_DENSITY)).  Per pixel the library keeps the minimum over the covering
 * particles of the 64-bit word (bits(w) << 32) | bits(s): the nearest particle, among several at the same depth
 * the one with the smallest s.  q = (int)fminf(fmaxf(floorf(((s - lo) / (hi - lo)) * 256), 0), 255), q = 0 where
 * hi == lo or the quotient is NaN; the colour runs blue - cyan - green - yellow - red over q = 0..255.  Box edges
 * and empty pixels as in sph_render_frame; depth and count buffers are those sph_render_frame produces. */
#define SPH_HAS_FIELD_FRAME 1
enum {
    SPH_FIELD_SPEED = 0,
    SPH_FIELD_DENSITY = 1,
    SPH_FIELD_PRESSURE = 2
};
typedef struct SphFieldFrameOptions {
    int32_t struct_size;   /* = sizeof(SphFieldFrameOptions) */
    int32_t width, height; /* 0 = 800 x 600; at most 4096 x 4096 */
    int32_t point_size;    /* 0 = 3; odd, 1..9 */
    int32_t field;         /* SPH_FIELD_* */
    float value_lo;        /* the colour scale runs from value_lo (blue) to value_hi (red); both 0: the minimum */
    float value_hi;        /* and maximum of s over ALL particles of this frame, reduced on the device */
} SphFieldFrameOptions;
/* sph_render_frame's queueing, streams and state rules (SPH_ESTATE before any state and for
 * SPH_FLAG_EXTERNAL_STATE handles; works with SPH_FLAG_NO_READBACK; with SPH_SWEEP_LINKED drawn from the arrays
 * sph_download_state reads; SPH_RENDER_PLAIN=1 selects the check path).  opt == NULL: 800 x 600, points of size
 * 3, speed, automatic range.  An unknown field, a non-finite value_lo / value_hi, value_hi < value_lo:
 * SPH_EINVAL.  Does not block: the automatic range stays on the device, where the compose reads it.
 * sph_frame_host and sph_download_frame_buffers serve the last frame of either kind; sph_get_render_time counts
 * both kinds. */
int sph_render_field(sph_handle *h, const SphFieldFrameOptions *opt);
/* The low words behind the last field frame, width x height, row 0 first: the bits of s of the particle that
 * colours the pixel, 0xFFFFFFFF where no particle covers it.  SPH_ESTATE if the last render was not a field frame. */
int sph_download_field_buffer(sph_handle *h, uint32_t *value_bits);
/* The range the last field frame used (the options' or the reduced one).  Blocks until it is on the host.
 * SPH_ESTATE if the last render was not a field frame. */
int sph_field_range(sph_handle *h, float *lo, float *hi);

/* ---- the column-density frame: how much fluid lies behind each pixel ----
 * Additive to version 3: test for SPH_HAS_COLUMN_FRAME.  Defined to the bit in DESIGN.md section 10h ("The column
 * frame"); all fp32, every operation rounded on its own.  The camera is sph_render_frame's.  Through the centre of
 * every pixel runs a ray from the eye; a particle whose squared distance b2 to that ray is below h h adds
 * c = MASS coeff (32/35) a^7, a2 = h h - b2: the line integral of its poly6 kernel along the ray, in closed form.  The
 * term is the unsigned 64-bit integer (uint64)(c 2^32), 2^52 where c >= 2^20, 0 where c is NaN or negative; a pixel's
 * column word is the sum of the terms of ALL particles modulo 2^64, so it depends on the set of rows only.  Value of a
 * pixel: (float)word 2^-32.  Colour: the field frame's quantiser over value_lo .. value_hi, then an integer ramp from a
 * thin film (223, 239, 255) to deep water (0, 48, 128); word 0: black; white wherever the box-edge layer has a sample
 * (the fluid is translucent: no depth test).  The image is point-sampled: a particle whose footprint holds no pixel
 * centre adds nothing. */
#define SPH_HAS_COLUMN_FRAME 1
typedef struct SphColumnFrameOptions {
    int32_t struct_size;   /* = sizeof(SphColumnFrameOptions) */
    int32_t width, height; /* 0 = 800 x 600; at most 4096 x 4096 */
    float value_lo;        /* the colour scale runs from value_lo to value_hi; both 0: from 0 to the largest */
    float value_hi;        /* column of this frame, reduced on the device */
} SphColumnFrameOptions;
/* sph_render_frame's queueing, streams and state rules (SPH_ESTATE before any state and for
 * SPH_FLAG_EXTERNAL_STATE handles; works with SPH_FLAG_NO_READBACK, every sweep and both key orders; needs no grid
 * and builds none; SPH_RENDER_PLAIN=1 selects the check path, one global atomic per particle and pixel).
 * opt == NULL: 800 x 600, automatic range.  A bad size, a non-finite value_lo / value_hi, value_hi < value_lo:
 * SPH_EINVAL.  Does not block.  sph_frame_host serves the RGB and sph_get_render_time counts the frame;
 * sph_download_frame_buffers (a column frame writes no depth or count), sph_download_field_buffer and sph_field_range
 * return SPH_ESTATE after it.  A flat or field frame rendered afterwards is what it would have been without it. */
int sph_render_column(sph_handle *h, const SphColumnFrameOptions *opt);
/* The column words behind the last column frame, width x height, row 0 first (value = word 2^-32, 0 = no particle
 * reaches the ray).  SPH_ESTATE if the last render was not a column frame. */
int sph_download_column_buffer(sph_handle *h, uint64_t *column_words);
/* The range the last column frame used (the options', or 0 and the value of its largest word).  Blocks until it is
 * on the host.  SPH_ESTATE if the last render was not a column frame. */
int sph_column_range(sph_handle *h, float *lo, float *hi);

/* ---- the liquid frame: the fluid as a shaded water surface ----
 * Additive to version 3: test for SPH_HAS_LIQUID_FRAME.  Defined to the bit in DESIGN.md section 10i ("The liquid
 * frame"); all fp32, every operation rounded on its own, nothing but + - x / sqrtf, comparisons and selects.  The camera
 * and the pixel rays are the column frame's.  Every particle is a sphere of `radius`; per pixel the library keeps the
 * smallest depth at which the pixel's ray enters a sphere at or behind the near plane (the front buffer, the bits of
 * wf, 0xFFFFFFFF where there is none) and the column frame's word.  The front buffer is smoothed `smooth_iterations`
 * times by a bilateral filter over (2 smooth_radius + 1)^2 pixels that ignores neighbours further than
 * smooth_depth away in depth, so silhouettes stay sharp; normals come from one-sided differences of the smoothed
 * view-space points; the colour is a diffuse and a specular term, a Fresnel blend to a sky colour and a per-channel
 * absorption by the column behind the pixel on the scale of thickness_scale.  RGB8, row 0 first: white where a box
 * edge is not behind the (unsmoothed) front, else the water colour, else black. */
#define SPH_HAS_LIQUID_FRAME 1
typedef struct SphLiquidFrameOptions {
    int32_t struct_size;       /* = sizeof(SphLiquidFrameOptions) */
    int32_t width, height;     /* 0 = 800 x 600; at most 4096 x 4096 */
    float radius;              /* of the spheres; 0 = h of the handle, else 0 < radius <= h */
    int32_t smooth_iterations; /* 0 = 3; -1 = none; at most 8 */
    int32_t smooth_radius;     /* k, in pixels; 0 = 3; -1 = a window of the pixel alone, which smooths nothing; at most 7 */
    float smooth_depth;        /* neighbours this far away in depth or further add nothing; 0 = 2 radius; > 0, finite */
    float light[3];            /* the direction towards the light in view space; all 0 = (-0.35, 0.8, 0.5); finite */
    float thickness_scale;     /* the column value that counts as optical depth 1; 0 = the frame's largest column, */
                               /* reduced on the device; >= 0, finite */
} SphLiquidFrameOptions;
/* sph_render_column's queueing, streams and state rules, SPH_RENDER_PLAIN=1 included.  opt == NULL: every default.
 * A bad size, radius, count, smooth_depth, light or thickness_scale: SPH_EINVAL.  Does not block.  sph_frame_host
 * serves the RGB and sph_get_render_time counts the frame; sph_download_frame_buffers, sph_download_field_buffer,
 * sph_field_range, sph_download_column_buffer and sph_column_range return SPH_ESTATE after it.  A flat, field or column
 * frame rendered afterwards is what it would have been without it. */
int sph_render_liquid(sph_handle *h, const SphLiquidFrameOptions *opt);
/* The buffers behind the last liquid frame, each width x height, row 0 first, each may be NULL: the front words, the
 * bits of the smoothed depth (0xFFFFFFFF = empty in both), the unit normals as 3 floats per pixel (0, 0, 0 where
 * empty) and the column words (those sph_render_column gives for the same state).  SPH_ESTATE if the last render was
 * not a liquid frame. */
int sph_download_liquid_buffers(sph_handle *h, uint32_t *front_bits, uint32_t *smooth_depth_bits, float *normals_xyz,
                                uint64_t *column_words);

/* ---- the field sample: SPH-interpolated density, speed or pressure on a regular lattice ----
 * Additive to version 3: test for SPH_HAS_FIELD_SAMPLE.  Defined to the bit in DESIGN.md section 10b ("The field
 * sample"); all fp32, every operation rounded on its own, in both math modes.  Point (ix, iy, iz) lies at
 * origin + (float)i * spacing per axis and lands at index (iz ny + iy) nx + ix.  Its cell is (int)(p / h) per axis;
 * a point with !(p >= 0) or a cell >= numCellsPerDim on any axis is outside and samples +0.  The walk is the density
 * sweep's: the 27 cells dz, dy, dx = -1..1 in that nesting, each cell's rows in the order of the grid's sorted
 * stream; candidate j with d2 = (dx dx + dy dy) + dz dz <= h h weighs m = MASS (((d_kernel_coeff diff) diff) diff),
 * diff = h h - d2.  DENSITY: the sum of m from 0 (no EPS_F clamp: empty space is 0) -- what kernelUpdatePressureAndDensity
 * forms for a particle at that point.  SPEED, PRESSURE: sum(m a_j) / sum(m), 0 where sum(m) is not > 0, a_j the field
 * frame's scalar of row j (from the values sph_download_state returns). */
#define SPH_HAS_FIELD_SAMPLE 1
typedef struct SphSampleLattice {
    int32_t struct_size;     /* = sizeof(SphSampleLattice) */
    int32_t nx, ny, nz;      /* each 1..4096, nx*ny*nz <= 1<<24 */
    float origin[3];
    float spacing[3];        /* finite, > 0 */
    int32_t field;           /* SPH_FIELD_* */
} SphSampleLattice;
/* Samples the state the handle holds NOW and queues the copy of the values to pinned host memory; does not block.
 * The walk needs a grid of that state.  With a grid phase done (sph_phase_grid, or the grid a timed step built
 * ahead) that grid is used as it is.  Otherwise the grid is built here exactly as a timed sph_step builds the next
 * step's grid ahead: the next step, timed or not, consumes it, and a click, upload or load drops it; no result of
 * any step changes.  sph_download_grid after the call returns the grid that was walked.  SPH_ESTATE: before any
 * state, inside a step split into phases (after sph_phase_density or sph_phase_force), for SPH_FLAG_EXTERNAL_STATE
 * handles, with SPH_SWEEP_LINKED (no cell table) and with SPH_KEY_MORTON (a row of cells is not one run of the
 * stream).  SPH_EINVAL: struct_size not set, dimensions out of range, a non-finite origin, a spacing that is not
 * finite and > 0, an unknown field.  No particles: all zeros.  Results only: the sampling kernel runs on the compute
 * stream behind the grid build whose events the next step takes over, so that step's SphKernelTimes.density, and
 * SphTimes.sphUpdate of a timed step, include the GPU time of every sample taken before it (as they include a frame
 * rendered behind a grid built ahead); sph_get_sample_time says how much that was.  SPH_SAMPLE_PLAIN=1 in the environment selects the
 * check path (one thread per point, every candidate loaded from global memory; identical values). */
int sph_sample_field(sph_handle *h, const SphSampleLattice *lat);
/* nx*ny*nz floats of the last sph_sample_field, owned by the handle, valid until the next sample.  Blocks until
 * the copy has landed.  NULL before the first sample. */
const float *sph_sample_host(sph_handle *h, int *nx, int *ny, int *nz);
/* GPU time of the sampling kernel alone (HIP events on the compute stream; not the grid build, which belongs to
 * the step that consumes it), summed over `samples` calls. */
int sph_get_sample_time(sph_handle *h, double *seconds, int64_t *samples, int reset);

/* ---- the surface mesh: the density iso-surface as an indexed triangle mesh, extracted on the device ----
 * Additive to version 3: test for SPH_HAS_SURFACE.  Defined to the bit in DESIGN.md section 10d ("The surface
 * mesh"): marching tetrahedra over the values sph_sample_field returns for SPH_FIELD_DENSITY on the same lattice.
 * A point is inside when f >= iso.  Every point owns up to seven edges, towards (1,0,0) (0,1,0) (0,0,1) (1,1,0)
 * (1,0,1) (0,1,1) (1,1,1); an edge whose ends differ carries one vertex at p_a + t (p_b - p_a), t = (iso - f_a) /
 * (f_b - f_a), a the owner, all fp32 and rounded on their own.  Vertices are numbered by owner L = (iz ny + iy) nx + ix,
 * then direction; triangles by cell L, then by the six tetrahedra of the cell, wound so that normals point out of
 * the fluid.  Degenerate triangles (f == iso at a point) stay.  The mesh is closed when the lattice's outer shell
 * is outside the fluid, open where the surface leaves the lattice. */
#define SPH_HAS_SURFACE 1
typedef struct SphSurfaceOptions {
    int32_t struct_size;     /* = sizeof(SphSurfaceOptions) */
    int32_t nx, ny, nz;      /* each 2..4096, nx*ny*nz <= 1<<24 */
    float origin[3];         /* finite */
    float spacing[3];        /* finite, > 0 */
    float iso;               /* finite, > 0 */
} SphSurfaceOptions;
/* Extracts the surface of the state the handle holds NOW and queues the copy of the mesh to pinned host memory.
 * State rules, grid handling and error codes are sph_sample_field's: the grid is found or built ahead in the same
 * way (sph_download_grid returns the one that was walked) and no result of any step depends on the call;
 * SPH_ESTATE before any state, inside an open phase-split step, for a handle in slab mode and with
 * SPH_SWEEP_LINKED / SPH_KEY_MORTON; SPH_EINVAL for a NULL opt, struct_size not set, dimensions out of range, a
 * non-finite origin, a spacing that is not finite and > 0, an iso that is not finite and > 0.  The values of the
 * last sph_sample_field are left alone: the surface samples into a buffer of its own.
 * Unlike sph_sample_field the call waits on the host once, for the two totals (16 bytes), to size the mesh; the
 * device and pinned buffers grow on demand; then it queues the emit and the copy and returns.  No particles, or no
 * edge that crosses iso: 0 vertices, 0 triangles, SPH_OK.  SPH_SURFACE_PLAIN=1 in the environment selects the check
 * path for the sample and the extraction (one thread per point, every corner loaded from global memory; the same
 * mesh). */
int sph_extract_surface(sph_handle *h, const SphSurfaceOptions *opt);
/* The mesh of the last sph_extract_surface: 3 floats per vertex, 3 vertex indices per triangle, owned by the handle,
 * valid until the next extraction.  Blocks until the copy has landed.  Any out-pointer may be NULL; with 0 vertices
 * (triangles) the pointer returned may be NULL.  SPH_ESTATE before the first extraction. */
int sph_surface_host(sph_handle *h, const float **vertices_xyz, int64_t *num_vertices,
                     const uint32_t **triangles, int64_t *num_triangles);
/* GPU time of the surface's sampling kernel and of its count + scan + emit launches (HIP events on the compute
 * stream), summed over `calls` extractions. */
int sph_get_surface_time(sph_handle *h, double *sample_seconds, double *extract_seconds, int64_t *calls, int reset);

/* ---- run diagnostics: exact sums, extrema and a histogram of the state, reduced on the device ----
 * Additive to version 3: test for SPH_HAS_DIAGNOSTICS.  Defined to the bit in DESIGN.md section 10c ("Diagnostics").
 * The rows are those sph_render_field reads, (x, y, z, vx, vy, vz, rho) per particle as sph_download_state returns
 * them; speed and prs are the field frame's scalars.  Every sum is a sum of signed 64-bit Q32.32 terms
 * q(t) = (int64)floor(t 2^32) of the double t (NaN: 0; t >= 2^31: INT64_MAX; t < -2^31: INT64_MIN; `saturated` counts
 * the terms that took one of those three branches), accumulated in integers only and reported as a 128-bit two's
 * complement value: the words depend on the SET of rows, not on their order, the launch shape or the number of slabs.
 * The term of the first eight sums is the fp32 value widened to double, that of V2 is ((double)vx vx + (double)vy vy)
 * + (double)vz vz.  Extrema are fp32 bit patterns ordered by the key b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000):
 * -0 < +0, a NaN sorts where its bits put it; no rows: min_bits = 0x7F800000, max_bits = 0xFF800000. */
#define SPH_HAS_DIAGNOSTICS 1
enum { /* indices of SphDiagnosticsRaw.sum */
    SPH_DIAG_SUM_X = 0, SPH_DIAG_SUM_Y = 1, SPH_DIAG_SUM_Z = 2,
    SPH_DIAG_SUM_VX = 3, SPH_DIAG_SUM_VY = 4, SPH_DIAG_SUM_VZ = 5,
    SPH_DIAG_SUM_RHO = 6, SPH_DIAG_SUM_PRS = 7, SPH_DIAG_SUM_V2 = 8,
    SPH_DIAG_SUMS = 9
};
enum { /* indices of SphDiagnosticsRaw.min_bits / max_bits */
    SPH_DIAG_EXT_X = 0, SPH_DIAG_EXT_Y = 1, SPH_DIAG_EXT_Z = 2,
    SPH_DIAG_EXT_SPEED = 3, SPH_DIAG_EXT_RHO = 4, SPH_DIAG_EXT_PRS = 5,
    SPH_DIAG_EXTREMA = 6
};
#define SPH_DIAG_BINS 256
typedef struct SphSum128 { /* lo + 2^64 hi: a two's complement sum of Q32.32 terms; its value is that times 2^-32 */
    uint64_t lo;
    int64_t hi;
} SphSum128;
typedef struct SphDiagnosticsOptions {
    int32_t struct_size; /* = sizeof(SphDiagnosticsOptions) */
    int32_t hist_field;  /* SPH_FIELD_* of the histogram, -1 = none */
    float value_lo;      /* the 256 bins are the field frame's q over value_lo .. value_hi; both 0: the minimum and */
    float value_hi;      /* maximum (by the key above) of the scalar over this call's rows, taken on the device */
} SphDiagnosticsOptions;
typedef struct SphDiagnosticsRaw {
    int32_t struct_size; /* = sizeof(SphDiagnosticsRaw) */
    int32_t pad_;        /* 0 */
    int64_t n;           /* rows */
    SphSum128 sum[SPH_DIAG_SUMS];
    uint32_t min_bits[SPH_DIAG_EXTREMA];
    uint32_t max_bits[SPH_DIAG_EXTREMA];
    uint64_t saturated;
    int32_t hist_field;    /* -1: no histogram (hist is all zero, the range words are 0) */
    uint32_t hist_lo_bits; /* the range the bins were cut over (the options' or the reduced one), fp32 bit patterns */
    uint32_t hist_hi_bits;
    int32_t pad2_;         /* 0 */
    uint64_t hist[SPH_DIAG_BINS];
} SphDiagnosticsRaw;
/* The derived values (DESIGN.md section 10c gives every expression; Python floats reproduce them bit for bit). */
typedef struct SphDiagnostics {
    int32_t struct_size; /* = sizeof(SphDiagnostics) */
    int32_t pad_;
    int64_t n;
    double mass;         /* n MASS */
    double com[3];       /* centre of mass; 0 without rows, like every quotient by n */
    double momentum[3];  /* MASS sum(v) */
    double kinetic;      /* 0.5 MASS sum(v^2) */
    double potential;    /* MASS 9.8 sum(y) (the constant is -GRAVITY) */
    double mean_rho, mean_prs;
    double min_rho, max_rho;
    double max_speed;
    double cfl;          /* max_speed timestep / h */
    double box_min[3], box_max[3]; /* the box of the particles */
    uint64_t saturated;
} SphDiagnostics;
/* Queues the reduction of the state the handle holds NOW (the rows sph_render_field reads), the optional histogram
 * behind it and the copy of the small result block to pinned memory, on the handle's streams; does not block.
 * opt == NULL: no histogram.  State rules of sph_render_field: SPH_ESTATE before any state and for
 * SPH_FLAG_EXTERNAL_STATE handles; works with SPH_FLAG_NO_READBACK, with every sweep (SPH_SWEEP_LINKED included)
 * and both key orders, between the phases of a split step too: it needs no grid and builds none, and no result of
 * any step changes.  SPH_EINVAL: an unknown hist_field, and with a histogram a non-finite value_lo / value_hi or
 * value_hi < value_lo.  SPH_DIAG_PLAIN=1 in the environment selects the check path (one thread per row, every term a
 * global integer atomic; identical words). */
int sph_diagnose(sph_handle *h, const SphDiagnosticsOptions *opt);
/* The words of the last sph_diagnose / sph_slab_diagnose.  Blocks until the copy has landed.  SPH_ESTATE before the
 * first one. */
int sph_diagnostics_host(sph_handle *h, SphDiagnosticsRaw *out);
/* Pure host code, no GPU and no handle: the derived values of `raw` for a run with `settings` (h, timestep). */
int sph_diagnostics_values(const SphDiagnosticsRaw *raw, const SphSettings *settings, SphDiagnostics *out);
/* Pure host code: merges `part` into `into` -- 128-bit adds, key-ordered minima and maxima, histogram adds -- the way
 * slabs, and the ranks of a one-process-per-GPU run, combine.  SPH_EINVAL when the two histogram fields or ranges
 * differ. */
int sph_diagnostics_add(SphDiagnosticsRaw *into, const SphDiagnosticsRaw *part);
/* GPU time of the diagnostics launches (HIP events on the compute stream), summed over `calls` calls. */
int sph_get_diagnostics_time(sph_handle *h, double *seconds, int64_t *calls, int reset);
/* The same kernels over the rows [i_begin, i_end) of buffer pair `buf` of a slab handle, on the handle's stream; read
 * the result with sph_diagnostics_host.  An automatic histogram range is SPH_EINVAL: a slab cannot know the global
 * range. */
int sph_slab_diagnose(sph_handle *h, int buf, int i_begin, int i_end, const SphDiagnosticsOptions *opt);

/* ---- passive tracers: points the caller seeds, carried by the interpolated velocity field step after step ----
 * Additive to version 3: test for SPH_HAS_TRACERS.  Defined to the bit in DESIGN.md section 10e ("Tracers"); all
 * fp32, every operation rounded on its own, in both math modes.  A handle holds m tracers, 0 <= m <= 1 << 24, in
 * the caller's order, each with a position p, the velocity u and the density sum den sampled by the last advect.
 * Cell, outside rule and walk are the field sample's (above).  Candidate j with d2 <= h h weighs
 * m_j = MASS (((d_kernel_coeff diff) diff) diff), diff = h h - d2; den = sum(m_j) and n = sum(m_j v_j) per axis,
 * all from +0, v_j the velocity sph_download_state returns for row j.  u = n / den per axis where den > 0, else +0.
 * Where den > 0 and dt != 0 the tracer moves to p + u dt (one multiply, one add per axis); everywhere else -- an
 * outside tracer, a NaN, empty space, dt == 0 -- its three position words are copied unchanged.  Tracers are not
 * reflected at the walls and carry no mass: one that leaves the grid is outside from the next call on and stays.
 * Tracers belong to the caller, not to the state: sph_setup, sph_upload_state and sph_load_state leave them alone,
 * and sph_save_state does not store them. */
#define SPH_HAS_TRACERS 1
/* Replaces the handle's tracers by m points (x, y, z interleaved; any float values; m == 0 clears them).
 * SPH_EINVAL: m < 0, m > 1 << 24, a NULL pos_xyz with m > 0.  SPH_ESTATE for SPH_FLAG_EXTERNAL_STATE handles.
 * Blocks until the points are on the device. */
int sph_tracers_set(sph_handle *h, const float *pos_xyz, int m);
/* One explicit Euler move of every tracer through the velocity field of the state the handle holds NOW.
 * dt == 0 samples without moving.  Queues the kernels and the copy of the results; does not block.
 * State rules, grid handling and error codes are sph_sample_field's: the grid is found (phase 1) or built ahead
 * (phase 0), the next step consumes it, a click, upload or load drops it, and no result of any step changes.
 * SPH_ESTATE before any state, inside an open phase-split step, for SPH_FLAG_EXTERNAL_STATE handles, with
 * SPH_SWEEP_LINKED and with SPH_KEY_MORTON.  SPH_EINVAL: a dt that is not finite.  No tracers set: SPH_OK, nothing
 * happens.  No particles: every tracer gets den = u = +0 and keeps its words.  SPH_TRACER_PLAIN=1 in the environment
 * selects the check path (one thread per tracer in caller order, every candidate loaded from global memory;
 * identical words). */
int sph_tracers_advect(sph_handle *h, float dt);
/* m x 4 floats each, owned by the handle, valid until the next advect or set.
 * pos_den = (x, y, z, den): den was sampled at the position before the move.  vel = (ux, uy, uz, +0).
 * Blocks until the copy has landed.  Before the first advect after a set: the positions as set, den = u = +0.
 * Any out-pointer may be NULL; with no tracers the pointers returned may be NULL and *m is 0. */
int sph_tracers_host(sph_handle *h, const float **pos_den, const float **vel, int *m);
typedef struct SphTracerStats {
    int32_t struct_size, pad_;  /* sizeof(SphTracerStats), 0: both written by the call */
    int64_t calls;              /* advects that ran kernels (either path) */
    uint64_t waves_shared;      /* waves of 64 sorted tracers that walked their groups' candidates from LDS ... */
    uint64_t waves_direct;      /* ... and waves that held too many groups and walked lane by lane */
    uint64_t groups;            /* distinct (row of cells, block of 8 cells in x) groups, summed over the waves */
    double seconds;             /* GPU time of key + sort + walk (HIP events on the compute stream) */
} SphTracerStats;
/* Sums since create or since the last reset; the three counters are what the walk kernel counted (the check path
 * counts none).  Blocks. */
int sph_get_tracer_stats(sph_handle *h, SphTracerStats *out, int reset);

/* ---- derived per-particle fields: vorticity, divergence, density gradient and neighbour count ----
 * Additive to version 3: test for SPH_HAS_DERIVED.  Defined to the bit in DESIGN.md section 10f ("Derived fields");
 * all fp32, every operation rounded on its own, in both math modes.  Row i of the grid's sorted stream walks the
 * density sweep's candidates (its own cell clamped into the grid, the 27 cells around it in dz, dy, dx order, each
 * cell's rows in stream order, itself included).  With e = p_j - p_i, u = v_j - v_i (the words sph_download_state
 * returns), d2 = (ex ex + ey ey) + ez ez, candidate j is taken unless d2 > h h; then diff = h h - d2,
 * a = (d_kernel_coeff diff) diff, m = MASS (a diff), w = MASS a, and from +0:
 *   rho += m;  g += w e (per axis);  s += w ((ux ex + uy ey) + uz ez);  c += w (e x u) (per axis);  count += 1.
 * grad_rho = 6 g, divergence = (6 s) / rho, vorticity = (6 c) / rho per axis; where rho is not > 0 the last two are
 * +0.  rho is this walk's own sum without the EPS_F clamp: the call works before the first step, and the density the
 * next step's sweep stores is max(rho, EPS_F). */
#define SPH_HAS_DERIVED 1
/* Queues the sweep over the particles of the state the handle holds NOW and the copies of its results; does not
 * block.  State rules and grid handling are sph_tracers_advect's: the grid is found (phase 1) or built ahead
 * (phase 0), the next step consumes it, a click, upload or load drops it, and no result of any step changes; the
 * sweep's GPU time lands in that step's SphKernelTimes.density.  SPH_ESTATE before any state, inside an open
 * phase-split step, for SPH_FLAG_EXTERNAL_STATE handles, with SPH_SWEEP_LINKED and with SPH_KEY_MORTON.  No
 * particles: SPH_OK, n = 0.  SPH_DERIVE_PLAIN=1 in the environment selects the check path (one thread per row, every
 * candidate loaded from global memory; identical words). */
int sph_derive(sph_handle *h);
/* The results of the last sph_derive in particle-id order, owned by the handle, valid until the next sph_derive:
 * vort_div = n x (wx, wy, wz, divergence), grad_rho = n x (gx, gy, gz, rho), neighbours = n counts.  Blocks until the
 * copies have landed.  Any out-pointer may be NULL; with n == 0 the pointers returned may be NULL.  SPH_ESTATE
 * before the first sph_derive. */
int sph_derived_host(sph_handle *h, const float **vort_div, const float **grad_rho, const uint32_t **neighbours, int *n);
typedef struct SphDeriveStats {
    int32_t struct_size, pad_;  /* sizeof(SphDeriveStats), 0: both written by the call */
    int64_t calls;              /* derives that ran a kernel (either path) */
    uint64_t runs_staged;       /* non-empty runs (of nine per wave of 64 rows) the default path walked from LDS ... */
    uint64_t runs_direct;       /* ... and runs longer than the LDS slice, walked from global memory */
    double seconds;             /* GPU time of the sweep (HIP events on the compute stream) */
} SphDeriveStats;
/* Sums since create or since the last reset; the two counters are what the default path's kernel counted (the check
 * path counts none).  Blocks. */
int sph_get_derive_stats(sph_handle *h, SphDeriveStats *out, int reset);

/* ---- bodies: the connected pieces of fluid (droplets, sheets) and the piece every particle belongs to ----
 * Additive to version 3: test for SPH_HAS_BODIES.  Defined to the bit in DESIGN.md section 10g ("Bodies"); all fp32,
 * every operation rounded on its own, in both math modes.  With r2 = link link, two particles i != j are linked when
 * d2 <= r2, e = p_j - p_i (the words sph_download_state returns), d2 = (ex ex + ey ey) + ez ez; a NaN d2 is no link.
 * A body is a connected component of that graph, its label the smallest particle id in it; a particle without a
 * link is a body of one.  Every result is an integer reduced by commutative operations: the same words for any
 * schedule, kernel path or sweep backend. */
#define SPH_HAS_BODIES 1
typedef struct SphBodyOptions {
    int32_t struct_size;        /* sizeof(SphBodyOptions) */
    float link;                 /* link length: 0 = h, else finite with 0 < link <= h */
} SphBodyOptions;
/* Labels the bodies of the state the handle holds NOW.  opt == NULL: link = h.  State rules, grid handling and error
 * codes are sph_derive's: the grid is found (phase 1) or built ahead (phase 0), the next step consumes it and no
 * result of any step changes; SPH_ESTATE before any state, inside an open phase-split step, for
 * SPH_FLAG_EXTERNAL_STATE handles, with SPH_SWEEP_LINKED and with SPH_KEY_MORTON; SPH_EINVAL for an unset struct_size
 * and for a link that is not finite, negative or greater than h.  No particles: SPH_OK, no bodies.  Like
 * sph_extract_surface the call waits on the host once, for the number of bodies, which sizes the table; the table's
 * kernels and the copies are queued and the call returns.  SPH_BODIES_PLAIN=1 in the environment selects the check
 * path (min-label propagation, one thread per row, repeated until nothing changes; identical words).  SPH_EHIP, and no
 * results, if a bounded loop of the default path ran out of trips (SphBodyStats.gave_up; never with a correct kernel). */
int sph_label_bodies(sph_handle *h, const SphBodyOptions *opt);
/* The results of the last sph_label_bodies, owned by the handle, valid until the next one: labels = n words in
 * particle-id order; table = num_bodies rows of 8 words in ascending label order: label, count, the bounding box's
 * minimum x y z and maximum x y z as fp32 bit patterns (extrema by the diagnostics' ordering key); largest = the label
 * of the body with the greatest count, the smallest such label on a tie (0 without particles).  Blocks until the
 * copies have landed.  Any out-pointer may be NULL; pointers returned for empty results may be NULL.  SPH_ESTATE before
 * the first sph_label_bodies. */
int sph_bodies_host(sph_handle *h, const uint32_t **labels, int *n, const uint32_t **table, int *num_bodies, uint32_t *largest);
typedef struct SphBodyStats {
    int32_t struct_size, pad_;  /* sizeof(SphBodyStats), 0: both written by the call */
    int64_t calls;              /* labellings that ran a kernel (either path) */
    uint64_t links;             /* unordered linked pairs found (exact) */
    uint64_t unions;            /* successful merges: n - num_bodies, whatever the schedule */
    uint64_t rounds;            /* sweeps the check path needed (the default path: 0) */
    uint64_t gave_up;           /* lanes of the default path that left a bounded loop at its bound: always 0 */
    double seconds;             /* GPU time of the kernels (HIP events on the compute stream) */
} SphBodyStats;
/* Sums since create or since the last reset.  Blocks. */
int sph_get_body_stats(sph_handle *h, SphBodyStats *out, int reset);

/* ---- per-body moments: mass, momentum, spin and shape of every body ----
 * Additive to version 3: test for SPH_HAS_BODY_MOMENTS.  Defined to the bit in DESIGN.md section 10k ("Body
 * moments").  The join of the bodies and the diagnostics: per body of sph_label_bodies, eighteen sums of the
 * diagnostics' Q32.32 terms q(t) over the body's rows (the rows sph_download_state returns), integers only, with the
 * diagnostics' NaN and saturation rules, reported as SphSum128.  Sums 0-8 are SPH_DIAG_SUM_*, same indices, same
 * terms.  The term of XX .. YZ is (double)a (double)b, exact in fp64; that of LX is (double)y vz - (double)z vy, of LY
 * (double)z vx - (double)x vz, of LZ (double)x vy - (double)y vx: both products exact, one rounding, by the
 * subtraction.  The words depend on the set of rows of each body only: the same for any schedule, kernel path or sweep
 * backend. */
#define SPH_HAS_BODY_MOMENTS 1
enum { /* indices of SphBodyMomentsRaw.sum beyond SPH_DIAG_SUM_* */
    SPH_BODY_SUM_XX = 9, SPH_BODY_SUM_YY = 10, SPH_BODY_SUM_ZZ = 11,
    SPH_BODY_SUM_XY = 12, SPH_BODY_SUM_XZ = 13, SPH_BODY_SUM_YZ = 14,
    SPH_BODY_SUM_LX = 15, SPH_BODY_SUM_LY = 16, SPH_BODY_SUM_LZ = 17,
    SPH_BODY_SUMS = 18
};
#define SPH_BODY_SIZE_BINS 32
typedef struct SphBodyMeasureOptions {
    int32_t struct_size;        /* sizeof(SphBodyMeasureOptions) */
    float link;                 /* as SphBodyOptions.link */
    uint32_t max_bodies;        /* the call refuses the moments of more bodies; 0 = no cap */
    int32_t pad_;               /* 0 */
} SphBodyMeasureOptions;
typedef struct SphBodyMomentsRaw { /* 304 bytes */
    uint32_t label, count;      /* the label table's */
    uint64_t saturated;         /* terms of the body that took a NaN or saturating branch */
    SphSum128 sum[SPH_BODY_SUMS];
} SphBodyMomentsRaw;
/* The derived values of one body (DESIGN.md section 10k gives every expression; Python floats reproduce them bit for
 * bit).  A body of one particle: covariance and kinetic_internal are rounding residue around 0, either sign. */
typedef struct SphBodyValues {
    double mass;                /* count MASS */
    double com[3];              /* centre of mass */
    double velocity[3];         /* mean velocity */
    double momentum[3];         /* MASS sum(v) */
    double kinetic;             /* 0.5 MASS sum(v^2) */
    double kinetic_internal;    /* ... less the kinetic energy of the body moving as a whole */
    double mean_rho, mean_prs;
    double covariance[6];       /* of the positions about com: xx yy zz xy xz yz */
    double gyration;            /* radius of gyration: sqrt(max(0, trace)) */
    double angular[3];          /* angular momentum about com */
    uint64_t saturated;
} SphBodyValues;
/* Labels the state the handle holds NOW exactly as sph_label_bodies does -- the same state rules, error codes, grid
 * handling, both paths, the same SphBodyStats accounting; sph_bodies_host afterwards serves this labelling -- and then
 * queues the moment launches over that labelling and the copies of their results; labels and moments are always of
 * the same state.  opt == NULL: link = h, no cap.  SPH_EINVAL also for a non-zero pad_.  More bodies than a non-zero
 * max_bodies: SPH_ENOMEM, the message names both numbers, nothing is allocated for the refused moments and the handle
 * holds no moments (the labelling stands).  A raw row is 304 bytes, on the device and in pinned memory.  No
 * particles: SPH_OK, no bodies.  SPH_BODIES_PLAIN=1 selects the check path of the moments too (one thread per row,
 * every term a global integer atomic; identical words). */
int sph_measure_bodies(sph_handle *h, const SphBodyMeasureOptions *opt);
/* The results of the last sph_measure_bodies, owned by the handle, valid until the next one: num_bodies rows in the
 * label table's order (ascending label), and size_hist = SPH_BODY_SIZE_BINS words, size_hist[b] the number of bodies
 * with floor(log2(count)) == b.  Blocks until the copies have landed.  Any out-pointer may be NULL; *rows may be NULL
 * without bodies.  SPH_ESTATE before the first sph_measure_bodies and after one that was refused. */
int sph_body_moments_host(sph_handle *h, const SphBodyMomentsRaw **rows, int *num_bodies, const uint32_t **size_hist);
/* Pure host code, no GPU and no handle: out[b] = the derived values of rows[b], b < num_bodies. */
int sph_body_values(const SphBodyMomentsRaw *rows, int num_bodies, const SphSettings *settings, SphBodyValues *out);
typedef struct SphBodyMeasureStats {
    int32_t struct_size, pad_;  /* sizeof(SphBodyMeasureStats), 0: both written by the call */
    int64_t calls;              /* calls that queued moment launches (either path) */
    double seconds;             /* GPU time of the moment launches alone (the labelling's: SphBodyStats.seconds) */
} SphBodyMeasureStats;
/* Sums since create or since the last reset.  Blocks. */
int sph_get_body_measure_stats(sph_handle *h, SphBodyMeasureStats *out, int reset);

/* ---- neighbour lists: every particle's neighbours within a radius, as CSR in particle-id order ----
 * Additive to version 3: test for SPH_HAS_NEIGHBOURS.  Defined to the bit in DESIGN.md section 10j ("Neighbour
 * lists"); all fp32, every operation rounded on its own, in both math modes.  With r2 = radius radius, particle j is a
 * neighbour of i when i != j and d2 <= r2, e = p_j - p_i (the words sph_download_state returns),
 * d2 = (ex ex + ey ey) + ez ez; a NaN d2 is no neighbour.  That is the bodies' link test: the relation is symmetric to
 * the bit, coincident particles are neighbours of each other, a particle is never in its own list.  The result:
 * offsets = n + 1 words, offsets[0] = 0, offsets[i + 1] - offsets[i] the number of neighbours of particle id i;
 * neighbours = offsets[n] particle ids.  Inside a list the ids ascend -- the whole result is then a function of the
 * positions alone, the same words for any sweep backend, stream layout, kernel path or launch shape -- or, with
 * SPH_NEIGHBOURS_WALK_ORDER, stand in the order in which the density sweep's walk of the particle's row meets them (the
 * 27 cells in dz, dy, dx nesting, each cell's rows in the order of the grid's sorted stream: defined through the grid
 * sph_download_grid returns after the call); that mode skips the sort.  Out of scope: multi-GPU lists, radii above h
 * (the 27-cell walk is the bound), per-entry distances (recompute them from the ids and the downloaded positions),
 * device pointers to the result. */
#define SPH_HAS_NEIGHBOURS 1
enum { SPH_NEIGHBOURS_WALK_ORDER = 1 };
typedef struct SphNeighbourOptions {
    int32_t struct_size;   /* = sizeof(SphNeighbourOptions) */
    float radius;          /* 0 = h, else finite with 0 < radius <= h */
    int32_t flags;         /* SPH_NEIGHBOURS_* */
    int32_t pad_;          /* 0 */
    uint64_t max_entries;  /* the call refuses a result with more entries; 0 = 1 << 28 (1 GiB of ids) */
} SphNeighbourOptions;
/* Lists the neighbours in the state the handle holds NOW.  opt == NULL: every default.  State rules, grid handling
 * and error codes are sph_label_bodies's: the grid is found (phase 1) or built ahead (phase 0), the next step consumes
 * it and no result of any step changes; SPH_ESTATE before any state, inside an open phase-split step, for
 * SPH_FLAG_EXTERNAL_STATE handles (lists cross slab boundaries), with SPH_SWEEP_LINKED and with SPH_KEY_MORTON;
 * SPH_EINVAL for an unset struct_size, an unknown flag, a non-zero pad_ and for a radius that is not finite, negative
 * or greater than h.  The call counts, scans, and waits on the host once, for the total and the longest count.  A
 * total above max_entries: SPH_ENOMEM, the message names both numbers, nothing is allocated for the refused result
 * and the handle holds no neighbour result (the stats show what was counted).  Otherwise the buffers grow on demand,
 * the emit, the sort and the copies are queued and the call returns.  No particles: SPH_OK, n = 0, offsets = {0}.
 * SPH_NEIGHBOURS_PLAIN=1 in the environment selects the check path (one thread per row, every candidate loaded from
 * global memory, the sort one thread per list; identical words). */
int sph_neighbour_lists(sph_handle *h, const SphNeighbourOptions *opt);
/* The results of the last sph_neighbour_lists, owned by the handle, valid until the next one.  Blocks until the copies
 * have landed.  Any out-pointer may be NULL; *neighbours may be NULL where entries == 0.  SPH_ESTATE before the first
 * sph_neighbour_lists and after one that was refused. */
int sph_neighbours_host(sph_handle *h, const uint64_t **offsets, const uint32_t **neighbours, int *n, uint64_t *entries);
typedef struct SphNeighbourStats {
    int32_t struct_size, pad_;  /* sizeof(SphNeighbourStats), 0: both written by the call */
    int64_t calls;              /* calls that ran a kernel (either path) */
    uint64_t entries;           /* sum of offsets[n] over those calls; a refused call adds what it counted */
    uint64_t longest;           /* the longest list of the last call */
    uint64_t runs_staged, runs_direct; /* as SphDeriveStats, summed over the count and the emit walk; check path: 0 */
    double seconds;             /* GPU time of count + scan + emit + sort (HIP events on the compute stream) */
} SphNeighbourStats;
/* Sums since create or since the last reset (a reset clears `longest` too).  Blocks. */
int sph_get_neighbour_stats(sph_handle *h, SphNeighbourStats *out, int reset);

/* ---- body tracks: which body of this labelling is which body of the last one, merges and splits ----
 * Additive to version 3: test for SPH_HAS_BODY_TRACKS.  Defined in DESIGN.md section 10l ("Body tracks"); integers
 * only.  cur is the labelling of the state the handle holds now, prev the labelling of the last successful
 * sph_track_bodies on this handle (its reference); particle ids denote the same particles in both.  With prow[id] and
 * crow[id] the table rows (ascending label) of particle id's body in prev and cur, an edge is a distinct pair
 * (prow[id], crow[id]) and its count the number of ids with that pair; edges stand in ascending (cur, prev) order.  The
 * main parent of a current body is the edge into it with the greatest count, the main child of a previous body the
 * edge out of it with the greatest count, a tie going to the smallest row.  c continues p exactly when p is c's main
 * parent and c is p's main child; it then takes p's track.  Every other current body is born, with track
 * next_track + (born bodies in rows before it); after the call next_track += born.  A previous body nobody continues
 * has ended.  The first call after create or sph_track_reset has no previous bodies and no edges: every body is born
 * with parents = 0, main_parent = 0xFFFFFFFF, main_overlap = 0.  The words are the same for any schedule, kernel path
 * or sweep backend. */
#define SPH_HAS_BODY_TRACKS 1
typedef struct SphBodyTrackOptions {
    int32_t struct_size;        /* sizeof(SphBodyTrackOptions) */
    float link;                 /* as SphBodyOptions.link; may differ from call to call */
    uint32_t max_edges;         /* the call refuses a result with more edges; 0 = no cap */
    uint32_t flags;             /* SPH_TRACK_* */
} SphBodyTrackOptions;
enum { SPH_TRACK_WITH_MOMENTS = 1 };
typedef struct SphBodyEdge { /* 16 bytes */
    uint32_t prev, cur;         /* rows of the previous and of the current table */
    uint32_t count;             /* particle ids with that pair */
    uint32_t flags;             /* SPH_EDGE_* */
} SphBodyEdge;
enum { SPH_EDGE_MAIN_PARENT = 1, SPH_EDGE_MAIN_CHILD = 2 };
typedef struct SphBodyTrack { /* per current body, 24 bytes */
    uint64_t track;
    uint32_t parents;           /* edges into the body */
    uint32_t main_parent;       /* row of the previous table, 0xFFFFFFFF without parents */
    uint32_t main_overlap;      /* that edge's count */
    uint32_t flags;             /* SPH_TRACK_CONTINUES or SPH_TRACK_BORN, SPH_TRACK_MERGED with parents >= 2 */
} SphBodyTrack;
typedef struct SphBodyFate { /* per previous body, 32 bytes */
    uint64_t track;
    uint32_t label, count;      /* the previous table's */
    uint32_t children;          /* edges out of the body */
    uint32_t main_child;        /* row of the current table */
    uint32_t main_overlap;      /* that edge's count */
    uint32_t flags;             /* SPH_FATE_CONTINUES or SPH_FATE_ENDED, SPH_FATE_SPLIT with children >= 2 */
} SphBodyFate;
enum { SPH_TRACK_CONTINUES = 1, SPH_TRACK_BORN = 2, SPH_TRACK_MERGED = 4,
       SPH_FATE_CONTINUES = 1, SPH_FATE_ENDED = 2, SPH_FATE_SPLIT = 4 };
typedef struct SphBodyTrackSummary {
    int32_t struct_size, pad_;  /* sizeof(SphBodyTrackSummary), 0: both written by the call */
    uint32_t previous_bodies, bodies, edges;
    uint32_t continued, born;   /* continued + born == bodies */
    uint32_t ended;             /* continued + ended == previous_bodies */
    uint32_t merges, splits;    /* current bodies with >= 2 parents, previous bodies with >= 2 children */
    uint64_t next_track;        /* after the call */
    uint64_t sequence;          /* successful calls since create or sph_track_reset, this one included */
} SphBodyTrackSummary;
/* Labels the state the handle holds NOW exactly as sph_label_bodies does -- the same state rules, error codes, grid
 * handling, both paths, the same SphBodyStats accounting; sph_bodies_host afterwards serves this labelling -- and then
 * joins it with the reference.  opt == NULL: link = h, no cap, no flags.  SPH_EINVAL also for an unknown flag bit.
 * Beyond the labelling's wait the call waits on the host at most twice, for the number of partial edges (which sizes
 * the sort) and the number of edges; the rest is queued.  More edges than a non-zero max_edges: SPH_ENOMEM, the
 * message names both numbers, the handle holds no track results, the labelling stands, and the reference and
 * next_track stay what they were: the next call behaves as if the refused one had never happened.  Only a successful
 * call makes cur the reference.  SPH_TRACK_WITH_MOMENTS: the call then queues the moments of this labelling as
 * sph_measure_bodies with max_bodies = 0 would, and sph_body_moments_host serves them, row for row beside the tracks.
 * No particles: SPH_OK, nothing.  A call that ends in SPH_EHIP forgets the reference as sph_track_reset does.
 * SPH_BODIES_PLAIN=1 selects the check path here too (every particle id a partial edge, run lengths instead of
 * atomics, one thread per body; identical words). */
int sph_track_bodies(sph_handle *h, const SphBodyTrackOptions *opt);
/* The results of the last sph_track_bodies, owned by the handle, valid until the next one: one SphBodyTrack per
 * current body and one SphBodyFate per previous body, each in its table's order, and the edges.  Blocks until the
 * copies have landed.  Any out-pointer may be NULL; pointers returned for empty results may be NULL.  SPH_ESTATE
 * before the first sph_track_bodies and after one that was refused. */
int sph_body_tracks_host(sph_handle *h, const SphBodyTrack **tracks, int *num_bodies, const SphBodyFate **previous, int *num_previous,
                         const SphBodyEdge **edges, int *num_edges, SphBodyTrackSummary *summary);
/* Forgets the reference and the track results; next_track and sequence start from 0 again. */
int sph_track_reset(sph_handle *h);
typedef struct SphBodyTrackStats {
    int32_t struct_size, pad_;  /* sizeof(SphBodyTrackStats), 0: both written by the call */
    int64_t calls;              /* calls that queued track launches (either path) */
    uint64_t partials;          /* partial edges the calls sorted: the only number that depends on the path and the stream */
    uint64_t edges;             /* sum of the edges over the calls; a refused call adds what it counted */
    double seconds;             /* GPU time of the track launches alone (the labelling's: SphBodyStats.seconds) */
} SphBodyTrackStats;
/* Sums since create or since the last reset.  Blocks. */
int sph_get_body_track_stats(sph_handle *h, SphBodyTrackStats *out, int reset);

/* ---- pair statistics: the radial distribution and the velocity structure of the fluid, per bin of separation ----
 * Additive to version 3: test for SPH_HAS_PAIR_STATS.  Defined to the bit in DESIGN.md section 10m ("Pair
 * statistics").  The pairs are the unordered pairs {i, j} of distinct particle ids that the neighbour lists' test takes
 * at `radius` (e = p_j - p_i in fp32, d2 = (ex ex + ey ey) + ez ez, taken when d2 <= r2 = radius radius; a NaN d2 is
 * not), each counted once.  The bin of a pair is the number of k < bins - 1 with edges2[k] < d2, edges2 the table of
 * sph_pair_edges: bins of equal width in r, compared as squares; d2 == edges2[k] lies in bin k.  Per bin: the number of
 * pairs and four sums of the diagnostics' Q32.32 terms q(t) (NaN and saturation rules included, `saturated` counts
 * them), integers only, reported as SphSum128.  With w = v_j - v_i per axis in fp32 and everything after it in fp64, one
 * rounding per operation: D2 sums (double)d2, W2 sums (wx wx + wy wy) + wz wz, A sums (ex wx + ey wy) + ez wz (half
 * the rate of change of d2: negative means closing), L2 sums (A A) / (double)d2 (0 where d2 == 0): the squared
 * velocity difference along the separation.  Every term is the same word for (i, j) and (j, i), and the words are the
 * same for any row order, sweep backend, kernel path or launch shape.  The sum of `pairs` over the bins is
 * SphBodyStats.links of sph_label_bodies at link = radius and half of sph_neighbour_lists' entries.  Out of scope:
 * multi-GPU runs, radii above h, other binnings, pairs restricted to or across bodies, wall corrections, device
 * pointers to the table. */
#define SPH_HAS_PAIR_STATS 1
#define SPH_PAIR_MAX_BINS 128
enum { SPH_PAIR_SUM_D2 = 0, SPH_PAIR_SUM_W2 = 1, SPH_PAIR_SUM_A = 2, SPH_PAIR_SUM_L2 = 3, SPH_PAIR_SUMS = 4 };
typedef struct SphPairOptions {
    int32_t struct_size;   /* = sizeof(SphPairOptions) */
    int32_t flags;         /* none defined: 0 */
    float radius;          /* 0 = h, else finite with 0 < radius <= h */
    int32_t bins;          /* 1 .. SPH_PAIR_MAX_BINS; 0 = 32 */
    int32_t pad_;          /* 0 */
} SphPairOptions;
typedef struct SphPairBinRaw { /* 80 bytes */
    uint64_t pairs;
    SphSum128 sums[SPH_PAIR_SUMS];
    uint64_t saturated;    /* terms of the bin that took a NaN or saturating branch */
} SphPairBinRaw;
typedef struct SphPairValues { /* per bin; DESIGN.md section 10m gives every expression, Python floats reproduce them */
    double r_lo, r_hi;     /* the bin's edges: fp64 square roots of edges2[k - 1] (0 for bin 0) and edges2[k] */
    double pairs;
    double mean_r2;        /* value(D2) / pairs; like the next three 0 for an empty bin */
    double s2;             /* value(W2) / pairs: <|dv|^2> */
    double s2_par;         /* value(L2) / pairs: <u_par^2> */
    double approach;       /* value(A) / pairs: <r u_par>, negative where the bin's pairs are closing */
    double g;              /* pairs over what n ideal-gas particles in the box would put into the shell: walls not corrected for */
    uint64_t saturated;    /* the bin's, over its four sums */
} SphPairValues;
/* Pure host code: the squared outer edges of `bins` bins (0 = 32: then 32 floats are written) of equal width up to
 * `radius` (0 = h): edges2[k] = (float)(t t), t = ((double)radius (double)(k + 1)) / (double)bins, every fp64 operation
 * rounded on its own; the last edge is r2 = radius radius in fp32 itself.  Non-decreasing; a tiny radius with many
 * bins may repeat an edge.  SPH_EINVAL: bins outside [0, 128], an h that is not finite and positive, a radius that is
 * not finite, negative or above h, a NULL table. */
int sph_pair_edges(float radius_or_0, float h, int bins, float *edges2);
/* Queues the walk over the pairs of the state the handle holds NOW, the join of its table and the copy of the table
 * and of the edges it used; does not block and waits for nothing on the host.  opt == NULL: every default.  State
 * rules, grid handling and error codes are sph_neighbour_lists's: the grid is found (phase 1) or built ahead (phase 0),
 * the next step consumes it and no result of any step changes; SPH_ESTATE before any state, inside an open phase-split
 * step, for SPH_FLAG_EXTERNAL_STATE handles (pairs cross slab boundaries), with SPH_SWEEP_LINKED and with
 * SPH_KEY_MORTON; SPH_EINVAL for an unset struct_size, any flag, a non-zero pad_, bins outside [0, 128], a radius that
 * is not finite, negative or greater than h, and, on the default path, more than 1 << 24 particles (the bound up to
 * which no accumulator can wrap).  No particles: SPH_OK, an all-zero table.
 * SPH_PAIRS_PLAIN=1 in the environment selects the check path (one thread per row, every candidate loaded from global
 * memory, the bin by a linear scan, every word a global atomic; identical words, exact for any n). */
int sph_pair_statistics(sph_handle *h, const SphPairOptions *opt);
/* The result of the last sph_pair_statistics, owned by the handle, valid until the next one: *bins rows and the *bins
 * squared edges the call used.  Blocks until the copies have landed.  Any out-pointer may be NULL.  SPH_ESTATE before
 * the first sph_pair_statistics. */
int sph_pair_statistics_host(sph_handle *h, const SphPairBinRaw **rows, const float **edges2, int *bins);
/* Pure host code, no GPU and no handle: out[k] = the derived values of bin k, k < bins, for n particles in the box of
 * `settings`.  SPH_EINVAL: bins outside [1, 128], n < 0, a NULL pointer, a table that holds a NaN or decreases. */
int sph_pair_values(const SphPairBinRaw *rows, const float *edges2, int bins, const SphSettings *settings, int64_t n, SphPairValues *out);
typedef struct SphPairStats {
    int32_t struct_size, pad_;  /* sizeof(SphPairStats), 0: both written by the call */
    int64_t calls;              /* calls that ran a kernel (either path) */
    uint64_t pairs;             /* sum of the tables' pairs over those calls */
    uint64_t runs_staged, runs_direct; /* as SphDeriveStats; check path: 0 */
    double seconds;             /* GPU time of clear + walk + join (HIP events on the compute stream) */
} SphPairStats;
/* Sums since create or since the last reset.  Blocks. */
int sph_get_pair_stats(sph_handle *h, SphPairStats *out, int reset);

/* ---- ray casting: what a line of sight hits first, and a lit frame from any pinhole camera ----
 * Additive to version 3: test for SPH_HAS_RAY_CAST.  Defined to the bit in DESIGN.md section 10n ("Ray casting"); all
 * fp32, every operation rounded on its own in both math modes, nothing but + - x / sqrtf, comparisons, selects and
 * conversions.  Every particle is a sphere of `radius` r, r2 = r r; a particle is visible when each coordinate p has
 * p >= 0 and p / h < numCellsPerDim: rows outside the grid and rows that are not finite are hit by no ray.  A ray is
 * o + t d, d not normalised, dd = (dx dx + dy dy) + dz dz; it is valid when o and d are finite, 0 <= t_min <= t_max
 * (t_max may be +inf), 2^-40 <= dd <= 2^40 and |o_a| <= 64 (numCellsPerDim h) on every axis; an invalid ray is not an
 * error: it misses.  Ray and visible particle p with id i: e = p - o, b = (ex dx + ey dy) + ez dz, tc = b / dd,
 * f = e - tc d, b2 = (fx fx + fy fy) + fz fz, a2 = r2 - b2; nothing unless a2 > 0; t = tc - sqrtf(a2 / dd); nothing
 * unless t_min <= t <= t_max (a NaN fails every test); t == 0 is stored as +0.  The pair's word is
 * (bits(t) << 32) | i, the ray's word the minimum over all pairs, 0xFFFFFFFFFFFFFFFF where there is none: the nearest
 * entry, among equal entries the smallest id.  Entries only: a ray that starts inside a sphere does not see it. */
#define SPH_HAS_RAY_CAST 1
#define SPH_CAST_MAX_RAYS (1 << 24)
#define SPH_CAST_MISS 0xFFFFFFFFFFFFFFFFull
typedef struct SphRay { /* 32 bytes */
    float o[3];
    float t_min;
    float d[3];
    float t_max;
} SphRay;
typedef struct SphCastOptions {
    int32_t struct_size;   /* = sizeof(SphCastOptions) */
    float radius;          /* of the spheres; 0 = 0.5 h, else 0 < radius <= h */
} SphCastOptions;
/* Casts rays[0, m) against the state the handle holds NOW: blocks while the rays are uploaded, then queues the kernel
 * and the copy of the m words.  opt == NULL: every default.  0 <= m <= SPH_CAST_MAX_RAYS.  State rules, grid handling
 * and error codes are sph_sample_field's: the grid is found (phase 1) or built ahead (phase 0), the next step consumes
 * it and no result of any step changes; SPH_ESTATE before any state, inside an open phase-split step, for
 * SPH_FLAG_EXTERNAL_STATE handles, with SPH_SWEEP_LINKED and with SPH_KEY_MORTON; SPH_EINVAL for an unset struct_size,
 * a bad radius, m out of range, a NULL rays with m > 0.  No particles: every ray misses.  The default path walks the
 * cell grid along each ray, one lane per ray.  SPH_CAST_PLAIN=1 in the environment selects the check path, here and in
 * sph_render_view: one thread per ray tests every row of the stream (identical words); admitted while rays x particles
 * <= 2^32, SPH_EINVAL beyond. */
int sph_cast_rays(sph_handle *h, const SphRay *rays, int m, const SphCastOptions *opt);
/* The words of the last sph_cast_rays in the caller's order, owned by the handle, valid until the next one.  Blocks
 * until the copy has landed.  Any out-pointer may be NULL; *words may be NULL where m == 0.  SPH_ESTATE before the
 * first sph_cast_rays. */
int sph_cast_host(sph_handle *h, const uint64_t **words, int *m);
/* The view frame.  The basis is computed once, on the host, in fp32: g = target - eye, fwd = g / |g|, s0 = fwd x up,
 * s = s0 / |s0|, u = s x fwd.  Through the centre of pixel (c, row), row 0 on top, runs the ray o = eye,
 * d = (fwd + ax s) + ay u, ax = tan_half_x ((c + 0.5) / (0.5 W) - 1), ay the same from (H - 1 - row) and tan_half_y,
 * t_min = near, t_max = far: t is the depth along the view axis.  With eye (5, 5, 15), target (5, 5, 0), up (0, 1, 0)
 * and both tans 2 these are the rays of the column and liquid frames.  The picture, RGB8, row 0 first: the sphere the
 * ray enters first, lit by one diffuse light, in a flat colour or the field frame's colour of its particle; white
 * where one of the box's twelve edges, a cylinder of edge_radius, is not behind it; else black. */
enum {
    SPH_VIEW_FLAT = 0,     /* every sphere (0.1, 0.35, 0.9) */
    SPH_VIEW_FIELD = 1     /* SPH_VIEW_FIELD + SPH_FIELD_*: the field frame's ramp of that field of the sphere's particle */
};
typedef struct SphViewOptions {
    int32_t struct_size;   /* = sizeof(SphViewOptions) */
    int32_t width, height; /* 0 = 800 x 600; at most 4096 x 4096 */
    float eye[3], target[3], up[3]; /* finite; target - eye and (target - eye) x up must not vanish */
    float tan_half_x, tan_half_y;   /* both 0: tan_half_y = 0.41421357 (45 degrees), tan_half_x = tan_half_y W / H; else both > 0, at most 1024 */
    float near, far;       /* the ray's t window; near 0 = h; far 0 = +inf; else 0 < near <= far */
    float radius;          /* of the spheres; 0 = 0.5 h, else 0 < radius <= h */
    int32_t shade;         /* SPH_VIEW_* */
    float value_lo;        /* a field shade's colour scale, as SphFieldFrameOptions': both 0 = the minimum and */
    float value_hi;        /* maximum over ALL particles, reduced on the device */
    float light[3];        /* the direction towards the light in world space; all 0 = (-0.35, 0.8, 0.5); finite */
    float edge_radius;     /* of the box edges; 0 = 0.002 boxDim; negative: no edges */
} SphViewOptions;
/* sph_cast_rays' state rules and grid handling, sph_render_frame's queueing: does not block.  opt == NULL: SPH_EINVAL
 * (a camera has to be given).  A bad size, camera, window, radius, shade, range, light or edge_radius: SPH_EINVAL.
 * sph_frame_host serves the RGB and sph_get_render_time counts the frame; the other kinds' download and range calls
 * return SPH_ESTATE after it.  A flat, field, column or liquid frame rendered afterwards is what it would have been
 * without it. */
int sph_render_view(sph_handle *h, const SphViewOptions *opt);
/* The words behind the last view frame, width x height, row 0 first.  SPH_ESTATE if the last render was not a view
 * frame. */
int sph_download_view_buffer(sph_handle *h, uint64_t *words);
typedef struct SphCastStats {
    int32_t struct_size, pad_;  /* sizeof(SphCastStats), 0: both written by the call */
    int64_t calls;              /* sph_cast_rays and sph_render_view calls that ran a kernel (either path) */
    uint64_t rays;              /* rays of those calls (a view: width x height) */
    uint64_t layers;            /* grid layers the default path's lanes looked into (check path: 0) */
    uint64_t tests;             /* ray-particle pairs tested; the check path: rays x particles */
    double seconds;             /* GPU time of sph_cast_rays' kernels (a view's is sph_get_render_time's) */
} SphCastStats;
/* Sums since create or since the last reset.  Blocks. */
int sph_get_cast_stats(sph_handle *h, SphCastStats *out, int reset);

const char *sph_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
