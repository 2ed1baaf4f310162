// Stand-in for the GLUT front end when ./sph is built without display.cpp.
// It defines the two globals the simulator links against (display.cpp:19-20)
// and a startVisualization() that steps the simulation without a window.
// Never linked together with display.cpp (duplicate symbols by design).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "sha256.h"
#include "simulator.h"
#include "sph_c_api.h"

bool mouseClicked = false;
int2 clickCoords;

extern "C" void glutInit(int *, char **) {}

// speed|density|pressure in the environment variable `var`: the field (SPH_FIELD_* of sph_c_api.h), -1 if it is
// unset.  An unknown name is reported with what happens instead, and gives -1.
static int env_field(const char *var, const char *instead) {
    const char *e = getenv(var);
    if (!e) return -1;
    const char *names[3] = {"speed", "density", "pressure"};
    for (int k = 0; k < 3; ++k)
        if (!strcmp(e, names[k])) return k;
    fprintf(stderr, "sph: %s=%s is not speed, density or pressure -- %s\n", var, e, instead);
    return -1;
}

// SPH_FREE_SHADE: the field that colours the frames, `column` (kShadeColumn) for column-density frames or `liquid`
// (kShadeLiquid) for the shaded water surface; unset: the reference's flat blue
static const int kShadeColumn = 100, kShadeLiquid = 101;
static int shade_field() {
    const char *e = getenv("SPH_FREE_SHADE");
    if (e && !strcmp(e, "column")) return kShadeColumn;
    if (e && !strcmp(e, "liquid")) return kShadeLiquid;
    return env_field("SPH_FREE_SHADE", "nor column or liquid: writing flat frames");
}

// <dir>/<pattern with the frame number f> opened for writing bytes, or NULL after a complaint on stderr
static FILE *open_out(const char *dir, const char *pattern, int f) {
    char name[32];
    snprintf(name, sizeof name, pattern, f);
    const std::string path = std::string(dir) + "/" + name;
    FILE *out = fopen(path.c_str(), "wb");
    if (!out) fprintf(stderr, "sph: cannot write %s\n", path.c_str());
    return out;
}

static bool write_bytes(FILE *out, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, out) == bytes; }

// a w x h image of RGB bytes, row 0 on top, as binary P6
static bool write_ppm(const char *dir, const char *pattern, int f, int w, int h, const void *rgb) {
    FILE *out = open_out(dir, pattern, f);
    if (!out) return false;
    fprintf(out, "P6\n%d %d\n255\n", w, h);
    const bool ok = write_bytes(out, rgb, (size_t)w * (size_t)h * 3);
    return (fclose(out) == 0) && ok;
}

// Binary little-endian PLY (binary keeps the floats' bits): `count` vertices whose properties are `props`, as the
// packed rows of `rowBytes` each say; with faces >= 0 also that many triangles, `list uchar int vertex_indices`, as
// packed 13-byte rows (the count 3, then three 32-bit indices).
struct PlyProp {
    const char *type, *name;
};
static bool write_ply(const char *dir, const char *pattern, int f, long long count, std::initializer_list<PlyProp> props,
                      const void *rows, size_t rowBytes, long long faces = -1, const void *faceRows = NULL) {
    FILE *out = open_out(dir, pattern, f);
    if (!out) return false;
    fprintf(out, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\n", count);
    for (const PlyProp &p : props) fprintf(out, "property %s %s\n", p.type, p.name);
    if (faces >= 0) fprintf(out, "element face %lld\nproperty list uchar int vertex_indices\n", faces);
    fprintf(out, "end_header\n");
    bool ok = write_bytes(out, rows, (size_t)count * rowBytes);
    if (faces > 0) ok = ok && write_bytes(out, faceRows, (size_t)faces * 13);
    return (fclose(out) == 0) && ok;
}

// SPH_FREE_FRAMES_DIR=<dir>: what the window would have shown after frame f, as <dir>/frame_%04d.ppm (binary P6).
// render_frame: the picture, or NULL where the run renders none (a multi-GPU run; the simulator has said so).
static const unsigned char *render_frame(Simulator *simulator, int field, int *w, int *h) {
    return field < 0                ? simulator->renderFrame(w, h)
           : field == kShadeColumn ? simulator->renderColumn(w, h)
           : field == kShadeLiquid ? simulator->renderLiquid(w, h)
                                   : simulator->renderField(field, w, h);
}

// SPH_FREE_SLICE=speed|density|pressure: beside each frame the cut plane z = 5 of that field, sampled on 400 x 400
// lattice points over [0, 10)^2 (sph_sample_field), as <dir>/slice_%04d.ppm: row 0 = largest y, coloured with
// the field frame's quantiser and ramp over the slice's own minimum and maximum.
static bool write_slice(Simulator *simulator, const char *dir, int f, int field) {
    const int N = 400;
    const float origin[3] = {0.f, 0.f, 5.f}, spacing[3] = {10.f / N, 10.f / N, 1.f};
    const float *v = simulator->sampleField(field, origin, spacing, N, N, 1);
    if (!v) return false;
    float lo = v[0], hi = v[0];
    for (int i = 1; i < N * N; ++i) {
        lo = v[i] < lo ? v[i] : lo;
        hi = v[i] > hi ? v[i] : hi;
    }
    std::string rgb((size_t)N * N * 3, '\0');
    for (int r = 0; r < N; ++r)
        for (int x = 0; x < N; ++x) {
            const float s = v[(N - 1 - r) * N + x];
            unsigned q = 0;
            if (hi != lo) {
                const float u = ((s - lo) / (hi - lo)) * 256.f;
                if (u == u) q = (unsigned)(int)fminf(fmaxf(floorf(u), 0.f), 255.f);
            }
            unsigned char *p = reinterpret_cast<unsigned char *>(&rgb[((size_t)r * N + x) * 3]);
            if (q < 64u) p[0] = 0, p[1] = (unsigned char)(4u * q), p[2] = 255;
            else if (q < 128u) p[0] = 0, p[1] = 255, p[2] = (unsigned char)(255u - 4u * (q - 64u));
            else if (q < 192u) p[0] = (unsigned char)(4u * (q - 128u)), p[1] = 255, p[2] = 0;
            else p[0] = 255, p[1] = (unsigned char)(255u - 4u * (q - 192u)), p[2] = 0;
        }
    return write_ppm(dir, "slice_%04d.ppm", f, N, N, rgb.data());
}

// SPH_FREE_SURFACE=<iso>: beside each frame the surface density == iso (sph_extract_surface) over 101^3 lattice
// points on [0, boxDim]^3, as <dir>/surface_%04d.ply: `float x y z` vertices and triangles.
static bool write_surface(Simulator *simulator, const char *dir, int f, float iso) {
    const int N = 101;
    const float sp = simulator->settings->boxDim / (float)(N - 1);
    const float origin[3] = {0.f, 0.f, 0.f}, spacing[3] = {sp, sp, sp};
    const float *verts = NULL;
    const unsigned *tris = NULL;
    long long nv = 0, nt = 0;
    if (!simulator->extractSurface(iso, origin, spacing, N, N, N, &verts, &nv, &tris, &nt)) return false;
    std::string faces((size_t)nt * 13, '\0');
    for (long long t = 0; t < nt; ++t) {
        faces[(size_t)t * 13] = 3;
        memcpy(&faces[(size_t)t * 13 + 1], tris + 3 * t, 12);
    }
    return write_ply(dir, "surface_%04d.ply", f, nv, {{"float", "x"}, {"float", "y"}, {"float", "z"}}, verts, 12, nt, faces.data());
}

// SPH_FREE_TRACERS=<count>: `count` passive tracers (sph_tracers_*), seeded at the setup positions of the particles
// with ids k n / count, advected by `timestep` after every frame; beside each written frame their state as
// <dir>/tracers_%04d.ply: vertex properties `float x y z vx vy vz density`.
static bool seed_tracers(Simulator *simulator, int count) {
    const int n = simulator->settings->numParticles;
    const float3 *p = simulator->getPosition();
    if (!p || n <= 0) return false;
    std::string seeds((size_t)count * 12, '\0');
    for (int k = 0; k < count; ++k) memcpy(&seeds[(size_t)k * 12], &p[(long long)k * n / count], 12);
    return simulator->setTracers(reinterpret_cast<const float *>(seeds.data()), count);
}
static bool write_tracers(Simulator *simulator, const char *dir, int f) {
    const float *pd = NULL, *u = NULL;
    int m = 0;
    if (!simulator->getTracers(&pd, &u, &m)) return false;
    std::string rows((size_t)m * 28, '\0');
    for (int i = 0; i < m; ++i) {
        memcpy(&rows[(size_t)i * 28], pd + 4 * (size_t)i, 12);
        memcpy(&rows[(size_t)i * 28 + 12], u + 4 * (size_t)i, 12);
        memcpy(&rows[(size_t)i * 28 + 24], pd + 4 * (size_t)i + 3, 4);
    }
    return write_ply(dir, "tracers_%04d.ply", f, m,
                     {{"float", "x"}, {"float", "y"}, {"float", "z"}, {"float", "vx"}, {"float", "vy"}, {"float", "vz"}, {"float", "density"}},
                     rows.data(), 28);
}

// SPH_FREE_PARTICLES=1: beside each written frame the particles with their derived fields (sph_derive) as
// <dir>/particles_%04d.ply: one vertex per particle in id order, properties
// `float x y z vx vy vz rho wx wy wz divergence gx gy gz` and `uint neighbours`.
static bool write_particles(Simulator *simulator, const char *dir, int f) {
    const int n = simulator->settings->numParticles;
    const float *wd = NULL, *gr = NULL;
    const uint32_t *nb = NULL;
    if (!simulator->deriveFlow(&wd, &gr, &nb)) return false;
    const float3 *p = simulator->getPosition();
    std::string vel((size_t)(n > 0 ? n : 1) * 12, '\0');
    if (!p || !simulator->getVelocity(reinterpret_cast<float *>(&vel[0]))) return false;
    std::string rows((size_t)n * 60, '\0');
    for (int i = 0; i < n; ++i) {
        char *r = &rows[(size_t)i * 60];
        memcpy(r, &p[i], 12);
        memcpy(r + 12, &vel[(size_t)i * 12], 12);
        memcpy(r + 24, gr + 4 * (size_t)i + 3, 4);  // rho
        memcpy(r + 28, wd + 4 * (size_t)i, 16);     // wx wy wz divergence
        memcpy(r + 44, gr + 4 * (size_t)i, 12);     // gx gy gz
        memcpy(r + 56, nb + i, 4);
    }
    return write_ply(dir, "particles_%04d.ply", f, n,
                     {{"float", "x"}, {"float", "y"}, {"float", "z"}, {"float", "vx"}, {"float", "vy"}, {"float", "vz"}, {"float", "rho"},
                      {"float", "wx"}, {"float", "wy"}, {"float", "wz"}, {"float", "divergence"}, {"float", "gx"}, {"float", "gy"},
                      {"float", "gz"}, {"uint", "neighbours"}},
                     rows.data(), 60);
}

// SPH_FREE_BODIES=<f>, f in (0, 1], the link length in units of h: beside each written frame the particles with the
// body they belong to (sph_label_bodies) as <dir>/bodies_%04d.ply: one vertex per particle in id order, properties
// `float x y z`, `uint label` and `uint body_count`; and one line on stderr, `bodies <frame> <num_bodies> <largest count>`.
static bool write_bodies(Simulator *simulator, const char *dir, int f, float link) {
    const int n = simulator->settings->numParticles;
    const uint32_t *labels = NULL, *table = NULL;
    int bodies = 0;
    uint32_t largest = 0;
    if (!simulator->labelBodies(link, &labels, &table, &bodies, &largest)) return false;
    const float3 *p = simulator->getPosition();
    if (!p) return false;
    // a label's row of the table: the labels ascend in it
    std::vector<uint32_t> countOf((size_t)(n > 0 ? n : 0), 0u);
    uint32_t most = 0;
    for (int b = 0; b < bodies; ++b) {
        countOf[table[8 * (size_t)b]] = table[8 * (size_t)b + 1];
        if (table[8 * (size_t)b] == largest) most = table[8 * (size_t)b + 1];
    }
    std::string rows((size_t)n * 20, '\0');
    for (int i = 0; i < n; ++i) {
        char *r = &rows[(size_t)i * 20];
        memcpy(r, &p[i], 12);
        memcpy(r + 12, labels + i, 4);
        memcpy(r + 16, &countOf[labels[i]], 4);
    }
    const bool ok = write_ply(dir, "bodies_%04d.ply", f, n,
                              {{"float", "x"}, {"float", "y"}, {"float", "z"}, {"uint", "label"}, {"uint", "body_count"}}, rows.data(), 20);
    if (ok) fprintf(stderr, "bodies %d %d %u\n", f, bodies, most);
    return ok;
}

// SPH_FREE_BODY_TABLE=<f>, f in (0, 1], the link length in units of h: beside each written frame the bodies' moments
// (sph_measure_bodies, sph_body_values) as <dir>/body_table_%04d.jsonl: one JSON line per body in label order with
// `label`, `count` and every field of SphBodyValues; doubles as %.17g, which reads back to the same double.
static void put_doubles(FILE *out, const char *name, const double *v, int k) {
    fprintf(out, ", \"%s\": [", name);
    for (int i = 0; i < k; ++i) fprintf(out, i ? ", %.17g" : "%.17g", v[i]);
    fputc(']', out);
}
static bool write_body_table(Simulator *simulator, const char *dir, int f, float link) {
    const SphBodyMomentsRaw *rows = NULL;
    int bodies = 0;
    if (!simulator->measureBodies(link, &rows, &bodies, NULL)) return false;
    std::vector<SphBodyValues> values((size_t)(bodies > 0 ? bodies : 0));
    SphSettings s; // (Settings and SphSettings share their layout)
    memcpy(&s, simulator->settings, sizeof s);
    if (sph_body_values(rows, bodies, &s, values.data()) != SPH_OK) return false;
    FILE *out = open_out(dir, "body_table_%04d.jsonl", f);
    if (!out) return false;
    for (int b = 0; b < bodies; ++b) {
        const SphBodyValues &v = values[(size_t)b];
        fprintf(out, "{\"label\": %u, \"count\": %u, \"mass\": %.17g", rows[b].label, rows[b].count, v.mass);
        put_doubles(out, "com", v.com, 3);
        put_doubles(out, "velocity", v.velocity, 3);
        put_doubles(out, "momentum", v.momentum, 3);
        fprintf(out, ", \"kinetic\": %.17g, \"kinetic_internal\": %.17g, \"mean_rho\": %.17g, \"mean_prs\": %.17g", v.kinetic,
                v.kinetic_internal, v.mean_rho, v.mean_prs);
        put_doubles(out, "covariance", v.covariance, 6);
        fprintf(out, ", \"gyration\": %.17g", v.gyration);
        put_doubles(out, "angular", v.angular, 3);
        fprintf(out, ", \"saturated\": %llu}\n", (unsigned long long)v.saturated);
    }
    return fclose(out) == 0;
}

// SPH_FREE_BODY_TRACKS=<f>, f in (0, 1], the link length in units of h: beside each written frame the bodies' tracks
// (sph_track_bodies; the reference is the previous written frame) as <dir>/body_tracks_%04d.jsonl: a line with the frame
// number and every field of the summary, one line per body in table order, one line per edge with `prev` and `cur` as
// labels; and one line on stderr, `tracks <frame> <bodies> <continued> <born> <ended> <merges> <splits>`.
static bool write_body_tracks(Simulator *simulator, const char *dir, int f, float link) {
    const uint32_t *table = NULL;
    const SphBodyTrack *tracks = NULL;
    const SphBodyFate *previous = NULL;
    const SphBodyEdge *edges = NULL;
    int bodies = 0, before = 0, numEdges = 0;
    SphBodyTrackSummary s;
    if (!simulator->trackBodies(link, &table, &tracks, &bodies, &previous, &before, &edges, &numEdges, &s)) return false;
    FILE *out = open_out(dir, "body_tracks_%04d.jsonl", f);
    if (!out) return false;
    fprintf(out,
            "{\"frame\": %d, \"previous_bodies\": %u, \"bodies\": %u, \"edges\": %u, \"continued\": %u, \"born\": %u, \"ended\": %u, "
            "\"merges\": %u, \"splits\": %u, \"next_track\": %llu, \"sequence\": %llu}\n",
            f, s.previous_bodies, s.bodies, s.edges, s.continued, s.born, s.ended, s.merges, s.splits, (unsigned long long)s.next_track,
            (unsigned long long)s.sequence);
    for (int b = 0; b < bodies; ++b) {
        const SphBodyTrack &t = tracks[b];
        fprintf(out, "{\"label\": %u, \"count\": %u, \"track\": %llu, \"parents\": %u, \"main_parent\": ", table[8 * (size_t)b],
                table[8 * (size_t)b + 1], (unsigned long long)t.track, t.parents);
        if (t.parents && t.main_parent < (uint32_t)before) fprintf(out, "%u", previous[t.main_parent].label);
        else fputs("null", out);
        fprintf(out, ", \"main_overlap\": %u, \"continues\": %s}\n", t.main_overlap, (t.flags & SPH_TRACK_CONTINUES) ? "true" : "false");
    }
    for (int e = 0; e < numEdges; ++e)
        fprintf(out, "{\"prev\": %u, \"cur\": %u, \"count\": %u, \"main_parent\": %s, \"main_child\": %s}\n", previous[edges[e].prev].label,
                table[8 * (size_t)edges[e].cur], edges[e].count, (edges[e].flags & SPH_EDGE_MAIN_PARENT) ? "true" : "false",
                (edges[e].flags & SPH_EDGE_MAIN_CHILD) ? "true" : "false");
    const bool ok = fclose(out) == 0;
    if (ok) fprintf(stderr, "tracks %d %u %u %u %u %u %u\n", f, s.bodies, s.continued, s.born, s.ended, s.merges, s.splits);
    return ok;
}

// SPH_FREE_PAIR_STATS=<bins>, 1 .. 128: beside each written frame the pair statistics of the state within h
// (sph_pair_statistics, sph_pair_values) as <dir>/pair_stats_%04d.jsonl: one JSON line per bin with `bin` and every field
// of SphPairValues, doubles as %.17g; and one line on stderr, `pairs <frame> <pairs> <saturated>`.
static bool write_pair_stats(Simulator *simulator, const char *dir, int f, int bins) {
    const SphPairBinRaw *rows = NULL;
    const float *edges2 = NULL;
    int k = 0;
    if (!simulator->pairStatistics(bins, 0.f, &rows, &edges2, &k)) return false;
    std::vector<SphPairValues> v((size_t)k);
    SphSettings s; // (Settings and SphSettings share their layout)
    memcpy(&s, simulator->settings, sizeof s);
    if (sph_pair_values(rows, edges2, k, &s, s.numParticles, v.data()) != SPH_OK) {
        fprintf(stderr, "sph: sph_pair_values refused the table\n");
        return false;
    }
    FILE *out = open_out(dir, "pair_stats_%04d.jsonl", f);
    if (!out) return false;
    unsigned long long pairs = 0, saturated = 0;
    for (int b = 0; b < k; ++b) {
        fprintf(out,
                "{\"bin\": %d, \"r_lo\": %.17g, \"r_hi\": %.17g, \"pairs\": %.17g, \"mean_r2\": %.17g, \"s2\": %.17g, "
                "\"s2_par\": %.17g, \"approach\": %.17g, \"g\": %.17g, \"saturated\": %llu}\n",
                b, v[b].r_lo, v[b].r_hi, v[b].pairs, v[b].mean_r2, v[b].s2, v[b].s2_par, v[b].approach, v[b].g,
                (unsigned long long)v[b].saturated);
        pairs += rows[b].pairs;
        saturated += rows[b].saturated;
    }
    const bool ok = fclose(out) == 0;
    if (ok) fprintf(stderr, "pairs %d %llu %llu\n", f, pairs, saturated);
    return ok;
}

// SPH_FREE_NEIGHBOURS=<f>, f in (0, 1], the radius in units of h: beside each written frame every particle's
// neighbours within that radius (sph_neighbour_lists) as <dir>/neighbours_%04d.bin: the 8 bytes `SPHNBR01`, uint32 n,
// uint32 0, uint64 entries, the n + 1 uint64 offsets, the uint32 ids, all little-endian; and one line on stderr,
// `neighbours <frame> <entries> <longest>`.  A refused result has printed the library's message: no file, no more tries.
static bool write_neighbours(Simulator *simulator, const char *dir, int f, float radius) {
    const uint32_t head[2] = {(uint32_t)simulator->settings->numParticles, 0u};
    const uint64_t *offsets = NULL;
    const uint32_t *ids = NULL;
    uint64_t entries = 0, longest = 0;
    if (!simulator->neighbourLists(radius, &offsets, &ids, &entries)) return false;
    for (uint32_t i = 0; i < head[0]; ++i) longest = offsets[i + 1] - offsets[i] > longest ? offsets[i + 1] - offsets[i] : longest;
    FILE *out = open_out(dir, "neighbours_%04d.bin", f);
    if (!out) return false;
    bool ok = write_bytes(out, "SPHNBR01", 8) && write_bytes(out, head, 8) && write_bytes(out, &entries, 8);
    ok = ok && write_bytes(out, offsets, ((size_t)head[0] + 1) * 8) && write_bytes(out, ids, (size_t)entries * 4);
    ok = (fclose(out) == 0) && ok;
    if (ok) fprintf(stderr, "neighbours %d %llu %llu\n", f, (unsigned long long)entries, (unsigned long long)longest);
    return ok;
}

// SPH_FREE_VIEW=ex,ey,ez,tx,ty,tz[,flat|speed|density|pressure]: beside each written frame the state seen from the eye
// (ex, ey, ez) looking at (tx, ty, tz) (sph_render_view: 800 x 600, up (0, 1, 0), every other option at its default)
// as <dir>/view_%04d.ppm.  parse_view: the options, or false after one line on stderr.
static bool parse_view(const char *e, SphViewOptions *o) {
    SphViewOptions v = {};
    float c[6];
    int used = 0, k = 0; // k: SPH_VIEW_FLAT, SPH_VIEW_FIELD + SPH_FIELD_*
    const char *names[4] = {"flat", "speed", "density", "pressure"};
    bool ok = sscanf(e, "%f,%f,%f,%f,%f,%f%n", &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &used) == 6;
    if (ok && e[used]) { // the shade's name and nothing else
        while (k < 4 && strcmp(e + used + 1, names[k])) ++k;
        ok = e[used] == ',' && k < 4;
    }
    for (int a = 0; ok && a < 6; ++a) ok = std::isfinite(c[a]);
    ok = ok && !(c[0] == c[3] && c[1] == c[4] && c[2] == c[5]);
    if (!ok) {
        fprintf(stderr, "sph: SPH_FREE_VIEW=%s is not ex,ey,ez,tx,ty,tz[,flat|speed|density|pressure] with an eye off its target -- writing no views\n", e);
        return false;
    }
    for (int a = 0; a < 3; ++a) v.eye[a] = c[a], v.target[a] = c[3 + a];
    v.up[1] = 1.f;
    v.shade = k;
    *o = v;
    return true;
}

static bool write_view(Simulator *simulator, const char *dir, int f, const SphViewOptions &view) {
    int w = 0, h = 0;
    const unsigned char *rgb = simulator->renderView(view, &w, &h);
    return rgb && write_ppm(dir, "view_%04d.ppm", f, w, h, rgb);
}

// SPH_FREE_STATS=1: for each written frame one JSON line of run diagnostics (Simulator::diagnostics) in
// <dir>/stats.jsonl; doubles as %.17g, which reads back to the same double
static bool write_stats(Simulator *simulator, FILE *out, int f) {
    SphDiagnostics d;
    if (!simulator->diagnostics(&d)) return false;
    fprintf(out,
            "{\"frame\": %d, \"kinetic\": %.17g, \"potential\": %.17g, \"momentum\": [%.17g, %.17g, %.17g], "
            "\"com\": [%.17g, %.17g, %.17g], \"max_speed\": %.17g, \"cfl\": %.17g, \"min_rho\": %.17g, "
            "\"mean_rho\": %.17g, \"max_rho\": %.17g, \"saturated\": %llu}\n",
            f, d.kinetic, d.potential, d.momentum[0], d.momentum[1], d.momentum[2], d.com[0], d.com[1], d.com[2], d.max_speed,
            d.cfl, d.min_rho, d.mean_rho, d.max_rho, (unsigned long long)d.saturated);
    return fflush(out) == 0;
}

void startVisualization(Simulator *simulator) {
    int frames = 100;
    if (const char *e = getenv("SPH_FREE_FRAMES")) frames = atoi(e);
    const char *framesDir = getenv("SPH_FREE_FRAMES_DIR");
    if (framesDir && !*framesDir) framesDir = NULL;
    int every = 1;
    if (const char *e = getenv("SPH_FREE_FRAME_EVERY")) every = atoi(e) > 0 ? atoi(e) : 1;
    const int field = framesDir ? shade_field() : -1;
    bool frameFiles = framesDir != NULL; // false: no frame files (any more)
    int slice = framesDir ? env_field("SPH_FREE_SLICE", "writing no slices") : -1;
    float surfaceIso = 0.f; // 0: no surfaces
    if (framesDir && getenv("SPH_FREE_SURFACE")) {
        surfaceIso = strtof(getenv("SPH_FREE_SURFACE"), NULL);
        if (!(surfaceIso > 0.f) || !std::isfinite(surfaceIso)) {
            fprintf(stderr, "sph: SPH_FREE_SURFACE=%s is not a finite level > 0 -- writing no surfaces\n", getenv("SPH_FREE_SURFACE"));
            surfaceIso = 0.f;
        }
    }
    int tracers = 0; // 0: no tracers
    if (framesDir && getenv("SPH_FREE_TRACERS")) {
        const char *e = getenv("SPH_FREE_TRACERS");
        char *end = NULL;
        const long v = strtol(e, &end, 10);
        if (end == e || *end || v < 1 || v > (1l << 24)) {
            fprintf(stderr, "sph: SPH_FREE_TRACERS=%s is not a count in 1..16777216 -- writing no tracers\n", e);
        } else {
            const int n = simulator->settings->numParticles;
            tracers = v > n ? n : (int)v;
            if (tracers > 0 && !seed_tracers(simulator, tracers)) tracers = 0;
        }
    }
    bool particles = false;
    if (framesDir && getenv("SPH_FREE_PARTICLES")) {
        const char *e = getenv("SPH_FREE_PARTICLES");
        particles = strcmp(e, "1") == 0;
        if (!particles) fprintf(stderr, "sph: SPH_FREE_PARTICLES=%s is not 1 -- writing no particle files\n", e);
    }
    float bodyLink = 0.f; // 0: no body files
    if (framesDir && getenv("SPH_FREE_BODIES")) {
        const char *e = getenv("SPH_FREE_BODIES");
        char *end = NULL;
        const float v = strtof(e, &end);
        if (end == e || *end || !std::isfinite(v) || !(v > 0.f) || v > 1.f)
            fprintf(stderr, "sph: SPH_FREE_BODIES=%s is not a link length in (0, 1] (units of h) -- writing no body files\n", e);
        else
            bodyLink = v * simulator->settings->h;
    }
    float bodyTableLink = 0.f; // 0: no body tables
    if (framesDir && getenv("SPH_FREE_BODY_TABLE")) {
        const char *e = getenv("SPH_FREE_BODY_TABLE");
        char *end = NULL;
        const float v = strtof(e, &end);
        if (end == e || *end || !std::isfinite(v) || !(v > 0.f) || v > 1.f)
            fprintf(stderr, "sph: SPH_FREE_BODY_TABLE=%s is not a link length in (0, 1] (units of h) -- writing no body tables\n", e);
        else
            bodyTableLink = v * simulator->settings->h;
    }
    float bodyTrackLink = 0.f; // 0: no body tracks
    if (framesDir && getenv("SPH_FREE_BODY_TRACKS")) {
        const char *e = getenv("SPH_FREE_BODY_TRACKS");
        char *end = NULL;
        const float v = strtof(e, &end);
        if (end == e || *end || !std::isfinite(v) || !(v > 0.f) || v > 1.f)
            fprintf(stderr, "sph: SPH_FREE_BODY_TRACKS=%s is not a link length in (0, 1] (units of h) -- writing no body tracks\n", e);
        else
            bodyTrackLink = v * simulator->settings->h;
    }
    float neighbourRadius = 0.f; // 0: no neighbour files
    if (framesDir && getenv("SPH_FREE_NEIGHBOURS")) {
        const char *e = getenv("SPH_FREE_NEIGHBOURS");
        char *end = NULL;
        const float v = strtof(e, &end);
        if (end == e || *end || !std::isfinite(v) || !(v > 0.f) || v > 1.f)
            fprintf(stderr, "sph: SPH_FREE_NEIGHBOURS=%s is not a radius in (0, 1] (units of h) -- writing no neighbour files\n", e);
        else
            neighbourRadius = v * simulator->settings->h;
    }
    int pairBins = 0; // 0: no pair statistics
    if (framesDir && getenv("SPH_FREE_PAIR_STATS")) {
        const char *e = getenv("SPH_FREE_PAIR_STATS");
        char *end = NULL;
        const long v = strtol(e, &end, 10);
        if (end == e || *end || v < 1 || v > SPH_PAIR_MAX_BINS)
            fprintf(stderr, "sph: SPH_FREE_PAIR_STATS=%s is not a number of bins in 1 .. 128 -- writing no pair statistics\n", e);
        else
            pairBins = (int)v;
    }
    SphViewOptions view = {};
    bool views = framesDir && getenv("SPH_FREE_VIEW") && parse_view(getenv("SPH_FREE_VIEW"), &view);
    FILE *stats = NULL;
    if (framesDir && getenv("SPH_FREE_STATS") && atoi(getenv("SPH_FREE_STATS")) != 0) {
        const std::string path = std::string(framesDir) + "/stats.jsonl";
        if (!(stats = fopen(path.c_str(), "w"))) fprintf(stderr, "sph: cannot write %s\n", path.c_str());
    }
    fprintf(stderr, "sph: built without GLUT -- running %d frames headless\n", frames);
    for (int f = 0; f < frames; ++f) {
        if (f == frames / 2 && getenv("SPH_FREE_CLICK")) {
            mouseClicked = true;
            clickCoords = make_int2(400, 300);
        }
        simulator->simulate();
        if (tracers > 0 && !simulator->advectTracers(simulator->settings->timestep)) tracers = 0;
        if (framesDir && tracers > 0 && f % every == 0 && !write_tracers(simulator, framesDir, f)) tracers = 0;
        if (framesDir && particles && f % every == 0 && !write_particles(simulator, framesDir, f)) particles = false;
        if (framesDir && bodyLink > 0.f && f % every == 0 && !write_bodies(simulator, framesDir, f, bodyLink)) bodyLink = 0.f;
        if (framesDir && bodyTableLink > 0.f && f % every == 0 && !write_body_table(simulator, framesDir, f, bodyTableLink)) bodyTableLink = 0.f;
        if (framesDir && bodyTrackLink > 0.f && f % every == 0 && !write_body_tracks(simulator, framesDir, f, bodyTrackLink)) bodyTrackLink = 0.f;
        if (framesDir && neighbourRadius > 0.f && f % every == 0 && !write_neighbours(simulator, framesDir, f, neighbourRadius))
            neighbourRadius = 0.f;
        if (framesDir && pairBins > 0 && f % every == 0 && !write_pair_stats(simulator, framesDir, f, pairBins)) pairBins = 0;
        if (framesDir && frameFiles && f % every == 0) {
            int w = 0, h = 0;
            const unsigned char *rgb = render_frame(simulator, field, &w, &h);
            if (!rgb) frameFiles = false; // no picture to write: the frames stop, the other outputs go on
            else if (!write_ppm(framesDir, "frame_%04d.ppm", f, w, h, rgb)) framesDir = NULL; // the directory takes no files
        }
        if (framesDir && views && f % every == 0 && !write_view(simulator, framesDir, f, view)) views = false;
        if (framesDir && slice >= 0 && f % every == 0 && !write_slice(simulator, framesDir, f, slice)) slice = -1;
        if (framesDir && surfaceIso > 0.f && f % every == 0 && !write_surface(simulator, framesDir, f, surfaceIso)) surfaceIso = 0.f;
        if (framesDir && stats && f % every == 0 && !write_stats(simulator, stats, f)) {
            fclose(stats);
            stats = NULL;
        }
    }
    if (stats) fclose(stats);
    const float3 *p = simulator->getPosition();
    if (p && simulator->settings->numParticles > 0)
        printf("particle 0 after %d frames: (%f, %f, %f)\n", frames, p[0].x, p[0].y, p[0].z);
    if (p && getenv("SPH_PRINT_SHA256"))
        printf("positions_sha256 %s\n",
               sha256_hex(p, (size_t)simulator->settings->numParticles * sizeof(float3)).c_str());
}
