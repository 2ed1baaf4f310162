// The case and winding tables of the surface mesh, derived from the geometry at compile
// time.  Plain C++17, no HIP: surface.hip places them in constant memory, tests/surface_selftest.cpp prints them.
//
// Corner k of a cell lies at the anchor + (k & 1, k >> 1 & 1, k >> 2 & 1).  Edge direction d = 0..6 leads from a
// point to its corner kDirCorner[d].  Tetrahedron sigma walks the path c0 = 0, c1 = c0 + e_s1, c2 = c1 + e_s2,
// c3 = 7; its case is the 4-bit word "path corner p is inside" << p.
#pragma once

#include <stdint.h>

namespace surface_tables {

constexpr int kDirs = 7, kTets = 6, kCases = 16;
// (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) as corner numbers
constexpr uint8_t kDirCorner[kDirs] = {1, 2, 4, 3, 5, 6, 7};
// the permutations of the axes: xyz xzy yxz yzx zxy zyx
constexpr uint8_t kPerm[kTets][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr int dir_of_corner(int c) {
    for (int d = 0; d < kDirs; ++d)
        if (kDirCorner[d] == c) return d;
    return -1;
}

// A vertex of a triangle, as the cell sees it: the edge's owner (a corner 0..6 of the cell) << 3 | its direction d.
// Triangle k of an entry is ref[3 k .. 3 k + 2], the winding already applied.
struct Entry {
    uint8_t ntri;
    uint8_t ref[6];
    uint8_t swapped; // bit k: triangle k had its last two vertices swapped (what the winding rule decided)
};

struct Tables {
    uint8_t dirCorner[8];       // kDirCorner (and a pad)
    uint8_t path[kTets][4];     // the corner numbers c0..c3 of tetrahedron sigma
    Entry tet[kTets][kCases];
    uint8_t cellTris[256];      // triangles of a cell by its 8 inside bits (bit k: corner k)
    bool undecided;             // a triangle lay in a plane the winding rule cannot judge: never, asserted below
};

struct Vec { int x, y, z; };
constexpr Vec corner_pos(int c) { return Vec{c & 1, (c >> 1) & 1, (c >> 2) & 1}; }
constexpr Vec sub(Vec a, Vec b) { return Vec{a.x - b.x, a.y - b.y, a.z - b.z}; }
constexpr Vec cross(Vec a, Vec b) { return Vec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
constexpr int dot(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the edge between path corners a < b of a tetrahedron: owner corner << 3 | direction
constexpr uint8_t edge_ref(const uint8_t path[4], int pa, int pb) {
    const int lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    return (uint8_t)(path[lo] << 3 | dir_of_corner(path[hi] ^ path[lo])); // (the path only ever adds axes)
}
// twice the midpoint of that edge
constexpr Vec edge_mid2(const uint8_t path[4], int pa, int pb) {
    const Vec a = corner_pos(path[pa]), b = corner_pos(path[pb]);
    return Vec{a.x + b.x, a.y + b.y, a.z + b.z};
}

constexpr Tables make_tables() {
    Tables T{};
    for (int d = 0; d < kDirs; ++d) T.dirCorner[d] = kDirCorner[d];
    for (int s = 0; s < kTets; ++s) {
        int c = 0;
        T.path[s][0] = 0;
        for (int k = 0; k < 3; ++k) T.path[s][k + 1] = (uint8_t)(c |= 1 << kPerm[s][k]);
    }
    for (int s = 0; s < kTets; ++s)
        for (int m = 0; m < kCases; ++m) {
            Entry &E = T.tet[s][m];
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int p = 0; p < 4; ++p) {
                if (m >> p & 1) in[ni++] = p;
                else out[no++] = p;
            }
            // the edges (inside corner, outside corner) of each triangle, by path position
            int tri[2][3][2] = {};
            if (ni == 1) {
                E.ntri = 1;
                for (int k = 0; k < 3; ++k) tri[0][k][0] = in[0], tri[0][k][1] = out[k];
            } else if (ni == 3) {
                E.ntri = 1;
                for (int k = 0; k < 3; ++k) tri[0][k][0] = in[k], tri[0][k][1] = out[0];
            } else if (ni == 2) {
                E.ntri = 2;
                const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                for (int t = 0; t < 2; ++t)
                    for (int k = 0; k < 3; ++k) tri[t][k][0] = q[pick[t][k]][0], tri[t][k][1] = q[pick[t][k]][1];
            }
            // from the centroid of O to the centroid of I, times ni no
            Vec g{0, 0, 0};
            for (int k = 0; k < ni; ++k) {
                const Vec p = corner_pos(T.path[s][in[k]]);
                g = Vec{g.x + no * p.x, g.y + no * p.y, g.z + no * p.z};
            }
            for (int k = 0; k < no; ++k) {
                const Vec p = corner_pos(T.path[s][out[k]]);
                g = Vec{g.x - ni * p.x, g.y - ni * p.y, g.z - ni * p.z};
            }
            for (int t = 0; t < E.ntri; ++t) {
                Vec mid[3] = {};
                for (int k = 0; k < 3; ++k) mid[k] = edge_mid2(T.path[s], tri[t][k][0], tri[t][k][1]);
                const int side = dot(cross(sub(mid[1], mid[0]), sub(mid[2], mid[0])), g);
                if (side == 0) T.undecided = true;
                const bool swap = side > 0;
                if (swap) E.swapped |= (uint8_t)(1 << t);
                const int order[3] = {0, swap ? 2 : 1, swap ? 1 : 2};
                for (int k = 0; k < 3; ++k) E.ref[3 * t + k] = edge_ref(T.path[s], tri[t][order[k]][0], tri[t][order[k]][1]);
            }
        }
    for (int b = 0; b < 256; ++b) {
        int count = 0;
        for (int s = 0; s < kTets; ++s) {
            int m = 0;
            for (int p = 0; p < 4; ++p) m |= (b >> T.path[s][p] & 1) << p;
            count += T.tet[s][m].ntri;
        }
        T.cellTris[b] = (uint8_t)count;
    }
    return T;
}

constexpr Tables kTables = make_tables();
static_assert(!kTables.undecided, "the winding rule left a triangle undecided");
static_assert(kTables.cellTris[0] == 0 && kTables.cellTris[255] == 0 && kTables.cellTris[1] == 6, "cell counts");

} // namespace surface_tables
