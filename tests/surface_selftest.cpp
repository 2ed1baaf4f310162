// Prints the tables of csrc/surface_tables.h, one entry per line, for tests/test_surface_cpu.py to hold against
// the restatement's.  Stand-alone, host only; built under ASan + UBSan.
#include <cstdio>

#include "surface_tables.h"

int main() {
    namespace st = surface_tables;
    const st::Tables &T = st::kTables;
    for (int d = 0; d < st::kDirs; ++d) printf("dir %d %d %d\n", d, st::kDirCorner[d], T.dirCorner[d]);
    for (int s = 0; s < st::kTets; ++s) printf("path %d %d %d %d %d\n", s, T.path[s][0], T.path[s][1], T.path[s][2], T.path[s][3]);
    for (int s = 0; s < st::kTets; ++s)
        for (int m = 0; m < st::kCases; ++m) {
            const st::Entry &E = T.tet[s][m];
            printf("tet %d %d %d %d", s, m, E.ntri, E.swapped);
            for (int k = 0; k < 3 * E.ntri; ++k) printf(" %d", E.ref[k]);
            printf("\n");
        }
    for (int b = 0; b < 256; ++b) printf("cell %d %d\n", b, T.cellTris[b]);
    printf("sizeof_entry %zu\n", sizeof(st::Entry));
    return T.undecided ? 1 : 0;
}
