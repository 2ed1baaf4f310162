// The multi-GPU driver's message plan: every size it derives from partition headers, as plain C++ over
// ints (no HIP, no RCCL, no C-ABI header).  Both ends of a face size a message from headers alone -- one
// from its own, the other from the copy it received -- so each count has ONE definition, here.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

namespace mgpu_host {

// Message header = the sender's partition bounds (device-written) + a status word.
//   b[0] #rows with key < (zlo-1) D^2   (migrants down that land deeper than the first layer)
//   b[1] #rows with key <  zlo    D^2   (all migrants down)
//   b[2] #rows with key < (zlo+1) D^2   (end of the lower boundary layer)
//   b[3] #rows with key < (zhi-1) D^2   (start of the upper boundary layer)
//   b[4] #rows with key <  zhi    D^2   (start of the migrants up)
//   b[5] #rows with key < (zhi+1) D^2   (end of the migrants up that land in the first layer)
struct Hdr { int b[6], n, status; };
static_assert(sizeof(Hdr) == 32, "header is 8 ints");

// ---- message layouts (both ends compute them from a header) ----
// DOWN message = [migrants down | lower boundary layer] = rows [0, m1) of the sender's
// partitioned array; the window sent is rows [0, F); rows [F, m1) go in a second message.
// UP message = [upper boundary layer | migrants up] = rows [m2, n); the window is the LAST
// F rows, [n-F, n) ([0, F) if n < F); rows [m2, n-F) -- the FIRST rows -- go in a second one.
struct Layout { int payload, offset, extra, extra_at; }; // extra_at: the second message's first row, at the sender
inline Layout down_layout(const Hdr &h, int F) {
    const int payload = h.b[2];
    return {payload, 0, std::max(0, payload - F), F};
}
inline Layout up_layout(const Hdr &h, int F) {
    const int payload = h.n - h.b[3];
    const int extra = std::max(0, payload - F);
    if (extra) return {payload, 0, extra, h.b[3]};
    return {payload, h.n >= F ? F - payload : h.b[3], 0, h.b[3]};
}

// What crosses a face, off the sender's header: its boundary layer (the receiver's halo), its migrants, and
// those of them that land in the receiver's first layer ("near").  No neighbour there: Hdr{}, all counts 0.
struct Inflow { int bnd, mig, near; };
inline Inflow from_below(const Hdr &dn) { return {dn.b[4] - dn.b[3], dn.n - dn.b[4], dn.b[5] - dn.b[4]}; }
inline Inflow from_above(const Hdr &up) { return {up.b[2] - up.b[1], up.b[1], up.b[1] - up.b[0]}; }

// Exchange B over the face between the slab with header `lo` and the one above it, `hi`: each sends
// the boundary layer of its SORTED array, i.e. the layer it kept plus the near migrants it took in.
//   up:   lo's [s_hi, i1) -> the last rows of hi's lower halo [i0-up, i0)
//   down: hi's [i0, e_lo) -> the first rows of lo's upper halo [i1, i1+down)
struct FaceB { int up, down; };
inline FaceB exchange_b(const Hdr &lo, const Hdr &hi) {
    return {from_below(lo).bnd + from_above(hi).near, from_above(hi).bnd + from_below(lo).near};
}
inline bool operator!=(const FaceB &a, const FaceB &b) { return a.up != b.up || a.down != b.down; }

// The combined array before its sort, [halo from below | my migrants down | migrants from below |
// mine | migrants from above | my migrants up | halo from above]: at[k] = first row of segment k,
// and where the sort must put the owned rows [i0, i1) and their two boundary layers [i0, e_lo),
// [s_hi, i1) -- the very rows exchange B sends.  The segments' sources: of the own partitioned array
// rows [0, m0) migrate down, [m0, m3) stay, [m3, n) migrate up; dn / up is what the neighbours send.
struct Assembly { int at[7], n_comb, i0, e_lo, s_hi, i1, m0, m3, n; Inflow dn, up; };
inline Assembly assemble(const Hdr &me, const Hdr &nb_dn, const Hdr &nb_up) {
    const Inflow dn = from_below(nb_dn), up = from_above(nb_up);
    const int m0 = me.b[1], m3 = me.b[4], n = me.n;
    const int counts[7] = {dn.bnd, m0, dn.mig, m3 - m0, up.mig, n - m3, up.bnd};
    Assembly a{{0}, 0, 0, 0, 0, 0, m0, m3, n, dn, up};
    for (int k = 0; k < 6; ++k) a.at[k + 1] = a.at[k] + counts[k];
    a.n_comb = a.at[6] + counts[6];
    a.i0 = dn.bnd + m0;
    a.i1 = a.n_comb - (up.bnd + (n - m3));
    a.e_lo = a.i0 + exchange_b(nb_dn, me).down;
    a.s_hi = a.i1 - exchange_b(me, nb_up).up;
    return a;
}

// Cut D layers into `world` contiguous slabs of about equal particle counts, every slab
// at least min_layers thick (cuts on layer boundaries).
inline std::vector<int> partition_layers(const std::vector<long long> &hist, int world, int min_layers) {
    const int D = (int)hist.size();
    std::vector<long long> cum(D + 1, 0);
    for (int z = 0; z < D; ++z) cum[z + 1] = cum[z] + hist[z];
    const long long total = cum[D];
    std::vector<int> cuts{0};
    for (int r = 1; r < world; ++r) {
        const double target = (double)total * r / world;
        int z = (int)(std::lower_bound(cum.begin(), cum.end(), (long long)std::ceil(target)) - cum.begin());
        z = std::min(z, D);
        if (z > 0 && std::fabs((double)cum[z - 1] - target) <= std::fabs((double)cum[z] - target)) --z;
        z = std::max(z, cuts.back() + min_layers);
        z = std::min(z, D - (world - r) * min_layers);
        cuts.push_back(z);
    }
    cuts.push_back(D);
    return cuts;
}

} // namespace mgpu_host
