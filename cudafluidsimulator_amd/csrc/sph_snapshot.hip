// Snapshots of the single domain's state: sph_save_state / sph_load_state.
#include "sph_handle.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace sph_host;

namespace {
struct SnapshotHeader { // 64 bytes
    char magic[8];      // "SPHSNAP1"
    int32_t n;
    int32_t reserved;
    int64_t stepIndex;
    SphSettings settings; // 32 bytes
    char pad[8];
};
static_assert(sizeof(SnapshotHeader) == 64, "snapshot header");
} // namespace

extern "C" {

int sph_save_state(sph_handle *h, const char *path) {
    if (!h || !path) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, "");
    if (!h->ready || (h->phase != 0 && !h->gridAhead)) return fail(h, SPH_ESTATE, "no complete state to save");
    int rc = sph_sync(h);
    if (rc) return rc;
    const size_t n = (size_t)h->n;
    std::vector<float4> p4(n ? n : 1), v4(n ? n : 1);
    if (n) {
        HIPCHK(h, hipMemcpy(p4.data(), h->pos4[h->cur], n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(v4.data(), h->vel4[h->cur], n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    SnapshotHeader hd{};
    memcpy(hd.magic, "SPHSNAP1", 8);
    hd.n = h->n;
    hd.stepIndex = h->stepIndex;
    hd.settings = h->settings;
    FILE *f = fopen(path, "wb");
    if (!f) return fail(h, SPH_EINVAL, std::string("cannot open ") + path);
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && (n == 0 || (fwrite(p4.data(), sizeof(float4), n, f) == n &&
                                                                fwrite(v4.data(), sizeof(float4), n, f) == n));
    ok = (fclose(f) == 0) && ok;
    return ok ? SPH_OK : fail(h, SPH_EINVAL, "short write");
}

int sph_load_state(sph_handle *h, const char *path) {
    if (!h || !path) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (h->external) return reject_slab_mode(h, "");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(h, SPH_EINVAL, std::string("cannot open ") + path);
    SnapshotHeader hd{};
    bool ok = fread(&hd, sizeof hd, 1, f) == 1 && memcmp(hd.magic, "SPHSNAP1", 8) == 0;
    if (ok && (hd.n != h->n || memcmp(&hd.settings.h, &h->settings.h, 24) != 0)) {
        fclose(f);
        return fail(h, SPH_EINVAL, "snapshot does not match this simulator's settings");
    }
    const size_t n = (size_t)h->n;
    std::vector<float4> p4(n ? n : 1), v4(n ? n : 1);
    ok = ok && (n == 0 || (fread(p4.data(), sizeof(float4), n, f) == n && fread(v4.data(), sizeof(float4), n, f) == n));
    fclose(f);
    if (!ok) return fail(h, SPH_EINVAL, "not a snapshot / truncated");
    std::vector<char> seen(n ? n : 1, 0);
    int zmin = h->P.D, zmax = -1;
    for (size_t i = 0; i < n; ++i) { // ids must be a permutation: they index devicePosition
        uint32_t id;
        memcpy(&id, &p4[i].w, 4);
        if (id >= n || seen[id]) return fail(h, SPH_EINVAL, "corrupt snapshot (ids)");
        seen[id] = 1;
        // the same box / NaN check as sph_upload_state: a corrupt file must not inject NaNs
        const float x = p4[i].x, y = p4[i].y, z = p4[i].z, hh = h->settings.h;
        const float qx = x / hh, qy = y / hh, qz = z / hh, Df = (float)h->P.D; // (range test before any conversion)
        if (!(qx >= 0.f && qx < Df && qy >= 0.f && qy < Df && qz >= 0.f && qz < Df && x >= 0.f && y >= 0.f && z >= 0.f) ||
            !(v4[i].x == v4[i].x && v4[i].y == v4[i].y && v4[i].z == v4[i].z))
            return fail(h, SPH_EINVAL, "corrupt snapshot (position outside the simulation box / NaN)");
        const int cz = (int)qz;
        zmin = cz < zmin ? cz : zmin;
        zmax = cz > zmax ? cz : zmax;
    }
    h->zLayers = zmax >= zmin ? zmax - zmin + 1 : 0;
    HIPCHK(h, hipStreamSynchronize(h->compute));
    HIPCHK(h, hipStreamSynchronize(h->copy));
    h->cur = 0;
    if (n) {
        int rc = staged_upload(h, h->pos4[0], (size_t)n,
                               [&](size_t k, float4 *dst, size_t cnt) { memcpy(dst, p4.data() + k, cnt * sizeof(float4)); });
        if (!rc)
            rc = staged_upload(h, h->vel4[0], (size_t)n,
                               [&](size_t k, float4 *dst, size_t cnt) { memcpy(dst, v4.data() + k, cnt * sizeof(float4)); });
        if (rc) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    state_replaced(h);
    h->stepIndex = hd.stepIndex;
    h->hostPosIsInit = false;
    if (h->hostPos) // getPosition() shows the loaded state (id order)
        for (size_t i = 0; i < n; ++i) {
            uint32_t id;
            memcpy(&id, &p4[i].w, 4);
            h->hostPos[3 * (size_t)id] = p4[i].x;
            h->hostPos[3 * (size_t)id + 1] = p4[i].y;
            h->hostPos[3 * (size_t)id + 2] = p4[i].z;
        }
    return SPH_OK;
}

} // extern "C"
