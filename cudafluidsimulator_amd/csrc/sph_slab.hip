// The sph_slab_* entry points: one z-slab of a multi-GPU run on caller-owned buffers (driver: mgpu_step.cpp).
#include "sph_handle.h"

using namespace sph_host;

namespace {

// A slab is a dozen z-layers: with the fixed chunk -> XCD map the floor pile of every layer (the lowest y band
// = the first eighth of a layer's rows) lands on the same XCD and the launch waits for it -- N = 8 slabs of the
// headline run over 100 steps, slowest slab: density 0.196 -> 0.149, force 0.285 -> 0.187 ms per step with the map
// moved on by one XCD per layer.  (The single domain's 80 layers: within noise either way, default off.)
int slab_rotate(const sph_handle *h) { return h->knobs.xcdRotate >= 0 ? h->knobs.xcdRotate : 1; }

// the sweeps' precondition: the last grid build sorted into `buf`
int slab_sorted_ok(sph_handle *h, int buf) {
    if (!h->gridValid || h->sorted != buf) return fail(h, SPH_ESTATE, "sph_slab_sort into this buffer first");
    return SPH_OK;
}

int slab_range_ok(sph_handle *h, int buf, int i_begin, int i_end, int n_all, bool sorted = false) {
    if (!h->external || !h->pos4[0]) return fail(h, SPH_ESTATE, "sph_bind_buffers first");
    if ((buf != 0 && buf != 1) || i_begin < 0 || i_end < i_begin || n_all < i_end || n_all > h->cap)
        return fail(h, SPH_EINVAL, "bad slab range");
    return sorted ? slab_sorted_ok(h, buf) : SPH_OK;
}

// sweep arguments of a launch over the rows [i_begin, i_end) of a slab's n_all (owned + halo) sorted rows
SweepArgs slab_sweep_args(sph_handle *h, int i_begin, int i_end, int n_all) {
    SweepArgs A = make_sweep_args(h);
    A.i_begin = i_begin;
    A.i_end = i_end;
    A.i_origin = i_begin & ~63; // hit-stream waves = whole words of the zero-pair filter's bit array
    A.n_all = n_all;
    A.tileChunk = tile_chunk(h, i_end - i_begin, h->zLayers);
    A.tileRotate = slab_rotate(h);
    A.force_out = nullptr;
    return A;
}

// the segment bounds a sort or partition left on the device, for the host
int read_bounds(sph_handle *h, int nthr, int32_t *out) {
    HIPCHK(h, hipMemcpyAsync(h->boundsHost, h->boundsDev, nthr * sizeof(int), hipMemcpyDeviceToHost, h->compute));
    HIPCHK(h, hipStreamSynchronize(h->compute));
    for (int k = 0; k < nthr; ++k) out[k] = h->boundsHost[k];
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_set_stream(sph_handle *h, void *hip_stream) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    HIPCHK(h, hipStreamSynchronize(h->compute));
    if (!h->ownCompute) h->ownCompute = h->compute;
    // NULL is HIP's default ("null") stream -- what torch.cuda.current_stream()
    // reports unless the caller switched streams.
    h->compute = (hipStream_t)hip_stream;
    return SPH_OK;
}

int sph_bind_buffers(sph_handle *h, void *pos4_a, void *vel4_a, void *pos4_b, void *vel4_b,
                     int capacity) {
    if (!h) return SPH_EINVAL;
    if (!h->external) return fail(h, SPH_ESTATE, "create with SPH_FLAG_EXTERNAL_STATE");
    if (!pos4_a || !vel4_a || !pos4_b || !vel4_b || capacity > h->cap || capacity < 0)
        return fail(h, SPH_EINVAL, "bad buffers / capacity exceeds options.capacity");
    h->pos4[0] = (float4 *)pos4_a;
    h->vel4[0] = (float4 *)vel4_a;
    h->pos4[1] = (float4 *)pos4_b;
    h->vel4[1] = (float4 *)vel4_b;
    return SPH_OK;
}

void *sph_get_stream(sph_handle *h) { return h ? (void *)h->compute : nullptr; }
void *sph_slab_records(sph_handle *h) { return (h && h->opt.sweep == SPH_SWEEP_LIST) ? (void *)h->pv8.get() : nullptr; }

int sph_slab_sort_async(sph_handle *h, int src_buf, int src_offset, int count,
                        const uint32_t *thresholds, int nthr, void *bounds_dev_out) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, src_buf, 0, 0, 0);
    if (rc) return rc;
    if (src_offset < 0 || count < 0 || (long long)src_offset + count > h->cap || nthr < 0 ||
        nthr > 8 || (nthr > 0 && !thresholds))
        return fail(h, SPH_EINVAL, "bad sort range");
    hipStream_t s = h->compute;
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->kt.sort, &pe))) return rc;
    h->ws.velSample = (h->quiet && h->knobs.zeroPairFilter) ? h->vel4[src_buf] + src_offset : nullptr; // the filter's reference velocity
    h->ws.vrefOut = h->quietVref;
    int res = sph_sort_cells(h->ws, h->P, h->pos4[src_buf] + src_offset, count, key_bits(h), s, h->cellRange,
                             h->P.numCells); // (clears the cell table too)
    // the segment bounds (and the element count, [nthr]) and the clearing of the hit-stream
    // cursors ride on the gather launch
    GatherExtras X = gather_extras(h);
    if (nthr > 0) {
        for (int k = 0; k < nthr; ++k) X.thr.v[k] = thresholds[k];
        X.nthr = nthr;
        X.bounds = bounds_dev_out ? static_cast<int *>(bounds_dev_out) : h->boundsDev.get();
    }
    sph_launch_gather(h->pos4[src_buf] + src_offset, h->vel4[src_buf] + src_offset,
                      h->ws.vals[res], h->ws.keys[res], h->pos4[src_buf ^ 1],
                      h->vel4[src_buf ^ 1], h->pv8, h->cellRange, count, s, X);
    HIPCHK(h, hipEventRecord(pe->b, s));
    if (nthr == 4) // [zlo, zlo+1, zhi-1, zhi] * D*D: the slab's owned z-layers
        h->zLayers = (int)((thresholds[3] - thresholds[0]) / (uint32_t)(h->P.D * h->P.D));
    HIPCHK(h, hipGetLastError());
    h->sorted = src_buf ^ 1;
    h->sortedKeyBuf = res;
    h->gridValid = true;
    h->slabOwnedEnd = h->slabOwnedBegin = 0; // (a new sorted array: no density sweep has vouched for any row of it yet)
    return SPH_OK;
}

int sph_slab_sort(sph_handle *h, int src_buf, int src_offset, int count,
                  const uint32_t *thresholds, int nthr, int32_t *bounds_out) {
    if (!h) return SPH_EINVAL;
    if (nthr > 0 && !bounds_out) return fail(h, SPH_EINVAL, "bad sort range");
    int rc = sph_slab_sort_async(h, src_buf, src_offset, count, thresholds, nthr, nullptr);
    if (rc) return rc;
    return nthr > 0 ? read_bounds(h, nthr, bounds_out) : SPH_OK;
}

int sph_slab_partition_async(sph_handle *h, int src_buf, int src_offset, int count,
                             const uint32_t *thresholds, int nthr, void *bounds_dev_out) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, src_buf, 0, 0, 0);
    if (rc) return rc;
    if (src_offset < 0 || count < 0 || (long long)src_offset + count > h->cap || nthr < 1 ||
        nthr > 8 || !thresholds)
        return fail(h, SPH_EINVAL, "bad partition range");
    for (int k = 1; k < nthr; ++k)
        if (thresholds[k] < thresholds[k - 1]) return fail(h, SPH_EINVAL, "thresholds must ascend");
    hipStream_t s = h->compute;
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->kt.sort, &pe))) return rc;
    Thresholds T{};
    for (int k = 0; k < nthr; ++k) T.v[k] = thresholds[k];
    // two launches (count per tile, move): grid.hip
    sph_launch_partition(h->P, h->pos4[src_buf] + src_offset, h->vel4[src_buf] + src_offset,
                         h->pos4[src_buf ^ 1], h->vel4[src_buf ^ 1], T, nthr, count, h->partTiles,
                         h->boundsDev, s);
    HIPCHK(h, hipEventRecord(pe->b, s));
    if (bounds_dev_out)
        HIPCHK(h, hipMemcpyAsync(bounds_dev_out, h->boundsDev, (nthr + 1) * sizeof(int),
                                 hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipGetLastError());
    h->gridValid = false;
    return SPH_OK;
}

int sph_slab_partition(sph_handle *h, int src_buf, int src_offset, int count,
                       const uint32_t *thresholds, int nthr, int32_t *bounds_out,
                       void *bounds_dev_out) {
    if (!h) return SPH_EINVAL;
    if (!bounds_out) return fail(h, SPH_EINVAL, "bad partition range");
    int rc = sph_slab_partition_async(h, src_buf, src_offset, count, thresholds, nthr, bounds_dev_out);
    if (rc) return rc;
    return read_bounds(h, nthr, bounds_out);
}

int sph_slab_copy_segments(sph_handle *h, int dst_buf, int nseg, const void *const *src_pos,
                           const void *const *src_vel, const int32_t *counts,
                           const int32_t *dst_offsets) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, dst_buf, 0, 0, 0);
    if (rc) return rc;
    if (nseg < 0 || nseg > 8 || (nseg > 0 && (!src_pos || !src_vel || !counts || !dst_offsets)))
        return fail(h, SPH_EINVAL, "bad segment list");
    SegmentTable T{};
    T.n = nseg;
    T.prefix[0] = 0;
    for (int k = 0; k < nseg; ++k) {
        if (counts[k] < 0 || dst_offsets[k] < 0 || (long long)dst_offsets[k] + counts[k] > h->cap ||
            (counts[k] > 0 && (!src_pos[k] || !src_vel[k])))
            return fail(h, SPH_EINVAL, "segment outside the bound buffers");
        T.spos[k] = static_cast<const float4 *>(src_pos[k]);
        T.svel[k] = static_cast<const float4 *>(src_vel[k]);
        T.dst[k] = dst_offsets[k];
        T.prefix[k + 1] = T.prefix[k] + counts[k];
    }
    sph_launch_copy_segments(T, h->pos4[dst_buf], h->vel4[dst_buf], h->compute);
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

int sph_slab_density(sph_handle *h, int buf, int i_begin, int i_end, int n_all) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, buf, i_begin, i_end, n_all, true);
    if (rc) return rc;
    SweepArgs A = slab_sweep_args(h, i_begin, i_end, n_all);
    h->slabOwnedBegin = i_begin;
    h->slabOwnedEnd = i_end;
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->kt.density, &pe))) return rc;
    if ((rc = launch_density(h, A, h->compute))) return rc;
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

int sph_slab_force(sph_handle *h, int buf, int i_begin, int i_end, int n_all) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, buf, i_begin, i_end, n_all, true);
    if (rc) return rc;
    SweepArgs A = slab_sweep_args(h, i_begin, i_end, n_all);
    A.quietAll = nullptr; // (rows next to the halo layers, whose quiet bits nobody computed here: no all-quiet skip)
    A.patchHalo = 1;
    PairEvent *pe = nullptr;
    if ((rc = pair_begin(h, &h->kt.force, &pe))) return rc;
    sph_launch_force(h->P, A, h->opt.math_mode, h->opt.sweep, h->compute);
    HIPCHK(h, hipEventRecord(pe->b, h->compute));
    HIPCHK(h, hipGetLastError());
    h->kt.steps += 1;
    return SPH_OK;
}

int sph_slab_patch_halo(sph_handle *h, int buf, int i_begin, int i_end, int n_all, void *hip_stream) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, buf, i_begin, i_end, n_all, true);
    if (rc) return rc;
    if (h->opt.sweep != SPH_SWEEP_LIST) return SPH_OK; // the other sweeps read vel4 directly
    SweepArgs A = make_sweep_args(h);
    A.i_begin = i_begin;
    A.i_end = i_end;
    A.n_all = n_all;
    sph_launch_patch_halo(A, hip_stream ? (hipStream_t)hip_stream : h->compute);
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

int sph_slab_apply_click(sph_handle *h, int buf, int mx, int my, int z_lo, int z_hi) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    if (!h->external || !h->pos4[0]) return fail(h, SPH_ESTATE, "sph_bind_buffers first");
    if (buf != 0 && buf != 1) return fail(h, SPH_EINVAL, "bad buffer index");
    if (h->opt.sweep == SPH_SWEEP_LINKED)
        return fail(h, SPH_ESTATE, "the click impulse is not available with SPH_SWEEP_LINKED");
    if (!h->gridValid || h->sorted != (buf ^ 1))
        return fail(h, SPH_ESTATE, "click needs a completed slab step (it reuses that step's grid)");
    sph_launch_click(h->P, h->cellRange, h->vel4[buf], mx, my, h->compute, z_lo, z_hi);
    HIPCHK(h, hipGetLastError());
    return SPH_OK;
}

int sph_slab_force_ranges(sph_handle *h, int buf, int i_origin, int a0, int b0, int a1, int b1,
                          int n_all, int last, void *hip_stream) {
    if (!h) return SPH_EINVAL;
    SPH_ON_DEVICE(h);
    int rc = slab_range_ok(h, buf, a0, b0 > a0 ? b0 : a0, n_all);
    if (!rc) rc = slab_range_ok(h, buf, a1, b1 > a1 ? b1 : a1, n_all);
    if (rc) return rc;
    if (i_origin < 0 || (b0 > a0 && i_origin > a0) || (b1 > a1 && (i_origin > a1 || a1 < b0)))
        return fail(h, SPH_EINVAL, "bad wave origin / ranges must ascend");
    if ((rc = slab_sorted_ok(h, buf))) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->compute;
    if (b0 > a0 || b1 > a1) {
        SweepArgs A = slab_sweep_args(h, a0, b0 > a0 ? b0 : a0, n_all); // (rows and chunk: set per launch below)
        A.i_origin = i_origin & ~63; // (the same rounding as sph_slab_density)
        A.patchHalo = 0;
        if (A.quietAll) {
            // the last launch of the step holds the rows next to the halo layers (exchange B is through on this
            // stream): "every row is quiet" needs the halo rows' word too.  Earlier launches are interior rows by
            // contract -- every neighbour an owned row.
            if (last && h->opt.sweep == SPH_SWEEP_LIST && h->slabOwnedEnd > h->slabOwnedBegin && h->slabOwnedEnd <= n_all) {
                uint32_t *halo = A.quietAll + 1;
                sph_launch_halo_quiet(h->pv8, h->slabOwnedBegin, h->slabOwnedEnd, n_all, h->quietVref, A.quietAll, halo, s);
                A.quietHalo = halo;
            } else if (last) {
                A.quietAll = nullptr;
            }
        }
        PairEvent *pe = nullptr;
        if ((rc = pair_begin(h, &h->kt.force, &pe, s))) return rc;
        if (h->opt.sweep == SPH_SWEEP_LIST) { // both ranges in one launch: one grid, one tail
            A.i_begin = a0;
            A.i_end = b0 > a0 ? b0 : a0;
            A.i_begin2 = a1;
            A.i_end2 = b1 > a1 ? b1 : a1;
            A.tileChunk = tile_chunk(h, (b0 > a0 ? b0 - a0 : 0) + (b1 > a1 ? b1 - a1 : 0), h->zLayers);
            sph_launch_force(h->P, A, h->opt.math_mode, h->opt.sweep, s);
        } else {
            for (int k = 0; k < 2; ++k) {
                A.i_begin = k ? a1 : a0;
                A.i_end = k ? b1 : b0;
                if (A.i_end <= A.i_begin) continue;
                A.tileChunk = tile_chunk(h, A.i_end - A.i_begin, h->zLayers);
                sph_launch_force(h->P, A, h->opt.math_mode, h->opt.sweep, s);
            }
        }
        HIPCHK(h, hipEventRecord(pe->b, s));
        HIPCHK(h, hipGetLastError());
    }
    if (last) h->kt.steps += 1;
    return SPH_OK;
}

} // extern "C"
