// The multi-GPU driver's object: create / destroy, the slabs' buffers, the cutting and re-cutting of
// the global row sequence into slabs, the optional worker threads, and the read-back of the state.
#include "mgpu_driver.h"

#include <algorithm>
#include <cstdlib>

using namespace mgpu_host;

namespace {

thread_local std::string g_create_error;

void start_workers(sph_mgpu *m) {
    Workers *w = new Workers();
    const int n = (int)m->slabs.size();
    w->rc.assign(n, SPH_OK);
    for (int k = 0; k < n; ++k)
        w->threads.emplace_back([w, k]() {
            long long seen = 0;
            for (;;) {
                const std::function<int(int)> *job;
                {
                    std::unique_lock<std::mutex> lk(w->mu);
                    w->wake.wait(lk, [&] { return w->stop || w->generation != seen; });
                    if (w->stop) return;
                    seen = w->generation;
                    job = w->job;
                }
                const int rc = (*job)(k);
                {
                    std::lock_guard<std::mutex> lk(w->mu);
                    w->rc[k] = rc;
                    if (--w->pending == 0) w->done.notify_all();
                }
            }
        });
    m->workers = w;
}

void stop_workers(sph_mgpu *m) {
    Workers *w = m->workers;
    if (!w) return;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->stop = true;
        w->wake.notify_all();
    }
    for (auto &t : w->threads) t.join();
    delete w;
    m->workers = nullptr;
}

int layer_of(const sph_mgpu *m, float z) {
    int c = (int)(z / m->settings.h); // getGridCell: IEEE divide, truncation (simulator.cu:59)
    return std::min(std::max(c, 0), m->D - 1);
}

// Release the slab's resources; its identity (rank, device, communicator) stays.
void free_slab(Slab &sl) {
    (void)hipSetDevice(sl.device);
    if (sl.h) sph_destroy(sl.h);
    if (sl.comm) (void)hipStreamDestroy(sl.comm);
    if (sl.bnd) (void)hipStreamDestroy(sl.bnd);
    if (sl.copy) (void)hipStreamDestroy(sl.copy);
    static_cast<SlabResources &>(sl) = SlabResources{}; // (every buffer and event)
}

// (Re)build the slabs' buffers for capacity m->cap / face capacity m->F.
int alloc_slab(sph_mgpu *m, Slab &sl) {
    HIPM(m, hipSetDevice(sl.device));
    SphOptions o{};
    o.struct_size = (int32_t)sizeof o;
    o.device = sl.device;
    o.math_mode = m->opt.math_mode;
    o.sweep = m->opt.sweep;
    o.flags = SPH_FLAG_EXTERNAL_STATE | SPH_FLAG_NO_READBACK;
    o.capacity = m->cap;
    int rc = sph_create(&m->settings, &o, &sl.h);
    if (rc) return fail(m, rc, std::string("sph_create: ") + sph_last_error(nullptr));
    for (int b = 0; b < 2; ++b) { // (the overflow round's ex_pos / ex_vel: ensure_extra, when one comes)
        for (DeviceBuf<F4> *state : {&sl.pos[b], &sl.vel[b]}) {
            if (m->cap) HIPM(m, state->alloc((size_t)m->cap));
            HIPM(m, hipMemset(*state, 0, (size_t)m->cap * sizeof(F4)));
        }
        if (m->F) HIPM(m, sl.rx_pos[b].alloc((size_t)m->F));
        if (m->F) HIPM(m, sl.rx_vel[b].alloc((size_t)m->F));
    }
    SPHM(m, sl, sph_bind_buffers(sl.h, sl.pos[0], sl.vel[0], sl.pos[1], sl.vel[1], m->cap));
    HIPM(m, sl.hdr_tx.alloc(1));
    HIPM(m, sl.hdr_rx.alloc(2));
    HIPM(m, sl.sortb.alloc(8));
    HIPM(m, hipMemset(sl.hdr_tx, 0, sizeof(Hdr)));
    HIPM(m, hipMemset(sl.hdr_rx, 0, 2 * sizeof(Hdr)));
    HIPM(m, sl.pinned.alloc(1));
    *sl.pinned = Pinned{};
    HIPM(m, sl.hostRows.alloc((size_t)m->cap));
    for (Event *e : {&sl.evDensity, &sl.evB, &sl.evBnd, &sl.evForce, &sl.evCopy, &sl.evTx[0], &sl.evTx[1], &sl.evRx[0], &sl.evRx[1]})
        HIPM(m, e->create(hipEventDisableTiming));
    for (auto &e : sl.evT) HIPM(m, e.create());
    HIPM(m, hipStreamCreateWithFlags(&sl.copy, hipStreamNonBlocking));
    if (m->shared_stream) {
        SPHM(m, sl, sph_set_stream(sl.h, m->shared));
        sl.s = m->shared;
        sl.comm = nullptr;
    } else {
        sl.s = (hipStream_t)sph_get_stream(sl.h);
        HIPM(m, hipStreamCreateWithFlags(&sl.comm, hipStreamNonBlocking));
        HIPM(m, hipStreamCreateWithFlags(&sl.bnd, hipStreamNonBlocking));
    }
    HIPM(m, hipDeviceSynchronize());
    return SPH_OK;
}

// Hand the global row sequence `p4/v4` (n rows, any order that is the canonical
// sequence: particle-id order at step 0, rank-concatenated sorted order later) out to the
// slabs: stable filter by the z-layer of each row.
int distribute(sph_mgpu *m, const std::vector<F4> &p4, const std::vector<F4> &v4) {
    const int n = (int)p4.size();
    std::vector<long long> hist(m->D, 0);
    std::vector<int> lay(n);
    for (int i = 0; i < n; ++i) {
        lay[i] = layer_of(m, p4[i].z);
        hist[lay[i]]++;
    }
    const int world = m->opt.world;
    if (world * 2 > m->D) return fail(m, SPH_EINVAL, "too many slabs for the grid");
    m->cuts = partition_layers(hist, world, 2);
    std::vector<long long> per(world, 0);
    long long layerMax = 0;
    for (int z = 0; z < m->D; ++z) layerMax = std::max(layerMax, hist[z]);
    for (int r = 0; r < world; ++r)
        for (int z = m->cuts[r]; z < m->cuts[r + 1]; ++z) per[r] += hist[z];
    const long long biggest = *std::max_element(per.begin(), per.end());
    int cap = m->opt.slab_capacity > 0 ? m->opt.slab_capacity : (int)(biggest * 1.6) + 65536;
    int F = m->opt.face_capacity > 0 ? m->opt.face_capacity : (int)(1.25 * (double)layerMax) + 4096;
    F = std::min(F, cap);
    if (biggest + 2 * layerMax > cap && m->opt.slab_capacity > 0)
        return fail(m, SPH_EINVAL, "slab_capacity too small for the largest slab plus its halos");
    // buffers are only re-made when they have to grow (a re-cut keeps them)
    const bool fits = m->slabs[0].h && m->cap >= (int)(biggest * 1.3) + 2 * (int)layerMax &&
                      (m->opt.face_capacity > 0 || m->F >= (int)(1.1 * (double)layerMax)) &&
                      (m->opt.slab_capacity == 0 || m->cap == cap);
    if (!fits) {
        m->cap = cap;
        m->F = F;
        for (auto &sl : m->slabs) {
            free_slab(sl);
            PASS(alloc_slab(m, sl));
        }
    }
    std::vector<F4> sp, sv;
    for (auto &sl : m->slabs) {
        sl.zlo = m->cuts[sl.rank];
        sl.zhi = m->cuts[sl.rank + 1];
        sl.has_dn = sl.rank > 0;
        sl.has_up = sl.rank < world - 1;
        sp.clear();
        sv.clear();
        for (int i = 0; i < n; ++i)
            if (lay[i] >= sl.zlo && lay[i] < sl.zhi) {
                sp.push_back(p4[i]);
                sv.push_back(v4[i]);
            }
        if ((int)sp.size() > m->cap) return fail(m, SPH_EINVAL, "slab capacity too small");
        HIPM(m, hipSetDevice(sl.device));
        HIPM(m, hipStreamSynchronize(sl.s));
        HIPM(m, hipStreamSynchronize(sl.copy));
        if (!sp.empty()) {
            // through the slab's pinned read-back buffer (cap rows): a hipMemcpy from pageable
            // memory leaves a deferred unpin behind that stalls the first steps
            const size_t bytes = sp.size() * sizeof(F4);
            memcpy(sl.hostRows, sp.data(), bytes);
            HIPM(m, hipMemcpyAsync(sl.pos[0], sl.hostRows, bytes, hipMemcpyHostToDevice, sl.s));
            HIPM(m, hipStreamSynchronize(sl.s));
            memcpy(sl.hostRows, sv.data(), bytes);
            HIPM(m, hipMemcpyAsync(sl.vel[0], sl.hostRows, bytes, hipMemcpyHostToDevice, sl.s));
            HIPM(m, hipStreamSynchronize(sl.s));
        }
        sl.cur = 0;
        sl.off = 0;
        sl.n_own = (int)sp.size();
        sl.expectValid = false;
        sl.copyPending = false;
        sl.hostRowsCount = 0;
        sl.rowsStale = true; // hostRows served as the upload's staging buffer
        sl.status = 0;
    }
    m->hostPosValid = false;
    return SPH_OK;
}

// the rank-concatenated sequence of the LOCAL slabs' owned rows (device -> host)
int gather_local(sph_mgpu *m, std::vector<F4> &p4, std::vector<F4> &v4) {
    p4.clear();
    v4.clear();
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        HIPM(m, hipStreamSynchronize(sl.s));
        const size_t at = p4.size();
        p4.resize(at + sl.n_own);
        v4.resize(at + sl.n_own);
        if (sl.n_own) {
            HIPM(m, hipMemcpy(p4.data() + at, sl.pos[sl.cur] + sl.off, (size_t)sl.n_own * sizeof(F4), hipMemcpyDeviceToHost));
            HIPM(m, hipMemcpy(v4.data() + at, sl.vel[sl.cur] + sl.off, (size_t)sl.n_own * sizeof(F4), hipMemcpyDeviceToHost));
        }
    }
    return SPH_OK;
}

int upload_common(sph_mgpu *m, const float *pos, const float *vel, int n) {
    if (n != m->n) return fail(m, SPH_EINVAL, "particle count differs from settings");
    std::vector<F4> p4((size_t)n), v4((size_t)n);
    const float hh = m->settings.h;
    for (int i = 0; i < n; ++i) {
        const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
        // (range test before any float -> int conversion: that of a NaN / out-of-range value is undefined on the host)
        const float qx = x / hh, qy = y / hh, qz = z / hh, Df = (float)m->D;
        if (!(qx >= 0.f && qx < Df && qy >= 0.f && qy < Df && qz >= 0.f && qz < Df && x >= 0.f && y >= 0.f && z >= 0.f))
            return fail(m, SPH_EINVAL, "position outside the simulation box");
        uint32_t id = (uint32_t)i;
        float idbits;
        memcpy(&idbits, &id, 4);
        p4[i] = {x, y, z, idbits};
        v4[i] = vel ? F4{vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], 0.f} : F4{0.f, 0.f, 0.f, 0.f};
    }
    m->phase = 0; // a fresh state also clears whatever a failed step left half-done
    m->poisoned = false;
    m->overflow = false;
    m->clickQueued = false;
    PASS(distribute(m, p4, v4));
    m->ready = true;
    m->step = 0;
    return SPH_OK;
}

// Scatter `rows` rows (pos4 with the particle id in .w; vel4 with rho in .w) into the caller's arrays in
// particle-id order; vel / rho may be null.  False: a row carries an id outside [0, n).
bool scatter_by_id(int n, const F4 *p4, const F4 *v4, size_t rows, float *pos, float *vel, float *rho) {
    for (size_t i = 0; i < rows; ++i) {
        uint32_t id;
        memcpy(&id, &p4[i].w, 4);
        if (id >= (uint32_t)n) return false;
        if (pos) { pos[3 * id] = p4[i].x; pos[3 * id + 1] = p4[i].y; pos[3 * id + 2] = p4[i].z; }
        if (vel) { vel[3 * id] = v4[i].x; vel[3 * id + 1] = v4[i].y; vel[3 * id + 2] = v4[i].z; }
        if (rho) rho[id] = v4[i].w;
    }
    return true;
}
const char *const kCorruptId = "corrupt particle id in device state";

} // namespace

int mgpu_host::fail(sph_mgpu *m, int code, const std::string &msg) {
    if (m) {
        std::lock_guard<std::mutex> lk(m->errMu);
        m->err = msg;
    } else {
        g_create_error = msg;
    }
    return code;
}

int mgpu_host::poison(sph_mgpu *m, int code, const std::string &msg) {
    if (!distributed(m)) return fail(m, code, msg);
    if (!m->poisoned) {
        m->poisoned = true;
        m->poisonCode = code;
        (void)fail(m, code, msg);
        for (auto &sl : m->slabs) sl.status = 1;
    }
    return SPH_OK;
}

int mgpu_host::for_each_slab(sph_mgpu *m, const std::function<int(Slab &)> &fn) {
    Workers *w = m->workers;
    if (!w) {
        for (auto &sl : m->slabs) PASS(fn(sl));
        return SPH_OK;
    }
    const std::function<int(int)> job = [&](int k) { return fn(m->slabs[k]); };
    {
        std::unique_lock<std::mutex> lk(w->mu);
        w->job = &job;
        w->pending = (int)w->threads.size();
        std::fill(w->rc.begin(), w->rc.end(), SPH_OK);
        ++w->generation;
        w->wake.notify_all();
        w->done.wait(lk, [&] { return w->pending == 0; });
        w->job = nullptr;
    }
    for (int rc : w->rc) PASS(rc);
    return SPH_OK;
}

int mgpu_host::recut(sph_mgpu *m) {
    if ((int)m->slabs.size() != m->opt.world) return SPH_OK; // needs the whole sequence in one process
    std::vector<F4> p4, v4;
    PASS(gather_local(m, p4, v4));
    const std::vector<int> before = m->cuts;
    PASS(distribute(m, p4, v4));
    if (m->cuts != before) m->stats.recuts++;
    return SPH_OK;
}

extern "C" {

const char *sph_mgpu_last_error(const sph_mgpu *m) { return m ? m->err.c_str() : g_create_error.c_str(); }

int sph_mgpu_unique_id(void *out128) {
    if (!out128) return SPH_EINVAL;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return SPH_EHIP;
    static_assert(sizeof(id) == 128, "ncclUniqueId");
    memcpy(out128, &id, sizeof id);
    return SPH_OK;
}

int sph_mgpu_create(const SphSettings *settings, const SphMgpuOptions *options, const void *unique_id128,
                    sph_mgpu **out) {
    if (!settings || !options || !out) return fail(nullptr, SPH_EINVAL, "null argument");
    *out = nullptr;
    SphMgpuOptions o{};
    const size_t sz = options->struct_size > 0 ? (size_t)options->struct_size : sizeof o;
    memcpy(&o, options, std::min(sz, sizeof o));
    if (o.world < 1 || o.rank_count < 1 || o.rank_count > SPH_MGPU_MAX_LOCAL || o.rank_begin < 0 ||
        o.rank_begin + o.rank_count > o.world)
        return fail(nullptr, SPH_EINVAL, "bad world / rank range");
    if (o.transport < SPH_TRANSPORT_LOOPBACK || o.transport > SPH_TRANSPORT_STREAMS)
        return fail(nullptr, SPH_EINVAL, "unknown transport");
    if ((o.transport == SPH_TRANSPORT_LOOPBACK || o.transport == SPH_TRANSPORT_RCCL_SELF ||
         o.transport == SPH_TRANSPORT_STREAMS) && o.rank_count != o.world)
        return fail(nullptr, SPH_EINVAL, "loopback / self transports need every slab in this process");
    if (o.transport == SPH_TRANSPORT_MAILBOX && o.rank_count != 1)
        return fail(nullptr, SPH_EINVAL, "mailbox transport: one slab per driver object");
    if (o.transport == SPH_TRANSPORT_RCCL && o.rank_count != o.world && (o.rank_count != 1 || !unique_id128))
        return fail(nullptr, SPH_EINVAL, "one process per GPU: rank_count = 1 and a unique id");
    if (o.sweep != SPH_SWEEP_LIST && o.sweep != SPH_SWEEP_LDS && o.sweep != SPH_SWEEP_DIRECT)
        return fail(nullptr, SPH_EINVAL, "sweep variant not available in slab mode");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SPH_ENODEV, "no HIP device: libsph_mgpu has no CPU fallback by design");
    sph_mgpu *m = new (std::nothrow) sph_mgpu();
    if (!m) return fail(nullptr, SPH_ENOMEM, "out of host memory");
    m->settings = *settings;
    m->opt = o;
    m->n = settings->numParticles;
    m->D = (int)settings->numCellsPerDim;
    m->DD = m->D * m->D;
    m->shared_stream = o.transport != SPH_TRANSPORT_RCCL && o.transport != SPH_TRANSPORT_STREAMS;
    m->slabs.resize(o.rank_count);
    for (int k = 0; k < o.rank_count; ++k) {
        m->slabs[k].rank = o.rank_begin + k;
        m->slabs[k].device = o.transport == SPH_TRANSPORT_RCCL ? o.devices[k] : o.devices[0];
        if (m->slabs[k].device < 0 || m->slabs[k].device >= ndev) {
            delete m;
            return fail(nullptr, SPH_EINVAL, "device ordinal out of range");
        }
    }
    for (int r = 0; r + 1 < o.world; ++r) {
        Slab *lo = local(m, r), *hi = local(m, r + 1);
        if (lo || hi) m->faces.push_back({r, lo, hi});
    }
    int rc = SPH_OK;
    if (m->shared_stream && (hipSetDevice(m->slabs[0].device) != hipSuccess ||
                             hipStreamCreateWithFlags(&m->shared, hipStreamNonBlocking) != hipSuccess))
        rc = fail(nullptr, SPH_EHIP, "hipStreamCreate failed");
    if (!rc) rc = init_comms(m, unique_id128);
    if (rc) {
        sph_mgpu_destroy(m);
        return rc;
    }
    if (const char *e = getenv("SPH_MGPU_THREADS"))
        if (atoi(e) != 0 && m->slabs.size() > 1) start_workers(m);
    *out = m;
    return SPH_OK;
}

void sph_mgpu_destroy(sph_mgpu *m) {
    if (!m) return;
    stop_workers(m);
    for (auto &sl : m->slabs) {
        (void)hipSetDevice(sl.device);
        if (sl.s) (void)hipStreamSynchronize(sl.s);
        if (sl.comm) (void)hipStreamSynchronize(sl.comm);
        if (sl.copy) (void)hipStreamSynchronize(sl.copy);
    }
    destroy_comms(m);
    for (auto &sl : m->slabs) free_slab(sl);
    if (m->shared) (void)hipStreamDestroy(m->shared);
    delete m;
}

int sph_mgpu_setup(sph_mgpu *m) {
    if (!m) return SPH_EINVAL;
    std::vector<float> pos((size_t)std::max(m->n, 1) * 3, 0.f);
    int rc = sph_initial_positions(&m->settings, pos.data());
    if (rc) return fail(m, rc, "sph_initial_positions failed");
    return upload_common(m, pos.data(), nullptr, m->n);
}

int sph_mgpu_upload_state(sph_mgpu *m, const float *pos_xyz, const float *vel_xyz, int n) {
    if (!m || (!pos_xyz && n > 0)) return fail(m, SPH_EINVAL, "null argument");
    return upload_common(m, pos_xyz, vel_xyz, n);
}

const float *sph_mgpu_positions_host(sph_mgpu *m) {
    if (!m) return nullptr;
    if (m->hostPos.size() != (size_t)m->n * 3) m->hostPos.assign((size_t)m->n * 3, 0.f);
    if (m->hostPosValid) return m->hostPos.data();
    auto failed = [m](const char *msg) -> const float * { m->err = msg; return nullptr; };
    for (auto &sl : m->slabs) {
        if (hipSetDevice(sl.device) != hipSuccess || hipStreamSynchronize(sl.copy) != hipSuccess)
            return failed("stream synchronize failed");
        if (sl.rowsStale) { // before the first step, or right after a re-cut: the uploaded state itself
            if (hipStreamSynchronize(sl.s) != hipSuccess) return failed("stream synchronize failed");
            if (sl.n_own && hipMemcpy(sl.hostRows, sl.pos[sl.cur] + sl.off, (size_t)sl.n_own * sizeof(F4),
                                      hipMemcpyDeviceToHost) != hipSuccess)
                return failed("hipMemcpy failed");
            sl.hostRowsCount = sl.n_own;
            sl.rowsStale = false;
        }
        if (!scatter_by_id(m->n, sl.hostRows, nullptr, (size_t)sl.hostRowsCount, m->hostPos.data(), nullptr, nullptr))
            return failed(kCorruptId);
    }
    m->hostPosValid = true;
    return m->hostPos.data();
}

int sph_mgpu_download_state(sph_mgpu *m, float *pos, float *vel, float *rho, int *written) {
    if (!m) return SPH_EINVAL;
    PASS(sph_mgpu_sync(m));
    std::vector<F4> p4, v4;
    PASS(gather_local(m, p4, v4));
    if (!scatter_by_id(m->n, p4.data(), v4.data(), p4.size(), pos, vel, rho)) return fail(m, SPH_EHIP, kCorruptId);
    if (written) *written = (int)p4.size();
    return SPH_OK;
}

int sph_mgpu_diagnostics(sph_mgpu *m, const SphDiagnosticsOptions *opt, SphDiagnosticsRaw *out) {
    if (!m || !out) return SPH_EINVAL;
    if (!m->ready) return fail(m, SPH_ESTATE, "setup()/upload_state() must come first");
    if (m->poisoned) return m->poisonCode; // (err holds the message)
    if (m->phase != 0) return fail(m, SPH_ESTATE, "diagnose between steps");
    // every slab queues its reduction behind its last step (the owned rows: what gather_local copies) ...
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        SPHM(m, sl, sph_slab_diagnose(sl.h, sl.cur, sl.off, sl.off + sl.n_own, opt));
    }
    // ... then the host waits for each and merges
    bool first = true;
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        SphDiagnosticsRaw part;
        SPHM(m, sl, sph_diagnostics_host(sl.h, &part));
        if (first) *out = part;
        else if (sph_diagnostics_add(out, &part)) return fail(m, SPH_EHIP, "the slabs' diagnostics do not merge");
        first = false;
    }
    return SPH_OK;
}

int sph_mgpu_get_stats(sph_mgpu *m, SphMgpuStats *out, int reset) {
    if (!m || !out) return SPH_EINVAL;
    PASS(sph_mgpu_sync(m));
    m->stats.local_slabs = (int)m->slabs.size();
    for (size_t k = 0; k < m->slabs.size(); ++k) {
        Slab &sl = m->slabs[k];
        HIPM(m, hipSetDevice(sl.device));
        SphKernelTimes kt{};
        SPHM(m, sl, sph_get_kernel_times(sl.h, &kt, reset));
        m->stats.owned[k] = sl.n_own;
        m->stats.grid_s[k] = kt.hash + kt.sort + kt.gather;
        m->stats.density_s[k] = kt.density;
        m->stats.force_s[k] = kt.force;
        m->stats.kernel_s[k] = m->stats.grid_s[k] + kt.density + kt.force;
    }
    *out = m->stats;
    if (reset) {
        const int ls = m->stats.local_slabs;
        m->stats = SphMgpuStats{};
        m->stats.local_slabs = ls;
    }
    return SPH_OK;
}

} // extern "C"
