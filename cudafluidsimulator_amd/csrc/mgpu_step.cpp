// The multi-GPU driver's step: four phases, the farewell of a driver whose checks failed, and the
// entry points that run them.
#include "mgpu_driver.h"

#include <algorithm>

using namespace mgpu_host;

namespace {

// (a neighbour that has said farewell takes part in no further round)
bool said_farewell(const Slab *lo, const Slab *hi) { return (lo && lo->nb_up.status) || (hi && hi->nb_dn.status); }

// last step's derived bounds against what the sort actually found (call with sl.expectValid)
bool sort_bounds_match(const Slab &sl) { return std::equal(sl.expect, sl.expect + 4, sl.pinned->sort); }

struct Piece { const F4 *p, *v; int count, at; }; // a row range bound for rows at.. of the combined array

// pieces holding payload rows [a, b) of the message received from below (which = 0: an UP
// message) or from above (which = 1: a DOWN message), bound for rows at.. of the combined array
void payload_rows(const sph_mgpu *m, const Slab &sl, int which, int a, int b, int at, std::vector<Piece> &out) {
    if (b <= a) return;
    const F4 *rp = sl.rx_pos[which], *rv = sl.rx_vel[which];
    auto add = [&](const F4 *p, const F4 *v, int rows) { out.push_back({p, v, rows, at}); at += rows; };
    if (which == 0) { // extra rows come FIRST, the window holds the rest
        const Layout L = up_layout(sl.nb_dn, m->F);
        if (a < L.extra) add(sl.ex_pos[0] + a, sl.ex_vel[0] + a, std::min(b, L.extra) - a);
        const int lo = std::max(a, L.extra) - L.extra;
        if (b > L.extra) add(rp + L.offset + lo, rv + L.offset + lo, (b - L.extra) - lo);
    } else { // the window holds rows [0, F), the extra rows follow
        const Layout L = down_layout(sl.nb_up, m->F);
        const int inwin = L.payload - L.extra;
        if (a < inwin) add(rp + L.offset + a, rv + L.offset + a, std::min(b, inwin) - a);
        const int lo = std::max(a, inwin) - inwin;
        if (b > inwin) add(sl.ex_pos[1] + lo, sl.ex_vel[1] + lo, (b - inwin) - lo);
    }
}

int ensure_extra(sph_mgpu *m, Slab &sl, int which, int rows) {
    if (rows <= sl.ex_cap[which]) return SPH_OK;
    const int capr = rows + rows / 4 + 1024;
    sl.ex_cap[which] = 0;
    HIPM(m, sl.ex_pos[which].alloc((size_t)capr));
    HIPM(m, sl.ex_vel[which].alloc((size_t)capr));
    sl.ex_cap[which] = capr;
    return SPH_OK;
}

// Exchange A, one round: per face the header and the two fixed-size windows (F rows of positions, of
// velocities) of the lower slab going up, then those of the upper slab going down.  Phase 1 and the
// farewell post the SAME calls per face: a stopping rank's neighbour waits in this round of its next step.
std::vector<Msg> exchange_a(sph_mgpu *m, bool farewell) {
    const size_t W = (size_t)m->F * sizeof(F4);
    std::vector<Msg> msgs;
    for (const auto [r, lo, hi] : m->faces) {
        // the farewell: not where both ends are here (stopping together) or the other end is gone already
        if (farewell && ((lo && hi) || said_farewell(lo, hi))) continue;
        // the step: of the partitioned array, the UP window is the last F rows and the DOWN window the
        // first F; the farewell: nobody reads the windows, the first rows of buffer 0 will do
        const int ub = lo && !farewell ? lo->sbuf : 0, w0 = lo && !farewell ? std::max(lo->n_own - m->F, 0) : 0;
        const int db = hi && !farewell ? hi->sbuf : 0;
        // r -> r+1: the UP message of r lands in hi's slot [0] (from below)
        msgs.push_back({r, r + 1, lo ? lo->hdr_tx : nullptr, hi ? &hi->hdr_rx[0] : nullptr, sizeof(Hdr)});
        msgs.push_back({r, r + 1, lo ? lo->pos[ub] + w0 : nullptr, hi ? hi->rx_pos[0] : nullptr, W});
        msgs.push_back({r, r + 1, lo ? lo->vel[ub] + w0 : nullptr, hi ? hi->rx_vel[0] : nullptr, W});
        // r+1 -> r: the DOWN message of r+1 lands in lo's slot [1] (from above)
        msgs.push_back({r + 1, r, hi ? hi->hdr_tx : nullptr, lo ? &lo->hdr_rx[1] : nullptr, sizeof(Hdr)});
        msgs.push_back({r + 1, r, hi ? hi->pos[db] : nullptr, lo ? lo->rx_pos[1] : nullptr, W});
        msgs.push_back({r + 1, r, hi ? hi->vel[db] : nullptr, lo ? lo->rx_vel[1] : nullptr, W});
    }
    return msgs;
}

// A step in four phases; between two phases every message posted so far has been handed
// to the transport (RCCL / copies: at once; mailbox: completed at the start of the next).
int step_phase1(sph_mgpu *m, SphTimes *times) {
    const int DD = m->DD;
    m->t_begin = std::chrono::steady_clock::now();

    // ---- 1. partition the owned rows by the z-range of their NEW cell (no host round trip)
    PASS(for_each_slab(m, [&](Slab &sl) -> int {
        HIPM(m, hipSetDevice(sl.device));
        if (times) HIPM(m, hipEventRecord(sl.evT[0], sl.s));
        const uint32_t thr[6] = {(uint32_t)(std::max(sl.zlo - 1, 0) * DD), (uint32_t)(sl.zlo * DD),
                                 (uint32_t)((sl.zlo + 1) * DD),            (uint32_t)((sl.zhi - 1) * DD),
                                 (uint32_t)(sl.zhi * DD),                  (uint32_t)((sl.zhi + 1) * DD)};
        SPHM(m, sl, sph_slab_partition_async(sl.h, sl.cur, sl.off, sl.n_own, thr, 6, sl.hdr_tx));
        // status word rides in the header: a rank that failed tells its neighbours
        sl.pinned->status = sl.status;
        HIPM(m, hipMemcpyAsync(&sl.hdr_tx->status, &sl.pinned->status, sizeof(int), hipMemcpyHostToDevice, sl.s));
        HIPM(m, hipMemcpyAsync(&sl.pinned->mine, sl.hdr_tx, sizeof(Hdr), hipMemcpyDeviceToHost, sl.s));
        sl.sbuf = sl.cur ^ 1;
        return SPH_OK;
    }));
    // ---- 2. exchange A: header + fixed-size windows, one round
    return deliver(m, exchange_a(m, false), false);
}

int step_phase2(sph_mgpu *m) {
    const int F = m->F;
    PASS(resolve_mail(m));
    // ---- 3. the step's ONE host synchronisation: own bounds + the neighbours' headers
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        HIPM(m, hipMemcpyAsync(sl.pinned->rx, sl.hdr_rx, 2 * sizeof(Hdr), hipMemcpyDeviceToHost, sl.s));
    }
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        HIPM(m, hipStreamSynchronize(sl.s));
    }
    m->stats.host_syncs++;
    bool overflow = false;
    m->overflow = false;
    for (auto &sl : m->slabs) {
        sl.mine = sl.pinned->mine;
        sl.nb_dn = sl.has_dn ? sl.pinned->rx[0] : Hdr{};
        sl.nb_up = sl.has_up ? sl.pinned->rx[1] : Hdr{};
        if (sl.expectValid) {
            if (!sort_bounds_match(sl)) sl.status = 1;
            if (sl.status)
                POISON(m, SPH_ESTATE,
                       "slab " + std::to_string(sl.rank) +
                           ": a particle crossed into a neighbour slab beyond its far boundary layer "
                           "(or out of it) in one step: z-velocity too high for this decomposition");
        }
        if ((sl.has_dn && sl.nb_dn.status) || (sl.has_up && sl.nb_up.status)) {
            sl.status = 1;
            POISON(m, SPH_ESTATE, "slab " + std::to_string(sl.rank) + ": a neighbour slab reported a failure");
        }
        // (what a slab would send down is what a slab below it would see coming from above, and vice versa)
        if (!sl.has_dn && from_above(sl.mine).mig != 0) POISON(m, SPH_ESTATE, "particles below the lowest slab");
        if (!sl.has_up && from_below(sl.mine).mig != 0) POISON(m, SPH_ESTATE, "particles above the highest slab");
        if (sl.has_dn && !sl.nb_dn.status && (down_layout(sl.mine, F).extra || up_layout(sl.nb_dn, F).extra)) overflow = true;
        if (sl.has_up && !sl.nb_up.status && (up_layout(sl.mine, F).extra || down_layout(sl.nb_up, F).extra)) overflow = true;
    }
    // ---- 3b. (rare) a face outgrew its fixed-size message: exact-size second round
    if (overflow) {
        m->overflow = true;
        m->stats.overflow_rounds++;
        std::vector<Msg> msgs;
        for (auto &sl : m->slabs) {
            HIPM(m, hipSetDevice(sl.device));
            if (sl.has_dn) PASS(ensure_extra(m, sl, 0, up_layout(sl.nb_dn, F).extra));
            if (sl.has_up) PASS(ensure_extra(m, sl, 1, down_layout(sl.nb_up, F).extra));
        }
        for (const auto [r, lo, hi] : m->faces) {
            if (said_farewell(lo, hi)) continue;
            // UP excess of r: rows [b3, b3+extra) of its partitioned array -> hi.ex[0]
            const Layout U = up_layout(lo ? lo->mine : hi->nb_dn, F), D = down_layout(hi ? hi->mine : lo->nb_up, F);
            if (U.extra) {
                const size_t B = (size_t)U.extra * sizeof(F4);
                msgs.push_back({r, r + 1, lo ? lo->pos[lo->sbuf] + U.extra_at : nullptr, hi ? hi->ex_pos[0] : nullptr, B});
                msgs.push_back({r, r + 1, lo ? lo->vel[lo->sbuf] + U.extra_at : nullptr, hi ? hi->ex_vel[0] : nullptr, B});
            }
            // DOWN excess of r+1: rows [F, b2) -> lo.ex[1]
            if (D.extra) {
                const size_t B = (size_t)D.extra * sizeof(F4);
                msgs.push_back({r + 1, r, hi ? hi->pos[hi->sbuf] + D.extra_at : nullptr, lo ? lo->ex_pos[1] : nullptr, B});
                msgs.push_back({r + 1, r, hi ? hi->vel[hi->sbuf] + D.extra_at : nullptr, lo ? lo->ex_vel[1] : nullptr, B});
            }
        }
        PASS(deliver(m, msgs, false));
    }
    return SPH_OK;
}

int step_phase3(sph_mgpu *m, SphTimes *times) {
    const int DD = m->DD;
    PASS(resolve_mail(m));
    // ---- 4. assemble, sort, density
    PASS(for_each_slab(m, [&](Slab &sl) -> int {
        HIPM(m, hipSetDevice(sl.device));
        const Assembly &as = sl.a = assemble(sl.mine, sl.nb_dn, sl.nb_up);
        if (as.n_comb > m->cap) POISON(m, SPH_ESTATE, "slab capacity exceeded by halo + migrants");
        if (as.i0 > as.e_lo || as.e_lo > as.s_hi || as.s_hi > as.i1)
            POISON(m, SPH_ESTATE, "slab " + std::to_string(sl.rank) + ": inconsistent exchange headers");
        if (m->poisoned) return SPH_OK; // the state is lost; only the step's remaining messages matter
        const int s = sl.sbuf, t = s ^ 1;
        std::vector<Piece> pieces;
        auto put_local = [&](int a, int b, int at) { if (b > a) pieces.push_back({sl.pos[s] + a, sl.vel[s] + a, b - a, at}); };
        auto put_rx = [&](int which, int a, int b, int at) { payload_rows(m, sl, which, a, b, at, pieces); };
        const Inflow &dn = as.dn, &up = as.up;
        put_rx(0, 0, dn.bnd, as.at[0]);               // from below: its upper boundary layer
        put_local(0, as.m0, as.at[1]);                // my migrants down
        put_rx(0, dn.bnd, dn.bnd + dn.mig, as.at[2]); // from below: its migrants up
        put_local(as.m0, as.m3, as.at[3]);            // what stays mine
        put_rx(1, 0, up.mig, as.at[4]);               // from above: its migrants down
        put_local(as.m3, as.n, as.at[5]);             // my migrants up
        put_rx(1, up.mig, up.mig + up.bnd, as.at[6]); // from above: its lower boundary layer
        if (sl.copyPending) { // the read-back of the last step still reads buffer t
            HIPM(m, hipStreamWaitEvent(sl.s, sl.evCopy, 0));
            sl.copyPending = false;
        }
        for (size_t a = 0; a < pieces.size(); a += 8) {
            const int k = (int)std::min<size_t>(8, pieces.size() - a);
            const void *sp[8], *sv[8];
            int32_t cnt[8], at[8];
            for (int q = 0; q < k; ++q) {
                const Piece &pc = pieces[a + q];
                sp[q] = pc.p, sv[q] = pc.v, cnt[q] = pc.count, at[q] = pc.at;
            }
            SPHM(m, sl, sph_slab_copy_segments(sl.h, t, k, sp, sv, cnt, at));
        }
        const uint32_t thr[4] = {(uint32_t)(sl.zlo * DD), (uint32_t)((sl.zlo + 1) * DD),
                                 (uint32_t)((sl.zhi - 1) * DD), (uint32_t)(sl.zhi * DD)};
        SPHM(m, sl, sph_slab_sort_async(sl.h, t, 0, as.n_comb, thr, 4, sl.sortb));
        HIPM(m, hipMemcpyAsync(sl.pinned->sort, sl.sortb, 4 * sizeof(int), hipMemcpyDeviceToHost, sl.s));
        const int expect[4] = {as.i0, as.e_lo, as.s_hi, as.i1};
        std::copy(expect, expect + 4, sl.expect);
        sl.expectValid = true;
        sl.sbuf = t ^ 1; // the sorted streams
        if (times) HIPM(m, hipEventRecord(sl.evT[1], sl.s));
        SPHM(m, sl, sph_slab_density(sl.h, sl.sbuf, as.i0, as.i1, as.n_comb));
        if (sl.comm) HIPM(m, hipEventRecord(sl.evDensity, sl.s));
        return SPH_OK;
    }));
    // ---- 5. exchange B (rho of the boundary layers, rides in vel4.w) || interior force sweep
    std::vector<Msg> msgs;
    const bool records = m->opt.sweep == SPH_SWEEP_LIST;
    // a row of what exchange B ships.  The list sweeps read neighbours from the interleaved (pos4, vel4) records,
    // into which the density sweep wrote rho: a boundary layer's records go straight into the neighbour's halo
    // rows (twice the bytes of vel4 alone -- a few hundred KB -- and no patch launch afterwards); the other
    // sweeps get vel4 rows.  A failed step: sizes as the headers dictate (the healthy neighbour posts the matching
    // calls), payload and destination anywhere inside the buffers -- their first rows: nothing will read them
    const size_t rowB = (records ? 2 : 1) * sizeof(F4);
    auto row = [&](Slab *sl, int k) -> F4 * {
        if (m->poisoned) return records ? static_cast<F4 *>(sph_slab_records(sl->h)) : sl->vel[0];
        return records ? static_cast<F4 *>(sph_slab_records(sl->h)) + 2 * (size_t)k : sl->vel[sl->sbuf] + k;
    };
    for (const auto [r, lo, hi] : m->faces) {
        // either end derives the counts from its own header and the one it received;
        // both ends in this process: the two derivations must agree
        const FaceB c = lo ? exchange_b(lo->mine, lo->nb_up) : exchange_b(hi->nb_dn, hi->mine);
        if (lo && hi && c != exchange_b(hi->nb_dn, hi->mine)) return fail(m, SPH_ESTATE, "exchange B plans disagree");
        if (said_farewell(lo, hi)) continue;
        if (m->poisoned && (c.up < 0 || c.down < 0 || c.up > m->cap || c.down > m->cap))
            return fail(m, SPH_ESTATE, "failed step: exchange sizes out of range");
        msgs.push_back({r, r + 1, lo ? row(lo, lo->a.s_hi) : nullptr, hi ? row(hi, hi->a.i0 - c.up) : nullptr, (size_t)c.up * rowB});
        msgs.push_back({r + 1, r, hi ? row(hi, hi->a.i0) : nullptr, lo ? row(lo, lo->a.i1) : nullptr, (size_t)c.down * rowB});
    }
    for (auto &sl : m->slabs)
        if (sl.comm) {
            HIPM(m, hipSetDevice(sl.device));
            if (m->poisoned) HIPM(m, hipEventRecord(sl.evDensity, sl.s)); // (no density sweep recorded it)
            HIPM(m, hipStreamWaitEvent(sl.comm, sl.evDensity, 0));
        }
    PASS(deliver(m, msgs, true));
    for (auto &sl : m->slabs)
        if (sl.comm) { HIPM(m, hipSetDevice(sl.device)); HIPM(m, hipEventRecord(sl.evB, sl.comm)); }
    return SPH_OK;
}

// The farewell of a poisoned driver: one more exchange A (header with status = 1 + the fixed-size windows)
// with every neighbour in another process that has not said farewell itself -- exactly the calls that
// neighbour posts in phase 1 of its next step -- then the error of the failed check.
int farewell(sph_mgpu *m) {
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        if (sl.bnd) HIPM(m, hipStreamSynchronize(sl.bnd));
        if (sl.comm) HIPM(m, hipStreamSynchronize(sl.comm)); // exchange B of this step is through
        sl.pinned->mine = Hdr{};
        sl.pinned->mine.status = 1;
        HIPM(m, hipMemcpyAsync(sl.hdr_tx, &sl.pinned->mine, sizeof(Hdr), hipMemcpyHostToDevice, sl.s));
    }
    PASS(deliver(m, exchange_a(m, true), false));
    if (m->opt.transport != SPH_TRANSPORT_MAILBOX)
        for (auto &sl : m->slabs) {
            HIPM(m, hipSetDevice(sl.device));
            HIPM(m, hipStreamSynchronize(sl.s));
        }
    return m->poisonCode; // (m->err still holds the message of the check that failed)
}

int step_phase4(sph_mgpu *m, SphTimes *times) {
    PASS(resolve_mail(m));
    if (m->poisoned) return farewell(m);
    PASS(for_each_slab(m, [&](Slab &sl) -> int {
        HIPM(m, hipSetDevice(sl.device));
        const int i0 = sl.a.i0, i1 = sl.a.i1, n_comb = sl.a.n_comb;
        const int a = sl.has_dn ? sl.a.e_lo : i0, b = sl.has_up ? sl.a.s_hi : i1;
        if (m->shared_stream) {
            // loopback / self transport: exchange B was delivered in stream order, there is
            // nothing to overlap -- the whole slab in ONE launch (one tail instead of two)
            if (m->opt.sweep != SPH_SWEEP_LIST) // (list: exchange B delivered whole records)
                SPHM(m, sl, sph_slab_patch_halo(sl.h, sl.sbuf, i0, i1, n_comb, nullptr));
            SPHM(m, sl, sph_slab_force_ranges(sl.h, sl.sbuf, i0, i0, i1, 0, 0, n_comb, 1, nullptr));
        } else {
            // interior layers: every neighbour is an owned row -> no need to wait for exchange B
            SPHM(m, sl, sph_slab_force_ranges(sl.h, sl.sbuf, i0, a, b, 0, 0, n_comb, 0, nullptr));
            // the two boundary layers in ONE launch once the halo densities are in: on a stream
            // of their own they join the interior's launch on the GPU instead of waiting for its
            // tail (with a shared stream -- loopback -- they simply follow it)
            hipStream_t bs = sl.bnd ? sl.bnd : sl.s;
            if (sl.bnd) HIPM(m, hipStreamWaitEvent(sl.bnd, sl.evB, 0));
            if (m->opt.sweep != SPH_SWEEP_LIST) SPHM(m, sl, sph_slab_patch_halo(sl.h, sl.sbuf, i0, i1, n_comb, bs));
            SPHM(m, sl, sph_slab_force_ranges(sl.h, sl.sbuf, i0, i0, a, b, i1, n_comb, 1, bs));
            if (sl.bnd) {
                HIPM(m, hipEventRecord(sl.evBnd, sl.bnd));
                HIPM(m, hipStreamWaitEvent(sl.s, sl.evBnd, 0));
            }
        }
        sl.cur = sl.sbuf ^ 1;
        sl.off = i0;
        sl.n_own = i1 - i0;
        // the click impulse of Simulator::simulate (simulator.cu:482-489) on the layers this slab owns:
        // new velocities, this step's (pre-integration) grid -- every row of an owned layer is an owned row
        if (m->clickQueued) SPHM(m, sl, sph_slab_apply_click(sl.h, sl.cur, m->clickX, m->clickY, sl.zlo, sl.zhi));
        if (times) HIPM(m, hipEventRecord(sl.evT[2], sl.s));
        // ---- 6. position read-back of the owned rows (simulator.cu:479-480), off the compute stream
        HIPM(m, hipEventRecord(sl.evForce, sl.s));
        HIPM(m, hipStreamWaitEvent(sl.copy, sl.evForce, 0));
        if (sl.n_own)
            HIPM(m, hipMemcpyAsync(sl.hostRows, sl.pos[sl.cur] + sl.off, (size_t)sl.n_own * sizeof(F4),
                                   hipMemcpyDeviceToHost, sl.copy));
        HIPM(m, hipEventRecord(sl.evCopy, sl.copy));
        sl.hostRowsCount = sl.n_own;
        sl.rowsStale = false;
        sl.copyPending = true;
        return SPH_OK;
    }));
    m->clickQueued = false;
    m->hostPosValid = false;
    m->step++;
    m->stats.steps++;
    if (times) {
        double grid = 0, sphu = 0;
        for (auto &sl : m->slabs) {
            HIPM(m, hipSetDevice(sl.device));
            HIPM(m, hipEventSynchronize(sl.evT[2]));
            float g = 0, u = 0;
            HIPM(m, hipEventElapsedTime(&g, sl.evT[0], sl.evT[1]));
            HIPM(m, hipEventElapsedTime(&u, sl.evT[1], sl.evT[2]));
            grid = std::max(grid, (double)g * 1e-3);
            sphu = std::max(sphu, (double)u * 1e-3);
        }
        times->buildGrid += grid;
        times->sphUpdate += sphu;
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - m->t_begin).count();
        times->memcpy += std::max(0.0, wall - grid - sphu); // host-visible rest: exchange waits + sync
        times->iters += 1;
    }
    if (m->opt.recut_every > 0 && m->step % m->opt.recut_every == 0) PASS(recut(m));
    return SPH_OK;
}

} // namespace

extern "C" {

int sph_mgpu_step_phase(sph_mgpu *m, int phase, SphTimes *times) {
    if (!m) return SPH_EINVAL;
    if (!m->ready) return fail(m, SPH_ESTATE, "setup()/upload_state() must come first");
    if (m->poisoned && m->phase == 0) return m->poisonCode; // (err holds the message; upload_state()/setup() starts over)
    if (phase < 1 || phase > 4 || phase != m->phase + 1) return fail(m, SPH_ESTATE, "step phases run 1, 2, 3, 4");
    int rc = phase == 1 ? step_phase1(m, times) : phase == 2 ? step_phase2(m)
             : phase == 3 ? step_phase3(m, times) : step_phase4(m, times);
    if (rc) {
        if (m->poisoned && phase == 4) m->phase = 0; // farewell sent: every later step reports the same failure
        return rc;
    }
    m->phase = phase == 4 ? 0 : phase;
    return SPH_OK;
}

int sph_mgpu_step(sph_mgpu *m, SphTimes *times) {
    if (!m) return SPH_EINVAL;
    if (m->opt.transport == SPH_TRANSPORT_MAILBOX)
        return fail(m, SPH_ESTATE, "mailbox transport: drive every rank's object with sph_mgpu_step_phase");
    for (int ph = 1; ph <= 4; ++ph) PASS(sph_mgpu_step_phase(m, ph, times));
    return SPH_OK;
}

int sph_mgpu_queue_click(sph_mgpu *m, int mouse_x, int mouse_y) {
    if (!m) return SPH_EINVAL;
    if (m->opt.sweep == SPH_SWEEP_LINKED) return fail(m, SPH_ESTATE, "the click impulse is not available with SPH_SWEEP_LINKED");
    if (m->phase != 0) return fail(m, SPH_ESTATE, "queue the click between steps");
    m->clickQueued = true;
    m->clickX = mouse_x;
    m->clickY = mouse_y;
    return SPH_OK;
}

int sph_mgpu_sync(sph_mgpu *m) {
    if (!m) return SPH_EINVAL;
    for (auto &sl : m->slabs) {
        HIPM(m, hipSetDevice(sl.device));
        HIPM(m, hipStreamSynchronize(sl.s));
        if (sl.comm) HIPM(m, hipStreamSynchronize(sl.comm));
        HIPM(m, hipStreamSynchronize(sl.copy));
        if (sl.expectValid && !sort_bounds_match(sl)) { // the last step's bounds check, now that its copy has landed
            sl.status = 1;
            return fail(m, SPH_ESTATE, "slab " + std::to_string(sl.rank) +
                                           ": a particle crossed more layers in z than this decomposition allows");
        }
    }
    return SPH_OK;
}

} // extern "C"
