// The multi-GPU driver's transports: how one round of messages gets from slab to slab, and the
// set-up and tear-down of the RCCL communicators.
#include "mgpu_driver.h"

#include <algorithm>
#include <deque>
#include <map>

using namespace mgpu_host;

namespace {

// SPH_TRANSPORT_MAILBOX (tests): several one-slab driver objects inside ONE process stand for
// the ranks of a one-process-per-GPU run; a send is a note in this table, the receive copies
// from it once the sending object has posted (the test steps every object phase by phase).
struct Mail { const void *src; size_t bytes; };
std::map<std::pair<int, int>, std::deque<Mail>> g_mail;
// receives of ALL objects waiting for the next phase: they are completed together, by
// whichever object enters the next phase first -- like RCCL, where a send has left the
// sender's buffer before any later kernel of the sender runs
struct PendingRecv { int src_rank, dst_rank; void *dst; size_t bytes; hipStream_t stream; long long epoch; };
std::vector<PendingRecv> g_pending;

int deliver_mailbox(sph_mgpu *m, const std::vector<Msg> &msgs) {
    for (const Msg &g : msgs) {
        if (local(m, g.src_rank)) g_mail[{g.src_rank, g.dst_rank}].push_back({g.src, g.bytes});
        if (local(m, g.dst_rank))
            g_pending.push_back({g.src_rank, g.dst_rank, g.dst, g.bytes, m->shared, m->step * 4 + m->phase});
    }
    return SPH_OK;
}

int deliver_streams(sph_mgpu *m, const std::vector<Msg> &msgs, bool on_comm_stream) {
    // what a grouped ncclSend/ncclRecv round does to the participating streams, with copies:
    // a receive starts once the sender's stream has reached the round, and no stream of the
    // round goes on before the messages it sends and receives are through
    const int q = on_comm_stream ? 1 : 0;
    auto stream_of = [&](Slab *sl) { return on_comm_stream ? sl->comm : sl->s; };
    std::vector<Slab *> part;
    for (const Msg &g : msgs)
        for (int r : {g.src_rank, g.dst_rank}) {
            Slab *sl = local(m, r);
            if (std::find(part.begin(), part.end(), sl) == part.end()) part.push_back(sl);
        }
    for (Slab *sl : part) HIPM(m, hipEventRecord(sl->evTx[q], stream_of(sl)));
    for (const Msg &g : msgs) {
        Slab *a = local(m, g.src_rank), *b = local(m, g.dst_rank);
        HIPM(m, hipStreamWaitEvent(stream_of(b), a->evTx[q], 0));
        HIPM(m, hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyDeviceToDevice, stream_of(b)));
    }
    for (Slab *sl : part) HIPM(m, hipEventRecord(sl->evRx[q], stream_of(sl)));
    for (const Msg &g : msgs) {
        Slab *a = local(m, g.src_rank), *b = local(m, g.dst_rank);
        HIPM(m, hipStreamWaitEvent(stream_of(a), b->evRx[q], 0)); // the sender's buffer is free again
    }
    return SPH_OK;
}

int deliver_loopback(sph_mgpu *m, const std::vector<Msg> &msgs) {
    for (const Msg &g : msgs) HIPM(m, hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyDeviceToDevice, m->shared));
    return SPH_OK;
}

int deliver_rccl(sph_mgpu *m, const std::vector<Msg> &msgs, bool on_comm_stream) {
    NCCLM(m, ncclGroupStart());
    if (m->opt.transport == SPH_TRANSPORT_RCCL_SELF) {
        // one rank, every message goes to itself: sends and receives match in posting order
        Slab &s0 = m->slabs[0];
        for (const Msg &g : msgs)
            NCCLM(m, ncclSend(g.src, g.bytes, ncclChar, 0, s0.comm_nccl, m->shared));
        for (const Msg &g : msgs)
            NCCLM(m, ncclRecv(g.dst, g.bytes, ncclChar, 0, s0.comm_nccl, m->shared));
    } else {
        for (const Msg &g : msgs) {
            if (Slab *a = local(m, g.src_rank)) {
                HIPM(m, hipSetDevice(a->device));
                NCCLM(m, ncclSend(g.src, g.bytes, ncclChar, g.dst_rank, a->comm_nccl, on_comm_stream ? a->comm : a->s));
            }
            if (Slab *b = local(m, g.dst_rank)) {
                HIPM(m, hipSetDevice(b->device));
                NCCLM(m, ncclRecv(g.dst, g.bytes, ncclChar, g.src_rank, b->comm_nccl, on_comm_stream ? b->comm : b->s));
            }
        }
    }
    NCCLM(m, ncclGroupEnd());
    return SPH_OK;
}

} // namespace

int mgpu_host::deliver(sph_mgpu *m, const std::vector<Msg> &msgs, bool on_comm_stream) {
    if (msgs.empty()) return SPH_OK;
    const int tr = m->opt.transport;
    std::vector<Msg> live; // the transports see no empty message
    for (const Msg &g : msgs) {
        if ((tr == SPH_TRANSPORT_STREAMS || tr == SPH_TRANSPORT_LOOPBACK) && (!g.src || !g.dst))
            return fail(m, SPH_ESTATE, std::string(tr == SPH_TRANSPORT_STREAMS ? "streams" : "loopback") +
                                           " transport needs every slab in this process");
        if (g.bytes) live.push_back(g);
    }
    if (tr == SPH_TRANSPORT_MAILBOX) return deliver_mailbox(m, live);
    if (tr == SPH_TRANSPORT_STREAMS) return deliver_streams(m, live, on_comm_stream);
    if (tr == SPH_TRANSPORT_LOOPBACK) return deliver_loopback(m, live);
    return deliver_rccl(m, live, on_comm_stream);
}

int mgpu_host::resolve_mail(sph_mgpu *m) {
    if (m->opt.transport != SPH_TRANSPORT_MAILBOX || g_pending.empty()) return SPH_OK;
    HIPM(m, hipDeviceSynchronize()); // the senders' data is complete (all objects share the device)
    const long long now = m->step * 4 + m->phase; // receives posted in EARLIER phases only
    std::vector<PendingRecv> later;
    for (const auto &r : g_pending) {
        if (r.epoch >= now) {
            later.push_back(r);
            continue;
        }
        auto &q = g_mail[{r.src_rank, r.dst_rank}];
        if (q.empty()) return fail(m, SPH_ESTATE, "mailbox: the sending rank has not run this phase yet");
        const Mail mm = q.front();
        q.pop_front();
        if (mm.bytes != r.bytes) return fail(m, SPH_ESTATE, "mailbox: sender and receiver disagree on a message size");
        HIPM(m, hipMemcpyAsync(r.dst, mm.src, r.bytes, hipMemcpyDeviceToDevice, r.stream));
    }
    g_pending.swap(later);
    HIPM(m, hipDeviceSynchronize());
    return SPH_OK;
}

int mgpu_host::init_comms(sph_mgpu *m, const void *unique_id128) {
    const SphMgpuOptions &o = m->opt;
    if (o.transport == SPH_TRANSPORT_RCCL_SELF) {
        int dev = m->slabs[0].device;
        ncclComm_t c = nullptr;
        if (ncclCommInitAll(&c, 1, &dev) != ncclSuccess) return fail(nullptr, SPH_EHIP, "ncclCommInitAll failed");
        for (auto &sl : m->slabs) sl.comm_nccl = c;
    } else if (o.transport == SPH_TRANSPORT_RCCL && o.rank_count == o.world) {
        std::vector<ncclComm_t> comms(o.world);
        std::vector<int> devs(o.world);
        for (int k = 0; k < o.world; ++k) devs[k] = m->slabs[k].device;
        if (ncclCommInitAll(comms.data(), o.world, devs.data()) != ncclSuccess) return fail(nullptr, SPH_EHIP, "ncclCommInitAll failed");
        for (int k = 0; k < o.world; ++k) m->slabs[k].comm_nccl = comms[k];
    } else if (o.transport == SPH_TRANSPORT_RCCL) {
        ncclUniqueId id;
        memcpy(&id, unique_id128, sizeof id);
        if (hipSetDevice(m->slabs[0].device) != hipSuccess ||
            ncclCommInitRank(&m->slabs[0].comm_nccl, o.world, id, o.rank_begin) != ncclSuccess)
            return fail(nullptr, SPH_EHIP, "ncclCommInitRank failed");
    }
    return SPH_OK;
}

void mgpu_host::destroy_comms(sph_mgpu *m) {
    ncclComm_t last = nullptr;
    for (auto &sl : m->slabs) {
        if (sl.comm_nccl && sl.comm_nccl != last) {
            last = sl.comm_nccl;
            (void)ncclCommDestroy(sl.comm_nccl);
        }
        sl.comm_nccl = nullptr;
    }
}
