// Read-back of a timed step's positions through an SDMA engine (see sph_handle::sdmaOk).  The only unit that
// talks to the HSA runtime.
#include "sph_handle.h"

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

// (the handle keeps the HSA objects as their 64-bit handles: no HSA header outside this unit)
hsa_signal_t sig(const sph_handle *h, int slot) { return hsa_signal_t{h->rbSig[slot]}; }

struct AgentSearch { int wantBdf; hsa_agent_t gpu, cpu; bool haveGpu, haveCpu; };
hsa_status_t find_agents(hsa_agent_t a, void *data) {
    AgentSearch *S = static_cast<AgentSearch *>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && !S->haveCpu) { S->cpu = a; S->haveCpu = true; }
    if (t == HSA_DEVICE_TYPE_GPU && !S->haveGpu) {
        uint32_t bdf = 0;
        if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS &&
            (S->wantBdf < 0 || (int)(bdf & 0xffff) == S->wantBdf)) { S->gpu = a; S->haveGpu = true; }
    }
    return HSA_STATUS_SUCCESS;
}

} // namespace

namespace sph_host {

void sdma_init(sph_handle *h) {
    if (!h->knobs.readbackSdma) return;
    if (h->external || h->mappedPos || !h->hostPos || !h->devPos[0]) return;
    if (hsa_init() != HSA_STATUS_SUCCESS) return;
    AgentSearch S{};
    S.wantBdf = -1;
    int bus = 0, dev = 0;
    if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, h->device) == hipSuccess &&
        hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, h->device) == hipSuccess)
        S.wantBdf = ((bus & 0xff) << 8) | ((dev & 0x1f) << 3);
    (void)hsa_iterate_agents(find_agents, &S);
    if (!S.haveGpu && S.wantBdf >= 0) { // no BDF match (virtualised ids): with ONE visible GPU there is no choice to make
        int count = 0;
        if (hipGetDeviceCount(&count) == hipSuccess && count == 1) {
            S.wantBdf = -1;
            (void)hsa_iterate_agents(find_agents, &S);
        }
    }
    uint64_t hz = 0;
    hsa_signal_t sg[2]{};
    if (!S.haveGpu || !S.haveCpu || hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &hz) != HSA_STATUS_SUCCESS || !hz ||
        hsa_signal_create(0, 0, nullptr, &sg[0]) != HSA_STATUS_SUCCESS ||
        hsa_signal_create(0, 0, nullptr, &sg[1]) != HSA_STATUS_SUCCESS) {
        (void)hsa_shut_down();
        return;
    }
    h->rbSig[0] = sg[0].handle;
    h->rbSig[1] = sg[1].handle;
    (void)hsa_amd_profiling_async_copy_enable(true);
    h->hsaGpu = S.gpu.handle;
    h->hsaCpu = S.cpu.handle;
    h->hsaTickSeconds = 1.0 / (double)hz;
    // The engines are not alike: on an MI355X four of them move 56 GB/s to the host and the rest 12.8
    // (scripts/microbench/sdma_d2h.cpp), and left to itself the HSA runtime sometimes hands out a slow one.
    // Time a few megabytes through every free engine once and keep the fastest.
    const size_t probe = std::min<size_t>((size_t)h->n * 3 * sizeof(float), (size_t)4 << 20);
    auto time_engine = [&](uint32_t engine) -> double { // seconds, or < 0
        double best = -1;
        for (int rep = 0; rep < 2; ++rep) {
            hsa_signal_store_relaxed(sg[0], 1);
            const hsa_status_t st = engine
                ? hsa_amd_memory_async_copy_on_engine(h->hostPos, S.cpu, h->devPos[0], S.gpu, probe, 0, nullptr, sg[0],
                                                      (hsa_amd_sdma_engine_id_t)engine, false)
                : hsa_amd_memory_async_copy(h->hostPos, S.cpu, h->devPos[0], S.gpu, probe, 0, nullptr, sg[0]);
            if (st != HSA_STATUS_SUCCESS) return -1;
            int tries = 0;
            while (hsa_signal_wait_scacquire(sg[0], HSA_SIGNAL_CONDITION_LT, 1, hz / 2, HSA_WAIT_STATE_BLOCKED) >= 1)
                if (++tries > 20) return -1;
            hsa_amd_profiling_async_copy_time_t t{};
            if (hsa_amd_profiling_get_async_copy_time(sg[0], &t) != HSA_STATUS_SUCCESS || t.end <= t.start) return -1;
            const double sec = (double)(t.end - t.start) * h->hsaTickSeconds;
            if (best < 0 || sec < best) best = sec;
        }
        return best;
    };
    if (probe >= ((size_t)1 << 16)) {
        double bestSec = time_engine(0);
        uint32_t mask = 0;
        if (hsa_amd_memory_copy_engine_status(S.cpu, S.gpu, &mask) == HSA_STATUS_SUCCESS)
            for (uint32_t bit = 1; bit && bit <= mask; bit <<= 1) {
                if (!(mask & bit)) continue;
                const double sec = time_engine(bit);
                if (sec > 0 && (bestSec < 0 || sec < 0.9 * bestSec)) { bestSec = sec; h->sdmaEngine = bit; }
            }
        if (bestSec < 0) { // no engine moved the probe: leave the read-back to the HIP runtime
            (void)hsa_signal_destroy(sg[0]);
            (void)hsa_signal_destroy(sg[1]);
            h->hsaTickSeconds = 0;
            (void)hsa_shut_down();
            return;
        }
        memset(h->hostPos, 0, probe);
    }
    h->sdmaOk = true;
    if (h->knobs.stepTrace) fprintf(stderr, "sph: read-back through SDMA engine id 0x%x (0 = the HSA runtime's choice)\n", h->sdmaEngine);
}

// wait for the SDMA copy out of devPos[slot] (if one is in flight); its duration goes to kt.readback
int sdma_wait(sph_handle *h, int slot) {
    if (!h->rbPending[slot]) return SPH_OK;
    for (int tries = 0;; ++tries) { // 60 x 0.5 s: a copy that never completes is an error, not a hang
        if (hsa_signal_wait_scacquire(sig(h, slot), HSA_SIGNAL_CONDITION_LT, 1, (uint64_t)(0.5 / h->hsaTickSeconds),
                                      HSA_WAIT_STATE_BLOCKED) < 1) break;
        if (tries >= 60) return fail(h, SPH_EHIP, "read-back copy did not complete");
    }
    hsa_amd_profiling_async_copy_time_t t{};
    if (hsa_amd_profiling_get_async_copy_time(sig(h, slot), &t) == HSA_STATUS_SUCCESS && t.end >= t.start)
        h->kt.readback += (double)(t.end - t.start) * h->hsaTickSeconds;
    h->rbPending[slot] = false;
    return SPH_OK;
}

// the host has seen the force sweep that filled devPos[slot] finish: copy it out
int sdma_issue(sph_handle *h, int slot) {
    for (int b = 0; b < 2; ++b) // (a HIP copy of an untimed step still writing the same host buffer)
        if (h->copyPending[b]) {
            HIPCHK(h, hipEventSynchronize(h->copyDone[b]));
            h->copyPending[b] = false;
        }
    int rc = sdma_wait(h, slot);
    if (rc) return rc;
    hsa_signal_t dep = sig(h, slot ^ 1);
    const hsa_agent_t gpu{h->hsaGpu}, cpu{h->hsaCpu};
    const bool haveDep = h->rbPending[slot ^ 1]; // copies land in one host buffer: one after the other
    hsa_signal_store_relaxed(sig(h, slot), 1);
    const size_t bytes = (size_t)h->n * 3 * sizeof(float);
    hsa_status_t st = HSA_STATUS_ERROR;
    if (h->sdmaEngine)
        st = hsa_amd_memory_async_copy_on_engine(h->hostPos, cpu, h->devPos[slot], gpu, bytes, haveDep ? 1 : 0,
                                                 haveDep ? &dep : nullptr, sig(h, slot), (hsa_amd_sdma_engine_id_t)h->sdmaEngine, false);
    if (st != HSA_STATUS_SUCCESS) // (no engine picked, or it is busy: the HSA runtime's own choice)
        st = hsa_amd_memory_async_copy(h->hostPos, cpu, h->devPos[slot], gpu, bytes, haveDep ? 1 : 0,
                                       haveDep ? &dep : nullptr, sig(h, slot));
    if (st != HSA_STATUS_SUCCESS) {
        h->sdmaOk = false; // fall back to the runtime's copy, now and from here on
        rc = sdma_wait(h, slot ^ 1);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(h->hostPos, h->devPos[slot], (size_t)h->n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->copy));
        HIPCHK(h, hipEventRecord(h->copyDone[slot], h->copy));
        h->copyPending[slot] = true;
        return SPH_OK;
    }
    h->rbPending[slot] = true;
    return SPH_OK;
}

// (sph_destroy: the signals exist once sdma_init got as far as creating them)
void sdma_destroy(sph_handle *h) {
    if (h->hsaTickSeconds <= 0) return;
    (void)sdma_wait(h, 0);
    (void)sdma_wait(h, 1);
    (void)hsa_signal_destroy(sig(h, 0));
    (void)hsa_signal_destroy(sig(h, 1));
    (void)hsa_shut_down();
}

} // namespace sph_host
