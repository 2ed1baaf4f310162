// csrc/sph_owned.h without a GPU and without the HIP runtime: the six functions the header calls are defined
// here, as counting fakes over malloc / free, and every scenario prints what it counted ("name value" lines) for
// tests/test_owned_cpu.py.  Built under ASan + UBSan: a block released twice, or never, is the sanitizer's report.
#include "sph_owned.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>

using sph_owned::DeviceBuf;
using sph_owned::Event;
using sph_owned::PinnedBuf;

namespace {

struct Kind {
    long made = 0, released = 0, unknown = 0; // unknown: a release of something this kind never handed out (or twice)
    std::set<void *> live;
    void *make(size_t bytes) {
        void *p = malloc(bytes ? bytes : 1);
        live.insert(p);
        ++made;
        return p;
    }
    void release(void *p) {
        if (!live.erase(p)) { ++unknown; return; }
        ++released;
        free(p);
    }
};
Kind g_dev, g_pin, g_evt;
bool g_failNext = false;   // the next allocation / creation of any kind fails
size_t g_lastBytes = 0;
unsigned g_lastFlags = 0;
std::string g_log;         // m / f: device, M / F: pinned, c / d: event, x: a refused call

bool refuse() {
    if (!g_failNext) return false;
    g_failNext = false;
    g_log += 'x';
    return true;
}

} // namespace

// (hipMalloc<T> and hipHostMalloc<T> of hip_runtime_api.h forward to these two)
extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    if (refuse()) return hipErrorOutOfMemory;
    *ptr = g_dev.make(size);
    g_lastBytes = size;
    g_log += 'm';
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr) {
    g_dev.release(ptr);
    g_log += 'f';
    return hipSuccess;
}
extern "C" hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int flags) {
    if (refuse()) return hipErrorOutOfMemory;
    *ptr = g_pin.make(size);
    g_lastBytes = size;
    g_lastFlags = flags;
    g_log += 'M';
    return hipSuccess;
}
extern "C" hipError_t hipHostFree(void *ptr) {
    g_pin.release(ptr);
    g_log += 'F';
    return hipSuccess;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags) {
    if (refuse()) return hipErrorOutOfMemory;
    *event = static_cast<hipEvent_t>(g_evt.make(1));
    g_lastFlags = flags;
    g_log += 'c';
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t event) {
    g_evt.release(event);
    g_log += 'd';
    return hipSuccess;
}

namespace {

void put(const std::string &name, long v) { printf("%s %ld\n", name.c_str(), v); }

// the calls a scenario made, and what is still held after it
void report(const char *tag) {
    printf("%s_log %s\n", tag, g_log.empty() ? "-" : g_log.c_str());
    put(std::string(tag) + "_live", (long)(g_dev.live.size() + g_pin.live.size() + g_evt.live.size()));
    g_log.clear();
}

struct StepEvents { Event e[6], c[2]; }; // the step ring's entry (sph_handle.h)

} // namespace

int main() {
    { // every allocation is released once at scope exit; alloc(count) asks for count elements
        DeviceBuf<double> d;
        PinnedBuf<float> p;
        Event e;
        put("scope_rc", d.alloc(10));
        put("scope_dev_bytes", (long)g_lastBytes);
        memset(d.get(), 0, 10 * sizeof(double));
        put("scope_rc", p.alloc(7, hipHostMallocMapped));
        put("scope_pin_bytes", (long)g_lastBytes);
        put("scope_pin_mapped", g_lastFlags == hipHostMallocMapped);
        put("scope_rc", p.alloc(7));
        put("scope_pin_default", g_lastFlags == hipHostMallocDefault);
        p[6] = 1.f;
        put("scope_rc", e.create(hipEventDisableTiming));
        put("scope_evt_flags", g_lastFlags == hipEventDisableTiming);
        double *raw = d; // the implicit conversions
        hipEvent_t rawE = e;
        put("scope_converts", raw == d.get() && rawE != nullptr && (d + 1) == raw + 1 && &d[2] == raw + 2);
    }
    report("scope"); // m M F M c, then (members in reverse) d F f

    { // alloc on a full object releases the old block first
        DeviceBuf<int> d;
        PinnedBuf<int> p;
        put("again_rc", d.alloc(4));
        put("again_rc", d.alloc(8));
        put("again_rc", p.alloc(4));
        put("again_rc", p.alloc(8));
    }
    report("again");

    { // a failed alloc leaves the object empty and releases nothing twice
        DeviceBuf<int> d;
        PinnedBuf<int> p;
        Event e;
        put("fail_rc_before", d.alloc(4) | p.alloc(4));
        g_failNext = true;
        put("fail_dev_refused", d.alloc(8) != hipSuccess);
        g_failNext = true;
        put("fail_pin_refused", p.alloc(8) != hipSuccess);
        g_failNext = true;
        put("fail_evt_refused", e.create() != hipSuccess);
        put("fail_empty", d.get() == nullptr && p.get() == nullptr && static_cast<hipEvent_t>(e) == nullptr);
        put("fail_rc_after", d.alloc(2)); // (and it can be used again)
    }
    report("fail");

    { // move construction and move assignment leave the source empty
        DeviceBuf<int> a, c;
        PinnedBuf<int> pa, pc;
        Event ea, ec;
        put("move_rc", a.alloc(4) | c.alloc(4) | pa.alloc(4) | pc.alloc(4) | ea.create() | ec.create());
        int *ra = a, *rpa = pa;
        hipEvent_t rea = ea;
        DeviceBuf<int> b(std::move(a));
        PinnedBuf<int> pb(std::move(pa));
        Event eb(std::move(ea));
        put("move_ctor_source_empty", a.get() == nullptr && pa.get() == nullptr && static_cast<hipEvent_t>(ea) == nullptr);
        put("move_ctor_target_holds", b.get() == ra && pb.get() == rpa && static_cast<hipEvent_t>(eb) == rea);
        g_log += '|';
        c = std::move(b); // releases c's own block, takes b's
        pc = std::move(pb);
        ec = std::move(eb);
        g_log += '|';
        put("move_assign_source_empty", b.get() == nullptr && pb.get() == nullptr && static_cast<hipEvent_t>(eb) == nullptr);
        put("move_assign_target_holds", c.get() == ra && pc.get() == rpa && static_cast<hipEvent_t>(ec) == rea);
        DeviceBuf<int> &self = c;
        c = std::move(self); // (self-assignment keeps the block)
        put("move_self_keeps", c.get() == ra);
    }
    report("move");

    { // reset() on an empty object calls nothing; reset() twice releases once
        DeviceBuf<int> d;
        PinnedBuf<int> p;
        Event e;
        d.reset();
        p.reset();
        e.reset();
        report("reset_empty");
        put("reset_rc", d.alloc(1) | p.alloc(1) | e.create());
        for (int k = 0; k < 2; ++k) d.reset(), p.reset(), e.reset();
        put("reset_leaves_empty", d.get() == nullptr && p.get() == nullptr && static_cast<hipEvent_t>(e) == nullptr);
    }
    report("reset");

    { // create twice creates once (create on first use)
        Event e;
        put("twice_rc", e.create(hipEventDisableTiming));
        hipEvent_t first = e;
        put("twice_rc", e.create(hipEventDisableTiming));
        put("twice_same", static_cast<hipEvent_t>(e) == first);
    }
    report("twice");

    { // the step ring's shape: 64 entries of 6 + 2 events
        const long before = g_evt.made;
        {
            StepEvents ring[64];
            long rc = 0;
            for (auto &se : ring) {
                for (auto &e : se.e) rc |= e.create();
                for (auto &e : se.c) rc |= e.create();
            }
            put("ring_rc", rc);
            put("ring_created", g_evt.made - before);
            put("ring_live_inside", (long)g_evt.live.size());
        }
        g_log.clear();
        report("ring");
    }

    put("total_dev_made", g_dev.made);
    put("total_dev_released", g_dev.released);
    put("total_pin_made", g_pin.made);
    put("total_pin_released", g_pin.released);
    put("total_evt_made", g_evt.made);
    put("total_evt_released", g_evt.released);
    put("total_unknown_releases", g_dev.unknown + g_pin.unknown + g_evt.unknown);
    return 0;
}
