// Owners of the three kinds of GPU resource the host code holds: device memory, pinned host memory, an event.
// Move-only; the destructor releases; each converts to the raw pointer / hipEvent_t it owns, so call sites
// read as they would with one.  Host only, header only: libsph_hip.so and libsph_mgpu.so both include it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <utility>

namespace sph_owned {

template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    // releases what it holds, then allocates `count` elements; on failure the object is left empty
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipFree(std::exchange(p_, nullptr)); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }

private:
    T *p_ = nullptr;
};

template <class T>
class PinnedBuf { // the same over hipHostMalloc / hipHostFree; flags: hipHostMallocMapped for the two mapped blocks
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T), flags);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(std::exchange(p_, nullptr)); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }

private:
    T *p_ = nullptr;
};

class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept {
        if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    // a no-op when already created (create on first use)
    hipError_t create(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void reset() { if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr)); }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

} // namespace sph_owned
