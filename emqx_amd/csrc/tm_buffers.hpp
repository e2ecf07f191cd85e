// The owning types of everything the host code gets from the HIP runtime by
// hand: a device block, a pinned host block, the two as a mirrored pair, an
// event.  Each is move-only,
// grows only, and gives its block back in reset() and in its destructor (the
// runtime's return code ignored there: nothing can be done about it).  A
// failed runtime call leaves its text in etm::error_buf() and returns TM_EIO.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>

#include "../../include/emqx_tm.h"
#include "tm_internal.hpp"

#define BUF_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            snprintf(etm::error_buf(), 512, "%s at %s:%d (%s)", hipGetErrorString(_e), __FILE_NAME__, __LINE__, \
                     #expr);                                                                  \
            return TM_EIO;                                                                    \
        }                                                                                     \
    } while (0)

// Device block of at least MIN elements.  dev >= 0: the block lives on that
// device, which is made current before every allocation and free, and the old
// block is freed before the new one is allocated (the sharded group's
// buffers); dev < 0: the current device, new block first.
template <class T, size_t MIN = 1024>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    int dev = -1;

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), dev(o.dev) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0), dev = o.dev;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // exactly n elements, into an empty buffer
    int alloc(size_t n) {
        if (dev >= 0) BUF_HIP(hipSetDevice(dev));
        BUF_HIP(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return TM_OK;
    }
    int reserve(size_t n, bool keep = false, size_t keep_n = 0) {
        if (n <= cap && p) return TM_OK;
        if (dev >= 0 && !keep) reset();
        DevBuf nb;
        nb.dev = dev;
        if (int rc = nb.alloc(std::max<size_t>(n + n / 4, MIN))) return rc;
        if (keep && p && keep_n) BUF_HIP(hipMemcpy(nb.p, p, keep_n * sizeof(T), hipMemcpyDeviceToDevice));
        *this = std::move(nb);
        return TM_OK;
    }
    void reset() {
        if (p) {
            if (dev >= 0) (void)hipSetDevice(dev);
            (void)hipFree((void*)p);
        }
        p = nullptr;
        cap = 0;
    }
};

// Pinned host block of at least MIN elements, allocated with FLAGS; the old
// block is freed before the new one is allocated.
template <class T, unsigned FLAGS = hipHostMallocDefault, size_t MIN = 1024>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;

    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~PinBuf() { reset(); }

    // exactly n elements, into an empty buffer
    int alloc(size_t n) {
        BUF_HIP(hipHostMalloc((void**)&p, n * sizeof(T), FLAGS));
        cap = n;
        return TM_OK;
    }
    int reserve(size_t n) {
        if (n <= cap && p) return TM_OK;
        reset();
        return alloc(std::max<size_t>(n + n / 4, MIN));
    }
    void reset() {
        if (p) (void)hipHostFree((void*)p);
        p = nullptr;
        cap = 0;
    }
};
// pinned memory of the sharded group: usable from every device's context
template <class T>
using PortableBuf = PinBuf<T, hipHostMallocPortable>;
// pinned bytes the device writes directly (tm_export_host): coherent, so a
// kernel's stores are visible to the host once its completion is
using CoherentBuf = PinBuf<uint8_t, hipHostMallocCoherent | hipHostMallocMapped, 4096>;

// A device block and its pinned mirror: an array that crosses the bus, as a
// result read back (fetch) or an input sent up (stage).  The two sides, the
// copy's length and the pointer a caller is handed are kept in agreement here.
// The copies are enqueued on the caller's stream and never waited for.
template <class T>
struct Mirror {
    DevBuf<T> d;
    PinBuf<T> h;

    // the device side only, never empty: a length of 0 still yields a block
    int reserve(size_t n) { return d.reserve(std::max<size_t>(n, 1)); }
    // the pinned side sized for n elements (never empty either) and the
    // device's first n copied into it; a call that never fetches pins nothing
    int fetch(size_t n, hipStream_t s) {
        if (int rc = h.reserve(std::max<size_t>(n, 1))) return rc;
        if (n) BUF_HIP(hipMemcpyAsync(h.p, d.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
        return TM_OK;
    }
    // both sides sized for n elements, src[0..n) copied to the device through
    // the pinned side
    int stage(const T* src, size_t n, hipStream_t s) {
        if (int rc = reserve(n)) return rc;
        if (int rc = h.reserve(std::max<size_t>(n, 1))) return rc;
        if (n) {
            memcpy(h.p, src, n * sizeof(T));
            BUF_HIP(hipMemcpyAsync(d.p, h.p, n * sizeof(T), hipMemcpyHostToDevice, s));
        }
        return TM_OK;
    }
    const T* view(bool device) const { return device ? d.p : h.p; }
};

// An event, created by the first create() with that call's flags.
struct Event {
    hipEvent_t e = nullptr;

    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e = std::exchange(o.e, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }

    int create(unsigned flags = hipEventDefault) {
        if (!e) BUF_HIP(hipEventCreateWithFlags(&e, flags));
        return TM_OK;
    }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};
