// dev_mem.hpp — who owns device memory in the host code: DevBuf (a growable allocation freed by its scope), Staging (host arguments of a one-shot
// entry point on their way to the device and back) and dev_upload (allocate + copy for the raw pointer fields of the handles).
// The rule: a device allocation is freed by the destructor of the object that holds it - a local DevBuf / Staging or a handle - never by a
// list of frees at the end of a function.  Needs common.hpp only.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "common.hpp"

namespace qmx {
bool is_device_ptr(const void *p);   // api_core.hip

// growable device scratch
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int32_t reserve(size_t bytes) {
        if (bytes <= cap) return QMX_OK;
        release();
        size_t want = std::max<size_t>(bytes, 4096);
        QMX_HIP(hipMalloc(&p, want));
        cap = want;
        return QMX_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // hands the allocation to a raw pointer field of a handle
    void *detach() {
        cap = 0;
        return std::exchange(p, nullptr);
    }
};

// The possibly-host arguments of a synchronous entry point: host memory is staged through a device buffer this object owns, device memory is
// used where it lies; a null pointer or zero bytes stages nothing.  back() copies with blocking hipMemcpy calls: behind the work of the null stream,
// while work on another stream is synchronised by the caller first.
struct Staging {
    template <class T> int32_t in(const T *src, size_t bytes, const T **dev) {
        *dev = src;
        if (!src || !bytes || is_device_ptr(src)) return QMX_OK;
        void *d = nullptr;
        QMX_TRY(alloc(bytes, &d));
        QMX_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        *dev = (const T *)d;
        return QMX_OK;
    }
    template <class T> int32_t in(const T *src, size_t bytes, T **dev) { return in(src, bytes, (const T **)dev); }
    template <class T> int32_t out(T *dst, size_t bytes, T **dev) {
        *dev = dst;
        if (!dst || !bytes || is_device_ptr(dst)) return QMX_OK;
        void *d = nullptr;
        QMX_TRY(alloc(bytes, &d));
        outs.push_back({dst, d, bytes});
        *dev = (T *)d;
        return QMX_OK;
    }
    // an argument the device reads and rewrites in place
    template <class T> int32_t inout(T *buf, size_t bytes, T **dev) {
        QMX_TRY(out(buf, bytes, dev));
        if (*dev != buf) QMX_HIP(hipMemcpy(*dev, buf, bytes, hipMemcpyHostToDevice));
        return QMX_OK;
    }
    int32_t back() {
        for (const Out &o : outs) QMX_HIP(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
        outs.clear();
        return QMX_OK;
    }

private:
    struct Out { void *host; const void *dev; size_t bytes; };
    std::vector<DevBuf> bufs;
    std::vector<Out> outs;
    int32_t alloc(size_t bytes, void **d) {
        DevBuf b;
        QMX_TRY(b.reserve(bytes));
        *d = b.p;
        bufs.push_back(std::move(b));
        return QMX_OK;
    }
};

// allocate `count` elements (at least one) at *dst and copy them from host or device memory; *dst stays null when either step fails
template <class T> int32_t dev_upload(T **dst, const T *src, size_t count) {
    *dst = nullptr;
    void *p = nullptr;
    QMX_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    if (count) {
        const hipError_t e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyDefault);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return hip_status(e, "dev_upload: hipMemcpy", __FILE__, __LINE__);
        }
    }
    *dst = (T *)p;
    return QMX_OK;
}
// ... into a DevBuf: the temporaries of a build
template <class T> int32_t dev_upload(DevBuf &dst, const T *src, size_t count) {
    QMX_TRY(dst.reserve(std::max<size_t>(count, 1) * sizeof(T)));
    if (count) QMX_HIP(hipMemcpy(dst.p, src, count * sizeof(T), hipMemcpyDefault));
    return QMX_OK;
}
// a field the destructor of its handle frees
template <class T> void dev_free(T *&p) {
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}
}  // namespace qmx
