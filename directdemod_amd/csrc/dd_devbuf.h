// Owners of device (hipMalloc) and pinned host (hipHostMalloc) memory for the host layer.  Internal, header-only.
//
// DDDevBuf<T> / DDPinnedBuf<T>: move-only, count elements of T, free in the destructor.  A handle (dd_fir, dd_iir, ...) holds
// them as members, so its *_destroy is `delete` plus whatever is not memory; a per-call temporary is a local; a lazily built
// table is filled in a local owner and moved into its slot only once the upload has succeeded.
//
// Process-lifetime caches (scratch entries, FFT tables, the NCO table ...) live in holders that are created with `new` and
// never deleted: no static object has a destructor that calls into HIP, because the runtime may be gone by then.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

template <class T, bool Pinned>
class DDBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DDBuf() = default;
    DDBuf(const DDBuf&) = delete;
    DDBuf& operator=(const DDBuf&) = delete;
    DDBuf(DDBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DDBuf& operator=(DDBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DDBuf() { reset(); }

    // releases what it held, allocates count elements; empty on failure.  flags: hipHostMalloc's (pinned memory only)
    hipError_t alloc(size_t count, unsigned flags = 0) {
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, count * sizeof(T), flags) : hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = count; }
        return e;
    }
    // nothing when the capacity suffices, else alloc: the contents are not kept
    hipError_t grow(size_t count, unsigned flags = 0) { return count <= n_ ? hipSuccess : alloc(count, flags); }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T* release() { T* p = p_; p_ = nullptr; n_ = 0; return p; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
};

template <class T> using DDDevBuf = DDBuf<T, false>;
template <class T> using DDPinnedBuf = DDBuf<T, true>;
