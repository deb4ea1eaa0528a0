// dev_mem.h -- every device and pinned allocation of libqmri.so goes through this file ("Who owns memory").
//   DevArr<T> / PinnedArr<T>   one array that may grow: call-scope scratch, and context members that are sized by the call (ensure)
//   DevPool                    the many arrays of one plan that live and die together; the plan keeps raw pointers (its device-view structs are
//                              passed to kernels by value and stay trivially copyable)
//   Event / Stream             owners of the two other call-scope resources
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#include "../../include/qmri.h"

struct qmri_ctx;
void qmri_set_error(qmri_ctx* ctx, const char* fmt, ...);
int qmri_stream_idle(qmri_ctx* ctx);            // waits for ctx->stream (ctx may be null: nothing to wait for); api_core.cpp
// live allocations, their bytes, allocations since process start: [0] device, [1] pinned.  One per process (api_core.cpp), read by qmri_debug_mem_stats.
struct MemCount { std::atomic<long long> live{0}, bytes{0}, total{0}; };
MemCount& qmri_mem_count(bool pinned);

namespace {
// the single allocation / free pair
inline hipError_t mem_alloc(bool pinned, void** p, size_t bytes) {
    *p = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    MemCount& c = qmri_mem_count(pinned);
    c.live.fetch_add(1, std::memory_order_relaxed); c.bytes.fetch_add((long long)bytes, std::memory_order_relaxed); c.total.fetch_add(1, std::memory_order_relaxed);
    return e;
}
inline void mem_free(bool pinned, void* p, size_t bytes) {
    if (!p) return;
    (void)(pinned ? hipHostFree(p) : hipFree(p));
    MemCount& c = qmri_mem_count(pinned);
    c.live.fetch_sub(1, std::memory_order_relaxed); c.bytes.fetch_sub((long long)bytes, std::memory_order_relaxed);
}
// allocates max(count, 1) elements of `esize` bytes into *p; on failure *p is null, the message is `what` or the library's own, QMRI_ERR_NOMEM
inline int mem_alloc_msg(qmri_ctx* ctx, bool pinned, void** p, size_t count, size_t esize, const char* what) {
    const hipError_t e = mem_alloc(pinned, p, std::max<size_t>(count, 1) * esize);
    if (e == hipSuccess) return QMRI_OK;
    if (what) qmri_set_error(ctx, "%s", what);
    else qmri_set_error(ctx, "%s of %zu bytes failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", count * esize, hipGetErrorString(e));
    return QMRI_ERR_NOMEM;
}
template <typename T> constexpr size_t mem_esize() { if constexpr (std::is_void_v<T>) return 1; else return sizeof(T); }   // void: cap counts bytes

// Move-only owner of p[cap].  ensure() never shrinks and does not keep the contents; a failed ensure() leaves the owner empty.
template <typename T, bool PINNED> struct MemArr {
    T* p = nullptr;
    size_t cap = 0;                                  // elements
    MemArr() = default;
    MemArr(MemArr&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    MemArr& operator=(MemArr&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~MemArr() { reset(); }
    void reset() { mem_free(PINNED, (void*)p, std::max<size_t>(cap, 1) * mem_esize<T>()); p = nullptr; cap = 0; }
    int ensure(qmri_ctx* ctx, size_t count, const char* what = nullptr) {
        if (p && cap >= count) return QMRI_OK;
        if (p) { const int st = qmri_stream_idle(ctx); if (st != QMRI_OK) return st; reset(); }      // (work in flight may still read the old array)
        const int st = mem_alloc_msg(ctx, PINNED, (void**)&p, count, mem_esize<T>(), what);
        if (st == QMRI_OK) cap = count;
        return st;
    }
    operator T*() const { return p; }
};
template <typename T> using DevArr = MemArr<T, false>;       // hipMalloc / hipFree
template <typename T> using PinnedArr = MemArr<T, true>;     // hipHostMalloc / hipHostFree
template <typename T> using DevBuf = DevArr<T>;              // (the name the call-scope scratch was written with)

// Device arrays of one plan: alloc() fills the plan's raw pointer and records it, reset() (or the destructor) frees everything recorded.
struct DevPool {
    struct Rec { void* p; size_t bytes; };
    std::vector<Rec> recs;
    DevPool() = default;
    DevPool(DevPool&& o) noexcept : recs(std::move(o.recs)) { o.recs.clear(); }
    DevPool& operator=(DevPool&& o) noexcept { if (this != &o) { reset(); recs = std::move(o.recs); o.recs.clear(); } return *this; }
    ~DevPool() { reset(); }
    template <typename T> int alloc(qmri_ctx* ctx, T** ptr, size_t count, const char* what = nullptr) {
        void* q = nullptr;
        const int st = mem_alloc_msg(ctx, false, &q, count, mem_esize<T>(), what);
        *ptr = (T*)q;
        if (st == QMRI_OK) recs.push_back({q, std::max<size_t>(count, 1) * mem_esize<T>()});
        return st;
    }
    // alloc(), then a blocking copy of the host array data[count] into it (count == 0: nothing to copy)
    template <typename T> int upload(qmri_ctx* ctx, T** ptr, const std::remove_const_t<T>* data, size_t count) {     // (T may be const: a plan's read-only view)
        const int st = alloc(ctx, ptr, count);
        if (st != QMRI_OK || count == 0) return st;
        const hipError_t e = hipMemcpy((void*)*ptr, data, count * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) return QMRI_OK;
        qmri_set_error(ctx, "hipMemcpy of %zu bytes to the device failed: %s (%s:%d)", count * sizeof(T), hipGetErrorString(e), __FILE__, __LINE__);
        return QMRI_ERR_HIP;
    }
    void free_one(const void* ptr) {                // a member that is replaced on its own
        for (size_t i = 0; ptr && i < recs.size(); ++i)
            if (recs[i].p == ptr) { mem_free(false, recs[i].p, recs[i].bytes); recs.erase(recs.begin() + (long)i); return; }
    }
    void reset() { for (const Rec& r : recs) mem_free(false, r.p, r.bytes); recs.clear(); }
};

struct Event {                                      // hipEventCreate* / hipEventDestroy
    hipEvent_t e = nullptr;
    Event() = default; Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct Stream {                                     // hipStreamCreate* / hipStreamDestroy
    hipStream_t s = nullptr;
    Stream() = default; Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
}  // namespace
