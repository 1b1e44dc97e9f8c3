// lm_own.h -- the four owners of HIP resources: DevBuf<T> (hipMalloc), PinnedBuf<T> (hipHostMalloc), Stream, Event.  Each is empty when
// default-constructed, move-only, and releases what it holds in its destructor; creation is explicit and returns hipError_t, so it sits
// inside HIP_TRY.  Creating into an owner that holds something releases that first: a function that fills a dozen owners and returns at the
// first failure may simply be called again.  Nothing outside this header calls a HIP create / free function.
// g_live counts the live resources of the process per kind -- raised in adopt(), lowered in reset(), nowhere else (lm_debug_live_resources).
// Depends on the HIP runtime header and the standard library only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <vector>

namespace lmd {

enum OwnKind { OWN_DEV = 0, OWN_PINNED = 1, OWN_STREAM = 2, OWN_EVENT = 3 };
inline std::atomic<long long> g_live[4];

template <typename H, OwnKind K>
class Owned {
public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}      // takes over a handle that release() gave out (lm_device_free, lm_host_free): it is counted already
    Owned(Owned&& o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = nullptr; o.n_ = 0; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; n_ = o.n_; o.h_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Owned() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    size_t size() const { return n_; }      // elements of a buffer (0: empty, or a stream / an event)
    H release() { H h = h_; h_ = nullptr; n_ = 0; return h; }      // hands the handle out, still live and still counted
    void reset() {
        if (!h_) return;
        if constexpr (K == OWN_DEV) (void)hipFree(h_);
        else if constexpr (K == OWN_PINNED) (void)hipHostFree(h_);
        else if constexpr (K == OWN_STREAM) (void)hipStreamDestroy(h_);
        else (void)hipEventDestroy(h_);
        g_live[K].fetch_sub(1, std::memory_order_relaxed);
        h_ = nullptr; n_ = 0;
    }
protected:
    hipError_t adopt(hipError_t e, H h, size_t n) {      // (the caller has the create call's result in hand: no argument of this call may BE the call)
        if (e == hipSuccess) { h_ = h; n_ = n; g_live[K].fetch_add(1, std::memory_order_relaxed); }
        return e;
    }
    H h_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
struct DevBuf : Owned<T*, OWN_DEV> {
    using Owned<T*, OWN_DEV>::Owned;
    hipError_t alloc(size_t n) { this->reset(); void* p = nullptr; const hipError_t e = hipMalloc(&p, n * sizeof(T)); return this->adopt(e, static_cast<T*>(p), n); }
    // room for n elements: as it is when large enough, otherwise released FIRST and then allocated (the peak stays low; the contents are
    // not kept, and the caller has made sure that nothing in flight reads them).  A failure leaves the buffer empty.
    hipError_t grow(size_t n) { return n <= this->n_ ? hipSuccess : alloc(n); }
};

template <typename T>
struct PinnedBuf : Owned<T*, OWN_PINNED> {
    using Owned<T*, OWN_PINNED>::Owned;
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        this->reset(); void* p = nullptr; const hipError_t e = hipHostMalloc(&p, n * sizeof(T), flags); return this->adopt(e, static_cast<T*>(p), n);
    }
    hipError_t grow(size_t n) { return n <= this->n_ ? hipSuccess : alloc(n); }
};

struct Stream : Owned<hipStream_t, OWN_STREAM> {
    using Owned::Owned;
    hipError_t create(unsigned flags) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithFlags(&s, flags); return adopt(e, s, 0); }
    hipError_t create(unsigned flags, int priority) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithPriority(&s, flags, priority); return adopt(e, s, 0); }
};

struct Event : Owned<hipEvent_t, OWN_EVENT> {
    using Owned::Owned;
    hipError_t create(unsigned flags = hipEventDefault) { reset(); hipEvent_t ev = nullptr; const hipError_t e = hipEventCreateWithFlags(&ev, flags); return adopt(e, ev, 0); }
};

// a device copy of v (at least one element is allocated: an empty list still has an address)
template <typename T>
hipError_t upload_vec(DevBuf<T>& b, const std::vector<T>& v) {
    hipError_t e = b.alloc(std::max<size_t>(v.size(), 1));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

}  // namespace lmd
