// device_buffer.hip.h -- who owns a device or page-locked host buffer of the three host libraries.
//
// bazbuf::Buffer<T, Policy> is a move-only owner of `cap()` elements of T.  It converts to T*, so launch sites, pointer arithmetic
// and null checks read as with a bare pointer; its destructor releases.  regrow() is the one home of the rule "drain the stream
// before freeing a buffer that work in flight may still use; the first allocation waits for nothing".
//
// A Policy says where the memory comes from: `status` (its value-initialised value means success),
// `static status alloc(void** p, size_t bytes)` and `static void release(void* p)`.  Counted<Raw, Which> wraps one so that every
// allocation shows in the library's live counts (the baz_*_debug_live_buffers taps).
//
// No HIP include of its own: the HIP policies and DeviceGuard below exist where the HIP runtime has been included in front of this
// file; without it the header is plain C++ (tests/test_device_buffer.py runs it over malloc / free).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace bazbuf {

template <typename T, typename Policy>
class Buffer {
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements

public:
    using status = typename Policy::status;

    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buffer() { release(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }   // (for reinterpret_cast, which takes no conversion)
    size_t cap() const { return cap_; }

    void release()
    {
        if (p_) Policy::release(p_);
        p_ = nullptr, cap_ = 0;
    }

    // n elements, uninitialised; what the owner held is released first.  On failure the owner is empty.
    status allocate(size_t n)
    {
        release();
        void* p = nullptr;
        const status s = Policy::alloc(&p, n * sizeof(T));
        if (s != status{}) return s;
        p_ = static_cast<T*>(p); cap_ = n;
        return s;
    }

    // Work in flight may still use a buffer that exists: drain() (returns a status) runs in front of its release, and a failed
    // drain keeps the buffer.  Nothing in flight can reference a buffer that does not exist yet: then drain() is not called.
    template <typename Drain>
    status retire(Drain&& drain)
    {
        if (!p_) return status{};
        const status s = drain();
        if (s == status{}) release();
        return s;
    }

    // At least n elements (contents are not kept).  Nothing happens while n <= cap().
    template <typename Drain>
    status regrow(size_t n, Drain&& drain)
    {
        if (n <= cap_) return status{};
        const status s = retire(drain);
        return s != status{} ? s : allocate(n);
    }
};

// Buffers that grow together share one drain: Once runs it at the first buffer that exists and repeats its answer from then on
// (retire() every buffer with the same Once, then allocate() them).
template <typename Drain>
struct Once {
    Drain drain;
    bool done = false;
    decltype(drain()) answer{};
    explicit Once(Drain d) : drain(d) {}
    auto operator()()
    {
        if (!done) answer = drain();
        done = true;
        return answer;
    }
};

// live allocations of this library in the process (each library is one translation unit: one copy each)
struct LiveCounts {
    std::atomic<uint64_t> device{0}, pinned{0};
    void report(uint64_t out[2]) const { out[0] = device.load(); out[1] = pinned.load(); }
};
namespace { LiveCounts g_live; }

template <typename Raw, std::atomic<uint64_t> LiveCounts::*Which>
struct Counted {
    using status = typename Raw::status;
    static status alloc(void** p, size_t bytes)
    {
        const status s = Raw::alloc(p, bytes);
        if (s == status{}) ++(g_live.*Which);
        return s;
    }
    static void release(void* p) { Raw::release(p), --(g_live.*Which); }
};

#ifdef __HIP__
struct HipDevice {
    using status = hipError_t;
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct HipPinned {
    using status = hipError_t;
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <typename T> using PinnedBuffer = Buffer<T, Counted<HipPinned, &LiveCounts::pinned>>;

// The drain a context hands its owners: launches of earlier calls on its stream may still use a buffer that is about to be freed
// (hipFree happens to synchronise the device today; nothing relies on it).
template <typename Ctx>
auto drain(Ctx* c) { return [c] { return hipStreamSynchronize(c->stream); }; }

// selects the context's device for a scope
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};
#endif

}  // namespace bazbuf
