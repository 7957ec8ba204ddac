// hip_owned.h -- move-only owners of HIP resources (host code): device and pinned host buffers, streams and events.
// Creating one returns the HIP status; the destructor frees what it holds.  A failed creation leaves the owner empty.
#pragma once
#include <cstddef>
#include <utility>

#include <hip/hip_runtime_api.h>

namespace hpfw {

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void *p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void *p) { return hipHostFree(p); }
};

// a buffer of `capacity()` bytes
template <class Mem>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buffer &operator=(Buffer &&o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~Buffer() { reset(); }

    // exactly `bytes`, in place of what was held
    hipError_t alloc(size_t bytes)
    {
        if (p_) {
            const hipError_t e = Mem::release(p_);
            p_ = nullptr;
            cap_ = 0;
            if (e != hipSuccess) return e;
        }
        const hipError_t e = Mem::alloc(&p_, bytes);
        if (e == hipSuccess) cap_ = bytes;
        else p_ = nullptr;
        return e;
    }
    // at least `bytes`; a buffer that grows loses its contents
    hipError_t ensure(size_t bytes) { return cap_ >= bytes ? hipSuccess : alloc(bytes); }
    void reset()
    {
        if (p_) (void)Mem::release(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    void *get() const { return p_; }
    template <class T>
    T *as() const { return static_cast<T *>(p_); }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

using DevBuf = Buffer<DeviceMem>;
using HostBuf = Buffer<PinnedMem>;

// a stream or an event: H the HIP handle type, Destroy its destroy call
template <class H, hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept
    {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Handle() { reset(); }
    void reset()
    {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

protected:
    // fills the handle through `create` (a HIP create call on &h_), in place of what was held
    template <class F>
    hipError_t make(F &&create)
    {
        reset();
        const hipError_t e = create(&h_);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }

private:
    H h_ = nullptr;
};

class Stream : public Handle<hipStream_t, hipStreamDestroy> {
public:
    // every stream the library creates is non-blocking: it does not wait for the null stream
    hipError_t create()
    {
        return make([](hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); });
    }
};

class Event : public Handle<hipEvent_t, hipEventDestroy> {
public:
    hipError_t create(unsigned flags = hipEventDisableTiming)
    {
        return make([flags](hipEvent_t *e) { return hipEventCreateWithFlags(e, flags); });
    }
};

} // namespace hpfw
