// A block of device or pinned host memory that owns itself: capacity in BYTES, move-only, frees itself.  A move assignment
// frees what the target held; release() frees now and reports.  Blocks grow through one function per rule, each taking the
// block: dev_exact, dev_at_least (below), dev_reserve, ensure_scratch (ctx.h), Grow (plan_gpu.hip), dev_grow
// (plan_fast.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace msim {

template <hipError_t (*Free)(void *)> struct Block {
    void *raw = nullptr; size_t cap = 0;
    Block() = default;
    Block(Block &&o) noexcept : raw(o.raw), cap(o.cap) { o.raw = nullptr; o.cap = 0; }
    Block &operator=(Block &&o) noexcept {
        if (this != &o) { (void)release(); raw = o.raw; cap = o.cap; o.raw = nullptr; o.cap = 0; }
        return *this;
    }
    ~Block() { (void)release(); }
    hipError_t release() {
        void *p = raw;
        raw = nullptr; cap = 0;
        return p ? Free(p) : hipSuccess;
    }
    explicit operator bool() const { return raw != nullptr; }
};
inline hipError_t dev_free(void *p) { return hipFree(p); }
inline hipError_t pin_free(void *p) { return hipHostFree(p); }
using DevBlock = Block<dev_free>;
using HostPinBlock = Block<pin_free>;                      // hipHostMalloc'ed (the small result and table blocks)
template <class T> struct Scratch : DevBlock { T *p() const { return static_cast<T *>(raw); } };
template <class T> struct Pinned : HostPinBlock { T *p() const { return static_cast<T *>(raw); } };

// exactly `bytes` into an EMPTY block (the allocate-once and exact-size buffers; the growth rules do their own arithmetic)
inline hipError_t dev_alloc(DevBlock &b, size_t bytes) {
    const hipError_t e = hipMalloc(&b.raw, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}
// exactly `bytes`, whatever the block held (contents are not kept)
inline hipError_t dev_exact(DevBlock &b, size_t bytes) {
    const hipError_t e = b.release();
    return e != hipSuccess || !bytes ? e : dev_alloc(b, bytes);
}
// at least `bytes`, allocated at exactly that size (contents are not kept; dev_reserve, ctx.h, adds slack to what it allocates)
inline hipError_t dev_at_least(DevBlock &b, size_t bytes) { return bytes <= b.cap ? hipSuccess : dev_exact(b, bytes); }
inline hipError_t pin_alloc(HostPinBlock &b, size_t bytes, unsigned flags = hipHostMallocDefault) {
    const hipError_t e = hipHostMalloc(&b.raw, bytes, flags);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}

}  // namespace msim
