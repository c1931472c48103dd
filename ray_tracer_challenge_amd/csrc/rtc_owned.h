// rtc_owned.h -- owners of what the host side of the device path holds through the HIP runtime: device arrays, the pinned staging
// buffer, events, a stream.  Host-only: included by rtc_device.hip alone, never by a kernel header, and not embedded for hiprtc.
//
// All four are non-copyable and movable, start empty, and release what they hold in their destructor.  ONE INVARIANT is the
// holder's, not theirs: a release (a destructor, release(), a grow() that has to reallocate, a map's clear()) happens with the
// device current on which the thing was made.  A context sets its device at the top of every entry point and before `delete`.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

#pragma GCC visibility push(hidden)  // (inline and host-only: nothing here is part of what the library exports)
namespace rtc {

// What the owners share: one handle, empty when null, freed by `Free`.
template <class H, hipError_t (*Free)(H)>
class Owned {
public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H())) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            release();
            h_ = std::exchange(o.h_, H());
        }
        return *this;
    }
    ~Owned() { release(); }
    void release() {
        if (h_) (void)Free(std::exchange(h_, H()));
    }
    H get() const { return h_; }
    operator H() const { return h_; }  // (to a HIP call or a kernel's argument block as the handle it is)

protected:
    H h_ = H();
};

// A grow-only device array of T, capacity() counting elements: hipMalloc and hipFree cost an animation's frames milliseconds, so a
// buffer is kept at the largest size it has had.
template <class T>
class DeviceArray {
public:
    // Room for at least `n` elements (nothing may be in flight that reads the old ones).  headroom: half as much again, for buffers
    // that grow by steps.  The array is empty while the allocation is attempted: a failed hipMalloc cannot leave a stale capacity
    // beside a freed pointer.
    hipError_t grow(size_t n, bool headroom = false) {
        if (p_.get() != nullptr && cap_ >= n) return hipSuccess;
        release();
        const size_t want = headroom ? std::max<size_t>(256 / sizeof(T), n + n / 2) : n;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) p_ = Block(p), cap_ = want;
        return e;
    }
    void release() { p_.release(), cap_ = 0; }
    T* get() const { return (T*)p_.get(); }
    operator T*() const { return get(); }
    size_t capacity() const { return cap_; }

private:
    typedef Owned<void*, hipFree> Block;
    Block p_;
    size_t cap_ = 0;  // (a moved-from array keeps a capacity beside a null pointer: grow() looks at the pointer first)
};

// Pinned host memory (grow-only, bytes): at least 64 KB, and half as much again as asked for.
class PinnedBuffer {
public:
    hipError_t grow(size_t bytes) {
        if (p_.get() != nullptr && cap_ >= bytes) return hipSuccess;
        p_.release(), cap_ = 0;
        const size_t want = std::max<size_t>(1u << 16, bytes + bytes / 2);
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) p_ = Block(p), cap_ = want;
        return e;
    }
    void* get() const { return p_.get(); }

private:
    typedef Owned<void*, hipHostFree> Block;
    Block p_;
    size_t cap_ = 0;
};

// An event, created by the first create() and kept; a stream likewise.
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, flags); }
};

}  // namespace rtc
#pragma GCC visibility pop
