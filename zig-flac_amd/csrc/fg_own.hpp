// fg_own.hpp -- the owners of HIP resources: a device buffer, a stream, an event.  Each is
// move-only and releases what it holds in its destructor, so a struct of owners needs no teardown
// code and its member order is its teardown order (members are destroyed last to first).  Carve and
// fit place several arrays in one owned buffer.  Host code only: no kernel unit includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

// shared by the translation units that include this header, not exported from libflacgpu.so
#define FG_LOCAL __attribute__((visibility("hidden")))

namespace fg {

// A grow-only device buffer of cap() elements of T.
template <class T>
class FG_LOCAL DevBuf {
    T *p_ = nullptr;
    uint64_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        DevBuf t(std::move(o));  // o is left empty; what this held goes with t
        std::swap(p_, t.p_);
        std::swap(cap_, t.cap_);
        return *this;
    }
    ~DevBuf() { hipFree(p_); }
    T *get() const { return p_; }
    uint64_t cap() const { return cap_; }
    // Nothing to do where `need` elements fit; otherwise the old buffer is freed and one of `need`
    // elements allocated, after *sync has drained where work queued on that stream may still use the
    // old one (NULL: the caller knows that none does).  On failure the buffer is left {nullptr, 0}.
    hipError_t grow(uint64_t need, const hipStream_t *sync = nullptr) {
        if (need <= cap_) return hipSuccess;
        hipError_t e = sync ? hipStreamSynchronize(*sync) : hipSuccess;
        if (e != hipSuccess) return e;
        hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
        e = hipMalloc(&p_, need * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        cap_ = need;
        return hipSuccess;
    }
};

// A HIP handle with its destroy function; Stream and Event add the one way each is created.
template <class H, hipError_t (*Destroy)(H)>
class FG_LOCAL Handle {
protected:
    H h_ = nullptr;

public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        Handle t(std::move(o));
        std::swap(h_, t.h_);
        return *this;
    }
    ~Handle() {
        if (h_) Destroy(h_);
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
};

struct FG_LOCAL Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};

struct FG_LOCAL Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = 0) { return hipEventCreateWithFlags(&h_, flags); }
};

// Carves one allocation into arrays, each aligned like an allocation of its own: take() hands the
// next n elements to each of its pointers and returns the bytes used so far.  A carve is written
// once, as a function of the base, and run twice (fit): on NULL for the size, then on the allocation.
struct Carve {
    uint8_t *base;
    uint64_t at = 0;
    template <class T, class... R>
    uint64_t take(uint64_t n, T *&p, R &...rest) {
        p = base ? (T *)(base + at) : nullptr;
        at += (n * sizeof(T) + 255u) & ~(uint64_t)255u;
        if constexpr (sizeof...(rest) > 0) take(n, rest...);
        return at;
    }
};

// Size, grow (DevBuf::grow's contract for `sync`), place: carve(base) returns the bytes it used.
template <class F>
hipError_t fit(DevBuf<uint8_t> &buf, F &&carve, const hipStream_t *sync = nullptr) {
    const hipError_t e = buf.grow(carve((uint8_t *)nullptr), sync);
    if (e == hipSuccess) carve(buf.get());
    return e;
}

}  // namespace fg
