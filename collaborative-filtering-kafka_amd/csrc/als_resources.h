// als_resources.h -- owners of the device resources the host code holds (host-only): each wraps exactly the HIP calls
// the engine made by hand before, is move-only, and releases in its destructor. The only place in csrc/ that calls
// hipMalloc / hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace cfk {

// n elements of T in device memory (T = char: a byte workspace).
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // Replaces the buffer (n = 0: none). On failure the buffer is empty.
    hipError_t alloc(size_t n) {
        reset();
        if (n == 0) return hipSuccess;
        const hipError_t st = hipMalloc((void**)&p_, n * sizeof(T));
        if (st == hipSuccess) n_ = n;
        else p_ = nullptr;
        return st;
    }
    // Grow-only: the old buffer is freed BEFORE the larger one is allocated (contents are not kept), so the peak is
    // the larger of the two, never their sum.
    hipError_t reserve(size_t n) { return n > n_ ? alloc(n) : hipSuccess; }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Pinned host staging memory.
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p_) (void)hipHostFree(p_);
    }
    hipError_t reserve(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        bytes_ = 0;
        const hipError_t st = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
        if (st == hipSuccess) bytes_ = bytes;
        return st;
    }
    void* get() const { return p_; }
    size_t bytes() const { return bytes_; }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// A stream the holder created (drained and destroyed on release) or borrowed from the caller (left alone).
class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { (void)release(); }
    hipError_t create() {
        hipError_t st = release();
        if (st == hipSuccess) st = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        own_ = st == hipSuccess;
        return st;
    }
    hipError_t borrow(hipStream_t s) {   // nullptr: the legacy default stream
        const hipError_t st = release();
        if (st == hipSuccess) s_ = s;
        return st;
    }
    hipError_t release() {
        if (!own_) {
            s_ = nullptr;
            return hipSuccess;
        }
        hipError_t st = hipStreamSynchronize(s_);
        if (st == hipSuccess) st = hipStreamDestroy(s_);
        if (st == hipSuccess) {
            own_ = false;
            s_ = nullptr;
        }
        return st;
    }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
    bool own_ = false;
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags = hipEventDefault) {   // once per Event
        return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags);
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace cfk
