// DevBuf<T>: the one owner of device memory in the host runtime (rt_host.cpp) — a pointer and an element capacity,
// move-only.  Memory is released with hipFree, never an async free: replacing a lane's buffers while earlier work
// may still be queued relies on hipFree's implicit synchronisation.  A DevBuf must be destroyed (or reset) while
// the device it was allocated on is current.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace rtmi {

template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return n_; }  // elements asked for (0 while empty)
    void reset() {
        if (p_) hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // Grow-only: a block of at least n elements stays; otherwise the old block is freed first, then max(n, 1)
    // elements are allocated (the contents are not kept).  On failure the buffer is empty.
    hipError_t reserve(size_t n) {
        if (p_ && n_ >= n) return hipSuccess;
        reset();
        hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace rtmi
