// devbuf.h -- the one place that allocates and frees device and pinned host memory: DevBuf<T> and PinnedBuf<T>, move-only
// owners of one block each.  No kernel code.  The reserve contract:
//   reserve_bytes(n)  nothing happens while the block holds n bytes or more; otherwise the old block is freed and exactly n
//                     bytes (16 for n = 0) are allocated.  Growth is exact, contents are NOT preserved, and a failed
//                     allocation leaves the buffer EMPTY (null, capacity 0) and returns the runtime's error, so the next
//                     call allocates again instead of trusting a capacity that no memory stands behind
//   borrow(p)         a non-owning view of somebody else's block (an ensemble member's slice): never freed, never grown
// The four allocator calls are macros, so a host program can stand in malloc and free (tests/host/devbuf_check.cpp).
#pragma once
#include <atomic>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#ifndef DEVBUF_DEV_ALLOC
#include <hip/hip_runtime.h>
typedef hipError_t devbuf_err_t;                       // 0 = success
#define DEVBUF_DEV_ALLOC(pp, bytes) hipMalloc(pp, bytes)
#define DEVBUF_DEV_FREE(p) hipFree(p)
#define DEVBUF_HOST_ALLOC(pp, bytes) hipHostMalloc(pp, bytes, hipHostMallocDefault)
#define DEVBUF_HOST_FREE(p) hipHostFree(p)
#endif

namespace devbuf {
// live owning blocks of this process and their bytes (pinn_debug_live_buffers); allocation is never on the step path
inline std::atomic<int64_t> live_blocks{0}, live_bytes{0};

template <typename T, bool PINNED>
class Buf {
  T* p_ = nullptr;
  size_t cap_ = 0;        // bytes owned; 0 for a view
  bool view_ = false;
  void forget() { p_ = nullptr; cap_ = 0; view_ = false; }

 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_), view_(o.view_) { o.forget(); }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; view_ = o.view_; o.forget(); }
    return *this;
  }
  ~Buf() { reset(); }

  void reset() {
    if (p_ && !view_) {
      if (PINNED) (void)DEVBUF_HOST_FREE((void*)p_); else (void)DEVBUF_DEV_FREE((void*)p_);
      live_blocks -= 1; live_bytes -= (int64_t)cap_;
    }
    forget();
  }
  devbuf_err_t reserve_bytes(size_t n) {
    assert(!view_ && "reserve on a borrowed view");
    if (p_ && cap_ >= n) return devbuf_err_t(0);
    reset();
    const size_t bytes = n ? n : 16;
    void* q = nullptr;
    const devbuf_err_t e = PINNED ? DEVBUF_HOST_ALLOC(&q, bytes) : DEVBUF_DEV_ALLOC(&q, bytes);
    if (e != devbuf_err_t(0)) return e;
    p_ = static_cast<T*>(q); cap_ = bytes;
    live_blocks += 1; live_bytes += (int64_t)bytes;
    return e;
  }
  template <typename U = T>
  devbuf_err_t reserve(size_t count) { return reserve_bytes(count * sizeof(U)); }      // typed buffers only
  void borrow(T* p) { reset(); p_ = p; view_ = true; }

  T* get() const { return p_; }
  size_t capacity_bytes() const { return cap_; }
  operator T*() const { return p_; }                    // kernel-argument lists and pointer arithmetic read as with a raw pointer
  template <typename U>
  U* as() const {                                       // the compute-dtype buffers: element type chosen at run time
    static_assert(std::is_void<T>::value, "as<U>() is for DevBuf<void>");
    return static_cast<U*>(p_);
  }
};
}  // namespace devbuf

template <typename T> using DevBuf = devbuf::Buf<T, false>;
template <typename T> using PinnedBuf = devbuf::Buf<T, true>;
