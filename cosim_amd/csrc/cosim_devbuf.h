// cosim_devbuf.h -- DevBuf<T, Alloc>: the one owner of an allocation of `count` elements of T.  Plain C++17, no HIP:
// cosim_engine.hip supplies the allocator policies over hipMalloc / hipHostMalloc, tests/devbuf_host.cpp builds it alone over a
// counting allocator on std::malloc.
//
// Move-only.  The destructor frees, a move leaves the source empty, move assignment frees what the destination held.  A failed
// alloc leaves the object empty, never dangling.  The two ways the engine's setters use it ("Owning device buffers"):
//   build, then commit   fill a local group of buffers, return on an error (the destructors undo it, what is set stays), then
//                        move-assign the group into the engine;
//   drop first           assign an empty group to the engine, then the same: one copy at the peak, nothing set after a failure.
// Structs handed to a kernel by value hold raw pointers, filled from get(): no DevBuf is ever memset or passed to a launch.
//
// Alloc: using error_t; static constexpr error_t ok; static error_t malloc(void**, size_t bytes), memset(void*, int, size_t bytes),
// to_device(void* dst, const void* host, size_t bytes), to_host(void* host, const void* src, size_t bytes); static void free(void*).
#pragma once
#include <cstddef>

namespace cosim {

template <class T, class Alloc>
class DevBuf {
 public:
  using error_t = typename Alloc::error_t;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }

  void reset() {
    if (p_) Alloc::free(p_);
    p_ = nullptr; n_ = 0;
  }
  // what was held goes first.  count 0: empty, no error (the allocators hand out no block of no bytes)
  error_t alloc(size_t count) {
    reset();
    if (count == 0) return Alloc::ok;
    void* q = nullptr;
    const error_t r = Alloc::malloc(&q, count * sizeof(T));
    if (r == Alloc::ok && q) { p_ = static_cast<T*>(q); n_ = count; }
    return r;
  }
  error_t alloc_zeroed(size_t count) {
    error_t r = alloc(count);
    if (r == Alloc::ok && p_) r = Alloc::memset(p_, 0, n_ * sizeof(T));
    if (r != Alloc::ok) reset();
    return r;
  }
  // a fresh block of `count` elements with the host's values in it
  error_t upload(const T* host, size_t count) {
    error_t r = alloc(count);
    if (r == Alloc::ok && p_) r = Alloc::to_device(p_, host, n_ * sizeof(T));
    if (r != Alloc::ok) reset();
    return r;
  }
  // the first `count` elements (at most size()) to the host
  error_t download(T* host, size_t count) const { return Alloc::to_host(host, p_, (count < n_ ? count : n_) * sizeof(T)); }

  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace cosim
