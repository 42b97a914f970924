// owned.h -- who frees a device buffer, a pinned host buffer, an event or a stream: one move-only owner per handle, and one
// grow-only buffer.  Host-only like schedule.h: no HIP, the free and allocate calls are policies that ycnr_als.hip supplies
// (DevPtr, HostPtr, Event, Stream and the three GrowBuf aliases there).  tests/cpp/owned_test.cc runs it with counting policies.
#pragma once

#include <cstddef>
#include <utility>

namespace ycnr {

// Owner of one handle H (a pointer, an event, a stream); a value-initialised H is "empty".  Free{}(h) runs once per handle held:
// in the destructor, or where put(), reset() or a move assignment replaces it.  Non-owning views are filled from get().
template <typename H, typename Free>
class Owned {
 public:
  Owned() = default;
  explicit Owned(H h) : h_(h) {}
  ~Owned() { reset(); }
  Owned(Owned &&o) noexcept : h_(o.release()) {}
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned &) = delete;
  Owned &operator=(const Owned &) = delete;

  H get() const { return h_; }
  explicit operator bool() const { return h_ != H{}; }
  // for out-parameters that create a handle, create(owner.put(), ...): what was held is freed first
  H *put() {
    reset();
    return &h_;
  }
  void reset(H h = H{}) {
    const H old = h_;
    h_ = h;
    if (old != H{}) Free{}(old);
  }
  H release() {
    const H h = h_;
    h_ = H{};
    return h;
  }

 private:
  H h_{};
};

// Grow-only buffer.  Alloc supplies  static Err alloc(size_t, void **),  static void free(void *)  and  static size_t grow(size_t)
// -- the capacity to allocate for a request; Err{} is success.  reserve() within the capacity makes no call; beyond it the old
// block is freed BEFORE the new one is allocated (the contents are per-call scratch, and the peak stays at one block), and a
// failed allocation leaves the buffer empty and returns Alloc's code unchanged.
template <typename Alloc>
class GrowBuf {
 public:
  using Err = decltype(Alloc::alloc(size_t{}, static_cast<void **>(nullptr)));
  GrowBuf() = default;
  ~GrowBuf() { clear(); }
  GrowBuf(GrowBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  GrowBuf &operator=(GrowBuf &&o) noexcept {
    if (this != &o) {
      clear();
      p_ = std::exchange(o.p_, nullptr), cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  GrowBuf(const GrowBuf &) = delete;
  GrowBuf &operator=(const GrowBuf &) = delete;

  Err reserve(size_t bytes) {
    if (bytes <= cap_) return Err{};
    clear();
    const size_t want = Alloc::grow(bytes);
    const Err e = Alloc::alloc(want, &p_);
    if (e == Err{})
      cap_ = want;
    else
      p_ = nullptr;
    return e;
  }
  void clear() {
    if (p_) Alloc::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  void *get() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  void *p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace ycnr
