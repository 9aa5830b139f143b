#pragma once
// bvcf_devmem.h — the owners of what bvcf_core.hip holds on the device: a buffer of device or of pinned host memory, a
// stream, an event.  Move-only; the destructor releases; a failed alloc / create leaves the owner empty, so a pointer and
// its size cannot disagree.  Host code only.
#include <hip/hip_runtime_api.h>

#include <stddef.h>

#include <utility>

namespace bvcf_mem {

template <class T, bool kPinned>
class Buf {
 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { reset(); }

  // frees what it holds, then n elements of T
  hipError_t alloc(size_t n) {
    reset();
    void *p = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess || !p) return e;
    p_ = static_cast<T *>(p);
    n_ = n;
    return hipSuccess;
  }
  void reset() {
    if (p_) kPinned ? (void)hipHostFree(p_) : (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  size_t size() const { return n_; }  // elements
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

template <class T>
using DevBuf = Buf<T, false>;
template <class T>
using PinBuf = Buf<T, true>;

template <class H, hipError_t (*kDestroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle &operator=(Handle &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  Handle(const Handle &) = delete;
  Handle &operator=(const Handle &) = delete;
  ~Handle() { reset(); }

  void reset() {
    if (h_) (void)kDestroy(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  hipError_t adopt(hipError_t e, H h) {
    h_ = e == hipSuccess ? h : nullptr;
    return e;
  }

 private:
  H h_ = nullptr;
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    hipStream_t s = nullptr;
    return adopt(hipStreamCreateWithFlags(&s, flags), s);
  }
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    hipEvent_t ev = nullptr;
    return adopt(hipEventCreateWithFlags(&ev, flags), ev);
  }
};

}  // namespace bvcf_mem
