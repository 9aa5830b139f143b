#pragma once
// bvcf_devmem.h — the owners of what bvcf_core.hip holds on the device: a buffer of device or of pinned host memory, a
// stream, an event.  Move-only; the destructor releases; a failed alloc / create leaves the owner empty, so a pointer and
// its size cannot disagree.  Host code only.
//
// Test mode (BVCF_POISON=XX, two hex digits; unset, empty or anything else: off, and alloc asks the runtime for exactly
// n * sizeof(T) bytes and touches nothing).  Read at every alloc, like the ctx's other knobs: it holds for a ctx created
// after it is set.  When on, alloc asks for kGuardBytes + payload + kGuardBytes, fills the payload with the byte XX and
// both guards with ~XX (poison copied into a guard shows), and lists the buffer -- a heap node that moves with its owner
// -- in a locked process-wide registry, under the file and line of the alloc call.  get() and size() describe the payload
// only.  guard_check() reads both guards of every live buffer (hipMemcpy for device memory, in place for pinned); reset()
// reads its own before it frees and records damage in the registry, since a destructor cannot report.  A damaged buffer is
// counted once.
// kGuardBytes = 4096 keeps the payload on the alignment the code relies on: 16 bytes for the u32x4 stores over a.census
// (bvcf_sites1.hip.h, "hipMalloc'ed: 16-byte aligned"), the .bed arena's aligned 16-byte pieces (bvcf_bedrows.hip.h) and
// the 64-byte records; 256 bytes as hipMalloc gives; the page that hipHostMalloc gives the pinned blocks the copies read.
// What the mode sees: an output that depends on bytes nobody wrote, and a store into a guard.  Not: a load out of bounds,
// a store that lands beyond the guard.
#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <utility>

namespace bvcf_mem {

constexpr size_t kGuardBytes = 4096;

// a live buffer of the test mode
struct Guarded {
  Guarded *prev = nullptr, *next = nullptr;
  unsigned char *base = nullptr;  // what the runtime gave: front guard, payload, back guard
  size_t bytes = 0;               // of the payload
  const char *file = "";
  int line = 0;
  int fill = 0;
  bool pinned = false;
  bool counted = false;  // its damage is in a count already
};

struct Registry {
  std::mutex mu;
  Guarded *head = nullptr;
  size_t live = 0;
  unsigned long freed_damaged = 0;  // buffers found damaged by reset() since the last guard_check()
  char first[256] = {0};            // ... and the first of them
};
inline Registry &registry() {
  static Registry *const r = new Registry;  // (never destroyed: owners may outlive every static)
  return *r;
}

// the fill byte, or -1: the mode is off
inline int poison_fill() {
  const char *e = getenv("BVCF_POISON");
  if (!e || !e[0] || !e[1] || e[2]) return -1;
  int v = 0;
  for (int i = 0; i < 2; i++) {
    const char c = e[i];
    const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    if (d < 0) return -1;
    v = v * 16 + d;
  }
  return v;
}

// reads g's guards; on damage writes "site: payload bytes, side, offset" into msg (if any).  The registry's lock is held
inline bool guards_damaged(const Guarded *g, char *msg, size_t cap) {
  static unsigned char host[kGuardBytes];  // (under the lock)
  const unsigned char want = (unsigned char)~g->fill;
  for (int side = 0; side < 2; side++) {
    const unsigned char *at = g->base + (side ? kGuardBytes + g->bytes : 0);
    bool unread = false;
    if (!g->pinned) {
      unread = hipMemcpy(host, at, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess;
      at = host;
    }
    for (size_t i = 0; i < kGuardBytes; i++)
      if (unread || at[i] != want) {
        // the offset counts from the payload's first byte: -1 is the byte in front of it, `bytes` the first one behind it
        const long long off = side ? (long long)(g->bytes + i) : (long long)i - (long long)kGuardBytes;
        if (msg && cap)
          snprintf(msg, cap, "%s:%d: %s buffer of %zu bytes: %s guard %s at offset %lld", g->file, g->line,
                   g->pinned ? "pinned" : "device", g->bytes, side ? "back" : "front", unread ? "unreadable" : "damaged", off);
        return true;
      }
  }
  return false;
}

// Checks every live buffer.  Returns how many buffers had a damaged guard since the last call, the ones reset() found
// included; msg receives the report of the first one (freed ones first), or an empty string
inline unsigned long guard_check(char *msg, size_t cap) {
  Registry &r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  unsigned long n = r.freed_damaged;
  if (msg && cap) snprintf(msg, cap, "%s", r.first);
  r.freed_damaged = 0;
  r.first[0] = 0;
  for (Guarded *g = r.head; g; g = g->next) {
    if (g->counted) continue;
    const bool want_msg = n == 0;
    if (guards_damaged(g, want_msg ? msg : nullptr, cap)) {
      g->counted = true;
      n++;
    }
  }
  return n;
}
inline size_t guarded_live() {
  Registry &r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  return r.live;
}

template <class T, bool kPinned>
class Buf {
 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)), g_(std::exchange(o.g_, nullptr)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
      g_ = std::exchange(o.g_, nullptr);
    }
    return *this;
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { reset(); }

  // frees what it holds, then n elements of T  (file, line: the caller's, the buffer's name in the test mode)
  hipError_t alloc(size_t n, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    reset();
    const size_t bytes = n * sizeof(T);
    const int fill = bytes ? poison_fill() : -1;
    void *p = nullptr;
    if (fill < 0) {
      const hipError_t e = raw_alloc(&p, bytes);
      if (e != hipSuccess || !p) return e;
      p_ = static_cast<T *>(p);
      n_ = n;
      return hipSuccess;
    }
    hipError_t e = raw_alloc(&p, bytes + 2 * kGuardBytes);
    if (e != hipSuccess || !p) return e;
    unsigned char *const base = static_cast<unsigned char *>(p);
    const int guard = (unsigned char)~fill;
    if (kPinned) {
      memset(base, guard, kGuardBytes);
      memset(base + kGuardBytes, fill, bytes);
      memset(base + kGuardBytes + bytes, guard, kGuardBytes);
    } else {
      e = hipMemset(base, guard, kGuardBytes);
      if (e == hipSuccess) e = hipMemset(base + kGuardBytes, fill, bytes);
      if (e == hipSuccess) e = hipMemset(base + kGuardBytes + bytes, guard, kGuardBytes);
      if (e == hipSuccess) e = hipDeviceSynchronize();  // (the ctx's streams do not wait for the null stream)
      if (e != hipSuccess) {
        (void)hipFree(base);
        return e;
      }
    }
    Guarded *const g = new Guarded;
    g->base = base;
    g->bytes = bytes;
    g->file = file;
    g->line = line;
    g->fill = fill;
    g->pinned = kPinned;
    Registry &r = registry();
    {
      std::lock_guard<std::mutex> lk(r.mu);
      g->next = r.head;
      if (r.head) r.head->prev = g;
      r.head = g;
      r.live++;
    }
    g_ = g;
    p_ = reinterpret_cast<T *>(base + kGuardBytes);
    n_ = n;
    return hipSuccess;
  }
  void reset() {
    if (g_) {
      Registry &r = registry();
      {
        std::lock_guard<std::mutex> lk(r.mu);
        char msg[sizeof r.first];
        if (!g_->counted && guards_damaged(g_, msg, sizeof msg)) {
          if (!r.freed_damaged++) memcpy(r.first, msg, sizeof msg);
        }
        (g_->prev ? g_->prev->next : r.head) = g_->next;
        if (g_->next) g_->next->prev = g_->prev;
        r.live--;
      }
      raw_free(g_->base);
      delete g_;
      g_ = nullptr;
    } else if (p_) {
      raw_free(p_);
    }
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  size_t size() const { return n_; }  // elements
  operator T *() const { return p_; }

 private:
  static hipError_t raw_alloc(void **p, size_t bytes) {
    return kPinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  }
  static void raw_free(void *p) { kPinned ? (void)hipHostFree(p) : (void)hipFree(p); }

  T *p_ = nullptr;
  size_t n_ = 0;
  Guarded *g_ = nullptr;  // test mode only
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
