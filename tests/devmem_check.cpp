// The owning types of bvcf_devmem.h, stand-alone (tests/test_devmem_cpu.py builds it with the address and undefined-
// behaviour sanitizers and runs it on a machine without a GPU).
//   default:            against the HIP runtime, where every allocation fails: the failure path
//   -DDEVMEM_STAND_INS: the runtime's calls replaced by malloc / free with counters: a double free or a lost buffer is
//                       an error of the sanitizer, and the counts must meet at the end
#include "bvcf_devmem.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

using namespace bvcf_mem;

#define CHECK(x)                                                \
  do {                                                          \
    if (!(x)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                  \
    }                                                           \
  } while (0)

#ifdef DEVMEM_STAND_INS
static long g_allocs = 0, g_frees = 0, g_made = 0, g_destroyed = 0;
static size_t g_last_bytes = 0;
static unsigned g_last_flags = 0;
static bool g_fail_next = false, g_fail_memset = false;
static unsigned char *g_last_ptr = nullptr;  // what the stand-in gave: in test mode the front guard's first byte
static long g_memsets = 0, g_copies = 0, g_syncs = 0;
static hipError_t stand_in_alloc(void **p, size_t n) {
  if (g_fail_next) {
    g_fail_next = false;
    return hipErrorOutOfMemory;
  }
  *p = malloc(n ? n : 1);
  g_allocs++;
  g_last_bytes = n;
  g_last_ptr = static_cast<unsigned char *>(*p);
  return hipSuccess;
}
static hipError_t stand_in_free(void *p) {
  CHECK(p);  // (the owners never pass a null pointer on)
  free(p);
  g_frees++;
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return stand_in_alloc(p, n); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags) {
  g_last_flags = flags;
  return stand_in_alloc(p, n);
}
hipError_t hipFree(void *p) { return stand_in_free(p); }
hipError_t hipHostFree(void *p) { return stand_in_free(p); }
// (the test mode's: "device" memory is the heap here, so the fill and the guards' read-back are memset and memcpy)
hipError_t hipMemset(void *p, int v, size_t n) {
  if (g_fail_memset) {
    g_fail_memset = false;
    return hipErrorInvalidValue;
  }
  memset(p, v, n);
  g_memsets++;
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) {
  CHECK(kind == hipMemcpyDeviceToHost);
  memcpy(dst, src, n);
  g_copies++;
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  g_syncs++;
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  g_made++;
  *s = (hipStream_t)malloc(1);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  g_made++;
  *e = (hipEvent_t)malloc(1);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  g_destroyed++;
  free(s);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  g_destroyed++;
  free(e);
  return hipSuccess;
}
}
#endif

struct Rec {
  int a, b, c;
};

template <class B>
static void check_failed_alloc(const char *what) {
#ifndef DEVMEM_STAND_INS
  B b;
  const hipError_t e = b.alloc(1000);
  printf("%s: alloc -> %d (%s)\n", what, (int)e, hipGetErrorString(e));
  CHECK(e != hipSuccess);
  CHECK(b.get() == nullptr && b.size() == 0);
  CHECK(b.alloc(7) != hipSuccess);  // a second alloc, and a reset, on the empty owner
  CHECK(b.get() == nullptr && b.size() == 0);
  b.reset();
  CHECK(b.get() == nullptr && b.size() == 0);
#else
  B b;
  CHECK(b.alloc(10) == hipSuccess && b.get() && b.size() == 10);
  g_fail_next = true;  // a failed regrow: what it held is gone, pointer and size agree
  CHECK(b.alloc(1000) == hipErrorOutOfMemory);
  CHECK(b.get() == nullptr && b.size() == 0);
  b.reset();
  CHECK(b.alloc(3) == hipSuccess && b.size() == 3);  // ... and the owner can be used again
  (void)what;
#endif
}

template <class B>
static void check_moves() {
  typedef decltype(std::declval<B>().get()) Ptr;
  B a;
  (void)a.alloc(5);  // (fails without the stand-ins: the moves of empty owners)
  const Ptr p = a.get();
  const size_t n = a.size();
  const Ptr conv = a;  // the implicit conversion
  CHECK(conv == p);
  B b(std::move(a));
  CHECK(a.get() == nullptr && a.size() == 0);
  CHECK(b.get() == p && b.size() == n);
  B c;
  (void)c.alloc(9);
  c = std::move(b);  // releases what c held
  CHECK(b.get() == nullptr && b.size() == 0);
  CHECK(c.get() == p && c.size() == n);
  B &self = c;
  c = std::move(self);
  CHECK(c.get() == p && c.size() == n);
  std::vector<B> v(3);  // as std::vector<Slot>::resize does
  v[1] = std::move(c);
  v.resize(40);
  CHECK(v[1].get() == p && v[1].size() == n && v[39].get() == nullptr);
  B empty, from_empty(std::move(empty));
  CHECK(from_empty.get() == nullptr && from_empty.size() == 0);
}  // every owner destroyed here: empty, moved-from and full ones

template <class H>
static void check_handle(bool make) {
  H a;
  CHECK(a.get() == nullptr && !a);
  a.reset();
  if (make) CHECK(a.create(0) == hipSuccess && a.get() != nullptr);
  const auto h = a.get();
  const decltype(a.get()) conv = a;
  CHECK(conv == h);
  H b(std::move(a));
  CHECK(a.get() == nullptr && b.get() == h);
  H c;
  if (make) CHECK(c.create(0) == hipSuccess);
  c = std::move(b);
  CHECK(b.get() == nullptr && c.get() == h);
  std::vector<H> v(2);
  v[0] = std::move(c);
  v.resize(20);
  CHECK(v[0].get() == h && c.get() == nullptr);
}

#ifdef DEVMEM_STAND_INS
static bool all_bytes(const unsigned char *p, size_t n, unsigned char v) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != v) return false;
  return true;
}

// The test mode (BVCF_POISON).  A guard is damaged here by a store through the pointer the stand-in allocator gave -- the
// front guard's first byte -- so every store stays inside the program's own block.
template <class B>
static void check_poison(const char *kind, bool pinned) {
  char msg[256], want[256];
  const size_t esz = sizeof(*std::declval<B>().get());
  CHECK(setenv("BVCF_POISON", "a5", 1) == 0);
  CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 0 && !msg[0]);
  const long memsets = g_memsets, syncs = g_syncs, copies = g_copies;
  {  // the layout, the fills, intact guards, one byte in front of the payload
    B b;
    const int line = __LINE__ + 1;
    CHECK(b.alloc(10) == hipSuccess);
    const size_t bytes = 10 * esz;
    unsigned char *const base = g_last_ptr;
    CHECK(g_last_bytes == bytes + 2 * kGuardBytes);
    CHECK(reinterpret_cast<unsigned char *>(b.get()) == base + kGuardBytes && b.size() == 10);
    CHECK(all_bytes(base, kGuardBytes, 0x5a) && all_bytes(base + kGuardBytes, bytes, 0xa5) &&
          all_bytes(base + kGuardBytes + bytes, kGuardBytes, 0x5a));
    CHECK(g_memsets == memsets + (pinned ? 0 : 3) && g_syncs == syncs + (pinned ? 0 : 1));  // hipMemset for device memory only
    CHECK(guarded_live() == 1 && guard_check(msg, sizeof msg) == 0 && !msg[0]);
    base[kGuardBytes - 1] = 0xa5;  // (poison copied one element too far down)
    snprintf(want, sizeof want, "%s:%d: %s buffer of %zu bytes: front guard damaged at offset -1", __FILE__, line, kind, bytes);
    CHECK(guard_check(msg, sizeof msg) == 1);
    if (strcmp(msg, want)) fprintf(stderr, "got  %s\nwant %s\n", msg, want);
    CHECK(!strcmp(msg, want));
    CHECK(guard_check(msg, sizeof msg) == 0 && !msg[0]);  // a buffer counts once ...
  }
  CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 0);  // ... also when it is freed
  {  // one byte behind the payload of a buffer that has moved twice; the move-assignment frees and unlists c's own
    B a;
    const int line = __LINE__ + 1;
    CHECK(a.alloc(3) == hipSuccess);
    unsigned char *const base = g_last_ptr;
    B b(std::move(a));
    B c;
    CHECK(c.alloc(4) == hipSuccess && guarded_live() == 2);
    c = std::move(b);
    CHECK(guarded_live() == 1 && guard_check(msg, sizeof msg) == 0);
    base[kGuardBytes + 3 * esz] = 0;
    snprintf(want, sizeof want, "%s:%d: %s buffer of %zu bytes: back guard damaged at offset %zu", __FILE__, line, kind, 3 * esz,
             3 * esz);
    CHECK(guard_check(msg, sizeof msg) == 1);
    if (strcmp(msg, want)) fprintf(stderr, "got  %s\nwant %s\n", msg, want);
    CHECK(!strcmp(msg, want));
    std::vector<B> v(2);  // the registry follows a vector's reallocation
    v[1] = std::move(c);
    v.resize(50);
    CHECK(guarded_live() == 1 && reinterpret_cast<unsigned char *>(v[1].get()) == base + kGuardBytes);
  }
  CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 0);
  int line5 = 0;
  {  // damage that only reset() sees is reported by the next check; an intact buffer freed beside it is not
    B a, ok;
    line5 = __LINE__ + 1;
    CHECK(a.alloc(5) == hipSuccess);
    g_last_ptr[kGuardBytes + 5 * esz + 7] ^= 1;
    CHECK(ok.alloc(6) == hipSuccess);
  }
  snprintf(want, sizeof want, "%s:%d: %s buffer of %zu bytes: back guard damaged at offset %zu", __FILE__, line5, kind, 5 * esz,
           5 * esz + 7);
  CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 1);
  if (strcmp(msg, want)) fprintf(stderr, "got  %s\nwant %s\n", msg, want);
  CHECK(!strcmp(msg, want));
  CHECK(guard_check(msg, sizeof msg) == 0 && !msg[0]);
  {  // a failed allocation, and a failed fill, leave an empty owner and an empty registry
    B a;
    CHECK(a.alloc(2) == hipSuccess && guarded_live() == 1);
    g_fail_next = true;
    CHECK(a.alloc(100) == hipErrorOutOfMemory);
    CHECK(a.get() == nullptr && a.size() == 0 && guarded_live() == 0);
    if (!pinned) {
      g_fail_memset = true;
      CHECK(a.alloc(100) == hipErrorInvalidValue);
      CHECK(a.get() == nullptr && a.size() == 0 && guarded_live() == 0);
    }
    CHECK(a.alloc(0) == hipSuccess && g_last_bytes == 0 && guarded_live() == 0);  // (no bytes: as without the mode)
    CHECK(a.alloc(1) == hipSuccess && a.size() == 1 && guarded_live() == 1);
  }
  check_moves<B>();  // every move of the plain mode, on listed buffers
  CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 0 && !msg[0]);
  CHECK(pinned ? g_copies == copies : g_copies > copies);  // device guards come back through hipMemcpy, pinned are read in place

  // off: unset, empty, and anything that is not two hex digits -- exactly the bytes asked for, nothing touched or listed
  const char *const off[] = {nullptr, "", "a", "a5x", "g0", "0x"};
  for (const char *v : off) {
    CHECK((v ? setenv("BVCF_POISON", v, 1) : unsetenv("BVCF_POISON")) == 0);
    const long m = g_memsets, c = g_copies, s = g_syncs;
    B b;
    CHECK(b.alloc(4) == hipSuccess && g_last_bytes == 4 * esz);
    CHECK(reinterpret_cast<unsigned char *>(b.get()) == g_last_ptr && b.size() == 4);
    CHECK(guarded_live() == 0 && guard_check(msg, sizeof msg) == 0 && !msg[0]);
    b.reset();
    CHECK(g_memsets == m && g_copies == c && g_syncs == s);
  }
  {  // a buffer of the mode outlives the knob: it is still checked and freed whole
    CHECK(setenv("BVCF_POISON", "00", 1) == 0);
    B b;
    CHECK(b.alloc(2) == hipSuccess && all_bytes(g_last_ptr, kGuardBytes, 0xff) && all_bytes(g_last_ptr + kGuardBytes, 2 * esz, 0));
    CHECK(unsetenv("BVCF_POISON") == 0);
    CHECK(guarded_live() == 1 && guard_check(msg, sizeof msg) == 0);
  }
  CHECK(guarded_live() == 0);
}
#endif

int main() {
#ifdef DEVMEM_STAND_INS
  CHECK(unsetenv("BVCF_POISON") == 0);
#endif
  check_failed_alloc<DevBuf<Rec>>("device");
  check_failed_alloc<PinBuf<Rec>>("pinned");
  check_moves<DevBuf<Rec>>();
  check_moves<PinBuf<unsigned char>>();
#ifdef DEVMEM_STAND_INS
  {
    DevBuf<Rec> d;
    CHECK(d.alloc(11) == hipSuccess && g_last_bytes == 11 * sizeof(Rec));  // elements in, bytes to the runtime
    PinBuf<Rec> h;
    CHECK(h.alloc(4) == hipSuccess && g_last_bytes == 4 * sizeof(Rec) && g_last_flags == hipHostMallocDefault);
  }
  check_handle<Stream>(true);
  check_handle<Event>(true);
  check_poison<DevBuf<Rec>>("device", false);
  check_poison<PinBuf<unsigned char>>("pinned", true);
  CHECK(g_copies > 0);  // (device guards are read through hipMemcpy, pinned ones in place)
  printf("poison ok\n");
#endif
  check_handle<Stream>(false);  // (no stream or event is created against the runtime)
  check_handle<Event>(false);
#ifdef DEVMEM_STAND_INS
  printf("allocs %ld frees %ld handles %ld destroyed %ld\n", g_allocs, g_frees, g_made, g_destroyed);
  CHECK(g_allocs > 0 && g_allocs == g_frees && g_made > 0 && g_made == g_destroyed);
#endif
  printf("devmem ok\n");
  return 0;
}
