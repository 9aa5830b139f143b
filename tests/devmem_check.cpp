// The owning types of bvcf_devmem.h, stand-alone (tests/test_devmem_cpu.py builds it with the address and undefined-
// behaviour sanitizers and runs it on a machine without a GPU).
//   default:            against the HIP runtime, where every allocation fails: the failure path
//   -DDEVMEM_STAND_INS: the runtime's calls replaced by malloc / free with counters: a double free or a lost buffer is
//                       an error of the sanitizer, and the counts must meet at the end
#include "bvcf_devmem.h"

#include <stdio.h>
#include <stdlib.h>

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
static bool g_fail_next = false;
static hipError_t stand_in_alloc(void **p, size_t n) {
  if (g_fail_next) {
    g_fail_next = false;
    return hipErrorOutOfMemory;
  }
  *p = malloc(n ? n : 1);
  g_allocs++;
  g_last_bytes = n;
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

int main() {
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
