// devbuf_check.cpp -- csrc/devbuf.h on the host: the four allocator macros stand on malloc / free, counted, with a switch
// that makes the Nth allocation fail.  Built with -fsanitize=address,undefined by tests/test_devbuf_host.py, so a double
// free or a use of freed memory ends the program even where no CHECK looks; leaks it counts itself (g_held).  Needs no GPU and no HIP.
#include <cstdio>
#include <cstdlib>
#include <utility>

typedef int devbuf_err_t;
static long g_allocs = 0, g_frees = 0, g_fail_at = 0;      // g_fail_at: allocation number (1-based) that fails; 0 = none
static long g_held = 0;                                    // blocks malloc gave and free has not seen: the program's own leak count
static size_t g_last_bytes = 0;
static void* g_last_freed = nullptr;
static int counted_alloc(void** pp, size_t bytes) {
  g_allocs += 1;
  if (g_allocs == g_fail_at) { *pp = nullptr; return 2; }  // (2: the runtime's out-of-memory code)
  g_last_bytes = bytes;
  *pp = malloc(bytes);
  if (*pp) g_held += 1;
  return *pp ? 0 : 2;
}
static int counted_free(void* p) { g_frees += 1; g_held -= 1; g_last_freed = p; free(p); return 0; }
#define DEVBUF_DEV_ALLOC(pp, bytes) counted_alloc(pp, bytes)
#define DEVBUF_DEV_FREE(p) counted_free(p)
#define DEVBUF_HOST_ALLOC(pp, bytes) counted_alloc(pp, bytes)
#define DEVBUF_HOST_FREE(p) counted_free(p)
#include "../../pinns-tf2.0_amd/csrc/devbuf.h"

static int g_failed = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed += 1; } \
  } while (0)
static bool live_is(long n, long bytes) { return devbuf::live_blocks.load() == n && devbuf::live_bytes.load() == bytes; }

template <typename B>
static void reserve_contract() {
  const long a0 = g_allocs, f0 = g_frees;
  {
    B b;
    CHECK(b.get() == nullptr && b.capacity_bytes() == 0);
    CHECK(b.reserve_bytes(100) == 0 && b.get() && b.capacity_bytes() == 100 && g_last_bytes == 100);
    CHECK(g_allocs == a0 + 1 && g_frees == f0 && live_is(1, 100));
    void* const p = b.get();
    CHECK(b.reserve_bytes(100) == 0 && b.reserve_bytes(40) == 0 && b.reserve_bytes(0) == 0);   // below capacity: nothing
    CHECK(b.get() == p && g_allocs == a0 + 1 && g_frees == f0 && b.capacity_bytes() == 100);
    CHECK(b.reserve_bytes(101) == 0);                                  // growth: one free, then exactly the size asked
    CHECK(g_frees == f0 + 1 && g_last_freed == p && g_allocs == a0 + 2 && g_last_bytes == 101);
    CHECK(b.capacity_bytes() == 101 && live_is(1, 101));
    b.reset();
    CHECK(b.get() == nullptr && b.capacity_bytes() == 0 && g_frees == f0 + 2 && live_is(0, 0));
    b.reset();                                                         // an empty buffer frees nothing
    CHECK(g_frees == f0 + 2);
    CHECK(b.reserve_bytes(0) == 0 && b.get() && b.capacity_bytes() == 16 && g_last_bytes == 16);   // 0 bytes gives 16
  }
  CHECK(g_frees == f0 + 3 && live_is(0, 0));                           // the destructor frees
}

// the stale-capacity case: a failed growth leaves nothing behind, so a smaller request allocates again
template <typename B>
static void failed_growth() {
  {
    B b;
    CHECK(b.reserve_bytes(64) == 0);
    const long a0 = g_allocs, f0 = g_frees;
    g_fail_at = g_allocs + 1;
    CHECK(b.reserve_bytes(128) != 0);
    CHECK(b.get() == nullptr && b.capacity_bytes() == 0 && g_frees == f0 + 1 && live_is(0, 0));
    CHECK(b.reserve_bytes(32) == 0);                                   // would pass a capacity of 64 that nothing stands behind
    CHECK(b.get() && b.capacity_bytes() == 32 && g_allocs == a0 + 2 && g_last_bytes == 32 && live_is(1, 32));
    g_fail_at = g_allocs + 1;                                          // a first allocation that fails
    B c;
    CHECK(c.reserve_bytes(8) != 0 && c.get() == nullptr && c.capacity_bytes() == 0 && live_is(1, 32));
    g_fail_at = 0;
  }
  CHECK(live_is(0, 0));
}

static void moves() {
  const long f0 = g_frees;
  {
    DevBuf<double> a;
    CHECK(a.reserve(10) == 0 && a.capacity_bytes() == 80);
    double* const p = a.get();
    DevBuf<double> b(std::move(a));                                    // construction: a is empty, b owns
    CHECK(a.get() == nullptr && a.capacity_bytes() == 0 && b.get() == p && b.capacity_bytes() == 80 && live_is(1, 80));
    DevBuf<double> c;
    CHECK(c.reserve(4) == 0 && live_is(2, 112));
    double* const q = c.get();
    c = std::move(b);                                                  // assignment: c's old block is freed, once
    CHECK(g_frees == f0 + 1 && g_last_freed == q && c.get() == p && b.get() == nullptr && live_is(1, 80));
    c = std::move(c);                                                  // onto itself: nothing
    CHECK(c.get() == p && g_frees == f0 + 1);
    p[9] = 1.0;                                                        // still ours (the sanitizer would object otherwise)
    double* const raw = c;                                             // the conversion kernel-argument lists use
    CHECK(raw == p && c + 1 == p + 1);
  }
  CHECK(g_frees == f0 + 2 && live_is(0, 0));                           // p freed exactly once
}

static void views() {
  const long a0 = g_allocs, f0 = g_frees;
  double block[8];
  {
    DevBuf<double> v;
    v.borrow(block + 2);
    CHECK(v.get() == block + 2 && v.capacity_bytes() == 0 && live_is(0, 0));
    v.reset();                                                         // only forgets the pointer
    CHECK(v.get() == nullptr && g_frees == f0);
    DevBuf<double> own;
    CHECK(own.reserve(3) == 0);
    own.borrow(block);                                                 // an owner that becomes a view gives its block back first
    CHECK(g_frees == f0 + 1 && own.get() == block && live_is(0, 0));
    DevBuf<double> w(std::move(own));                                  // a moved view stays a view
    CHECK(w.get() == block && own.get() == nullptr);
    DevBuf<void> u;
    u.borrow(block);
    CHECK(u.as<double>() == block && u.as<float>() == (float*)block);
  }
  CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1 && live_is(0, 0));     // no view was freed
}

int main() {
  reserve_contract<DevBuf<void>>();
  reserve_contract<DevBuf<double>>();
  reserve_contract<PinnedBuf<int>>();
  failed_growth<DevBuf<void>>();
  failed_growth<PinnedBuf<double>>();
  moves();
  views();
  CHECK(g_allocs > 0 && g_frees > 0 && g_held == 0 && live_is(0, 0));
  if (g_failed) { fprintf(stderr, "devbuf_check: %d check(s) failed\n", g_failed); return 1; }
  printf("devbuf_check ok: %ld allocations, %ld frees\n", g_allocs, g_frees);
  return 0;
}
