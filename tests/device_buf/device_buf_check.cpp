// csrc/device_buf.hpp under an allocator that fails on request.  Stand-alone: the four allocator functions are defined here
// over malloc / free, with a count of live blocks and "the k-th allocation fails"; built with -fsanitize=address,undefined
// (tests/emul/Makefile), run by tests/test_device_buf.py.  For k = 1 .. the allocations of the scenario the properties of the
// owner are checked, and after every scenario no block is live - this program's count, and the sanitizer's leak check at exit.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "device_buf.hpp"

static std::set<void*> g_live[2];      // device, pinned
static long g_allocs = 0, g_fail_at = 0, g_frees = 0;
static int g_failures = 0;
constexpr int E_NO_MEMORY = 2;

static int take(int kind, void** p, size_t bytes) {
  if (++g_allocs == g_fail_at) {
    *p = reinterpret_cast<void*>(0x1);      // a failing allocator may leave anything behind: the owner must not keep it
    return E_NO_MEMORY;
  }
  *p = std::malloc(bytes ? bytes : 1);
  g_live[kind].insert(*p);
  return 0;
}
static int give(int kind, void* p) {
  if (g_live[kind].erase(p) != 1) {      // freed twice, never allocated, or through the other kind's function
    std::printf("FAIL: free of a block that is not live (kind %d)\n", kind);
    ++g_failures;
    return 1;
  }
  ++g_frees;
  std::free(p);
  return 0;
}
namespace mpmpc {
int device_alloc(void** p, size_t bytes) { return take(0, p, bytes); }
int device_free(void* p) { return give(0, p); }
int pinned_alloc(void** p, size_t bytes) { return take(1, p, bytes); }
int pinned_free(void* p) { return give(1, p); }
}  // namespace mpmpc
using namespace mpmpc;

#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      std::printf("FAIL line %d (allocation %ld fails): %s\n", __LINE__, g_fail_at, #cond); \
      ++g_failures;                                                                         \
    }                                                                                       \
  } while (0)
static size_t live() { return g_live[0].size() + g_live[1].size(); }
template <class B>
static bool empty(const B& b) { return b.get() == nullptr && b.count() == 0 && !b; }
template <class B>
static bool holds(const B& b, size_t n) { return b.get() != nullptr && b.count() == n; }

// One scenario: every allocation of it is numbered, allocation `fail_at` fails (0: none does).  -> allocations it made
static long scenario(long fail_at) {
  g_allocs = 0;
  g_fail_at = fail_at;
  {
    // alloc over a held buffer frees the old block; a failed alloc leaves the buffer empty
    Buf<double> a;
    CHECK(empty(a));
    int e = a.alloc(10);                                     // allocation 1
    CHECK(e == (fail_at == 1 ? E_NO_MEMORY : 0));
    CHECK(e ? empty(a) : holds(a, 10));
    if (!e) { a[0] = 1.0; a[9] = 2.0; }
    const long frees = g_frees;
    const size_t before = live();
    e = a.alloc(20);                                         // allocation 2
    CHECK(g_frees == frees + (before ? 1 : 0));              // the old block went, whether the new one came or not
    CHECK(e == (fail_at == 2 ? E_NO_MEMORY : 0));
    CHECK(e ? empty(a) && live() == 0 : holds(a, 20) && live() == 1);
    double* raw = a;                                         // reads as a pointer
    CHECK(raw == a.get());

    // move construction: the source is empty, the block has one owner
    Buf<double> b(std::move(a));
    CHECK(empty(a));
    CHECK(b.get() == raw && b.count() == (raw ? 20u : 0u));
    // move assignment: the destination's old block is freed exactly once, the source is empty
    Buf<double> c;
    e = c.alloc(5);                                          // allocation 3
    CHECK(e == (fail_at == 3 ? E_NO_MEMORY : 0));
    const long frees2 = g_frees;
    const bool c_held = c.get() != nullptr;
    c = std::move(b);
    CHECK(g_frees == frees2 + (c_held ? 1 : 0));
    CHECK(empty(b) && c.get() == raw);
    c = std::move(c);                                        // onto itself: nothing happens
    CHECK(c.get() == raw && g_frees == frees2 + (c_held ? 1 : 0));
    // a struct of buffers can be reset by assignment (what the launch slots do)
    struct Pair { Buf<int> x; Buf<unsigned, Mem::Pinned> y; int tag = 0; };
    Pair s;
    e = s.x.alloc(3);                                        // allocation 4
    CHECK(e ? empty(s.x) : holds(s.x, 3));
    e = s.y.alloc(2);                                        // allocation 5 (page-locked)
    CHECK(e ? empty(s.y) : holds(s.y, 2) && g_live[1].count(s.y.get()) == 1);
    s.tag = 7;
    s = Pair{};
    CHECK(empty(s.x) && empty(s.y) && s.tag == 0 && g_live[1].empty());

    // alloc_all over three buffers, two of them holding something: all three or none
    Buf<double> g0;
    Buf<int> g1;
    Buf<char, Mem::Pinned> g2;
    e = g0.alloc(4);                                         // allocation 6
    e = g2.alloc(4);                                         // allocation 7
    const long at = g_allocs;
    e = alloc_all(Want{g0, 8}, Want{g1, 16}, Want{g2, 32});  // allocations 8, 9, 10
    const bool fails = fail_at > at && fail_at <= at + 3;
    CHECK(e == (fails ? E_NO_MEMORY : 0));
    if (fails) CHECK(empty(g0) && empty(g1) && empty(g2));
    else CHECK(holds(g0, 8) && holds(g1, 16) && holds(g2, 32));
    CHECK(g_allocs == at + (fails ? fail_at - at : 3));      // nothing is allocated behind the failure
    // ... and the group can be allocated again after a failure
    if (fails) {
      e = alloc_all(Want{g0, 8}, Want{g1, 16}, Want{g2, 32});
      CHECK(e == 0 && holds(g0, 8) && holds(g1, 16) && holds(g2, 32));
    }
    g1.reset();
    CHECK(empty(g1));
    g1.reset();                                              // twice: nothing to free
  }
  CHECK(live() == 0);                                        // the destructors freed the rest
  return g_allocs;
}

int main() {
  const long n = scenario(0);      // no failure: counts the allocations
  long scenarios = 1;
  for (long k = 1; k <= n; ++k, ++scenarios) scenario(k);
  std::printf("device_buf_check: %ld scenarios, %ld allocations in the scenario, %d failures, %zu blocks live\n", scenarios, n,
              g_failures, live());
  return g_failures == 0 && live() == 0 ? 0 : 1;
}
