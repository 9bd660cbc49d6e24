// csrc/device_scratch.hpp on its own: the layout of a scratch block and the scratch's grow under an allocator that fails on
// request.  Stand-alone: device_alloc / device_free are defined here over malloc / free, with a count of live blocks and "the
// k-th allocation fails"; built with -fsanitize=address,undefined (tests/emul/Makefile), run by tests/test_scratch.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "device_scratch.hpp"

static std::set<void*> g_live;
static long g_allocs = 0, g_fail_at = 0, g_frees = 0;
static int g_failures = 0;
constexpr int E_NO_MEMORY = 2;

namespace mpmpc {
int device_alloc(void** p, size_t bytes) {
  if (++g_allocs == g_fail_at) {
    *p = reinterpret_cast<void*>(0x1);      // a failing allocator may leave anything behind: the scratch must not keep it
    return E_NO_MEMORY;
  }
  *p = std::malloc(bytes ? bytes : 1);
  g_live.insert(*p);
  return 0;
}
int device_free(void* p) {
  if (g_live.erase(p) != 1) {      // freed twice or never allocated
    std::printf("FAIL: free of a block that is not live\n");
    ++g_failures;
    return 1;
  }
  ++g_frees;
  std::free(p);
  return 0;
}
int pinned_alloc(void**, size_t) { return E_NO_MEMORY; }      // (declared by device_buf.hpp; nothing here takes page-locked memory)
int pinned_free(void*) { return 1; }
}  // namespace mpmpc
using namespace mpmpc;

#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      std::printf("FAIL line %d (allocation %ld fails): %s\n", __LINE__, g_fail_at, #cond); \
      ++g_failures;                                                                         \
    }                                                                                       \
  } while (0)

// ---------------------------------------------------------------------------------------------- the layout
struct Span { size_t off, bytes, align; };
template <class T>
static Span span(const Region<T>& r, size_t want_count) {
  CHECK(r.count == want_count && r.bytes() == sizeof(T) * want_count);
  return Span{r.off, r.bytes(), alignof(T)};
}
// starts on multiples of 8, ascending, disjoint, every region as large as its elements need, the block ends with the last one
static void check_spans(const std::vector<Span>& s, size_t total) {
  size_t end = 0;
  for (const Span& r : s) {
    CHECK(r.off % 8 == 0 && r.off % r.align == 0);
    CHECK(r.off >= end);                       // ascending and disjoint: nothing starts inside its predecessor
    if (r.bytes) end = r.off + r.bytes;
  }
  CHECK(total == end);
}

// the block of mpmpc_lidar_scan_world as csrc/mpmpc_lidar.hpp and csrc/mpmpc_walls.hpp reserve it: B = 3 cars, 5 beams, 7 discs,
// a 4 x 6 map; without walls, or with 2 walls of total extent 9 (six header words a wall)
static void lidar_world_block(bool walls) {
  Layout L;
  std::vector<Span> s;
  s.push_back(span(L.add<double>(3 * 3), 9));        // pose
  s.push_back(span(L.add<double>(5), 5));            // angles
  s.push_back(span(L.add<double>(3 * 5), 15));       // ranges
  s.push_back(span(L.add<int>(3 + 1), 4));           // disc offsets
  s.push_back(span(L.add<int>(3 * 7), 21));          // discs: 84 bytes, the next region starts at the next multiple of 8
  s.push_back(span(L.add<int8_t>(4 * 6), 24));       // the map
  CHECK(s[5].off == 9 * 8 + 5 * 8 + 15 * 8 + 16 + 84 + 4);      // 332 -> 336
  const size_t before = L.bytes();
  CHECK(before == 336 + 24);
  if (walls) {
    s.push_back(span(L.add<int>(3 + 1), 4));         // wall offsets
    s.push_back(span(L.add<int>(6 * 2), 12));        // headers
    s.push_back(span(L.add<int>(4 * 2), 8));         // end cells
    s.push_back(span(L.add<int>(9), 9));             // the table: 36 bytes, 4 more to the next multiple of 8
    s.push_back(span(L.add<int>(2), 2));             // ok
    CHECK(s[6].off == before);
    CHECK(L.bytes() == before + 16 + 48 + 32 + 36 + 4 + 8);
  }
  check_spans(s, L.bytes());
}

static void layout_checks() {
  g_fail_at = 0;
  Layout L;
  CHECK(L.bytes() == 0);
  const auto a = L.add<int8_t>(3);      // 3 bytes: the next region starts at 8
  CHECK(a.off == 0 && L.bytes() == 3);
  const auto none = L.add<double>(0);      // a region of no elements takes nothing and moves nothing
  CHECK(none.count == 0 && none.bytes() == 0 && none.off % 8 == 0 && L.bytes() == 3);
  const auto b = L.add<int>(5);
  CHECK(b.off == 8 && L.bytes() == 8 + 20);
  const auto none2 = L.add<int>(0);
  CHECK(L.bytes() == 28 && none2.count == 0);
  const auto c = L.add<double>(2);
  CHECK(c.off == 32 && L.bytes() == 48);
  check_spans({span(a, 3), span(none, 0), span(b, 5), span(none2, 0), span(c, 2)}, L.bytes());
  // a typed handle resolves against the base to a pointer of its own type
  alignas(8) char base[48] = {};
  CHECK((void*)a.at(base) == (void*)base && (void*)b.at(base) == (void*)(base + 8) && (void*)c.at(base) == (void*)(base + 32));
  c.at(base)[1] = 2.5;
  b.at(base)[4] = 7;
  CHECK(c.at(base)[1] == 2.5 && b.at(base)[4] == 7);
  // arrays a kernel finds back to back are ONE region with a named split: the second part starts where the first one's
  // elements end, whatever the count (the seen masks of K0s: [B][2] then [B] ints; the scan match's [3][B])
  for (size_t nb : {size_t(1), size_t(3), size_t(64), size_t(65)}) {
    Layout M;
    (void)M.add<double>(nb);
    const auto seen = M.add<int>(3 * nb), discs = seen.part(0, 2 * nb), wall = seen.part(2 * nb, nb);
    CHECK(discs.off == seen.off && discs.count == 2 * nb);
    CHECK(wall.off == discs.off + sizeof(int) * discs.count && wall.count == nb);
    CHECK(wall.off + wall.bytes() == seen.off + seen.bytes() && M.bytes() == seen.off + seen.bytes());
    const auto out = M.add<int>(3 * nb), score = out.part(0, nb), cand = out.part(nb, nb), hits = out.part(2 * nb, nb);
    CHECK(cand.off == score.off + sizeof(int) * nb && hits.off == cand.off + sizeof(int) * nb);
    CHECK(discs.off % 8 == 0 && out.off % 8 == 0);      // (the discs' masks are read as 64-bit words)
  }
  lidar_world_block(false);
  lidar_world_block(true);
}

// ---------------------------------------------------------------------------------------------- grow
// One scenario: two scratches (as two devices of one table) each go small -> larger -> smaller -> larger again -> the same
// again; every allocation is numbered and allocation `fail_at` fails (0: none does).  -> allocations made
static long scenario(long fail_at) {
  g_allocs = 0;
  g_fail_at = fail_at;
  const size_t before = g_live.size();
  SpScratch table[2];
  const size_t needs[5] = {100, 1000, 50, 5000, 5000};
  for (SpScratch& g : table) {
    std::lock_guard<std::mutex> lock(g.mu);
    size_t held = 0;      // what the scratch must hold by now
    for (size_t need : needs) {
      const long allocs = g_allocs, frees = g_frees;
      char* const old = g.block;
      const int e = grow(g, need);
      if (held >= need) {      // fits: nothing allocated, nothing freed, the block stays
        CHECK(e == 0 && g_allocs == allocs && g_frees == frees && g.block == old && g.bytes == held);
        continue;
      }
      CHECK(g_allocs == allocs + 1);                        // (also: the call after a failed grow allocates, held being 0)
      CHECK(g_frees == frees + (held ? 1 : 0));             // the old block went exactly once, whether the new one came or not
      const bool fails = g_allocs == fail_at;
      CHECK(e == (fails ? E_NO_MEMORY : 0));
      if (fails) CHECK(g.block == nullptr && g.bytes == 0);
      else CHECK(g.block != nullptr && g.bytes == need && g_live.count(g.block) == 1);
      held = fails ? 0 : need;
      if (g.block) std::memset(g.block, 0x5a, g.bytes);     // (the sanitizer checks that the block is that large)
    }
    CHECK(held == 5000 && g.stream == nullptr);             // the repeated last call made good a failure of the one before
  }
  CHECK(g_live.size() == before + 2);                       // one block per scratch
  for (SpScratch& g : table) {                              // never freed by design: the program frees it for the leak check
    CHECK(device_free(g.block) == 0);
    g.block = nullptr;
  }
  return g_allocs;
}

int main() {
  layout_checks();
  const long n = scenario(0);      // no failure: counts the allocations
  long scenarios = 1;
  for (long k = 1; k <= n; ++k, ++scenarios) scenario(k);
  std::printf("scratch_check: %ld scenarios, %ld allocations in the scenario, %d failures, %zu blocks live\n", scenarios, n, g_failures,
              g_live.size());
  return g_failures == 0 && g_live.empty() ? 0 : 1;
}
