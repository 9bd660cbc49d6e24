// What an entry point without a handle is built from (mpmpc_speed_profile, mpmpc_lidar_scan, ...: device ordinal and host arrays
// in, one block of device memory, a kernel or two, host arrays out): the layout of its block and the per-device scratch that
// holds the block between calls.  Host only: no HIP header - the memory comes through device_buf.hpp's device_alloc /
// device_free, a stream is named by the runtime's own opaque pointer type.  tests/scratch/scratch_check.cpp runs both under an
// allocator that fails on request; the library's translation unit adds the part that needs the runtime (scratch_acquire,
// mpmpc_handle.hpp).
#pragma once
#include <cassert>
#include <cstddef>
#include <mutex>

#include "device_buf.hpp"

typedef struct ihipStream_t* hipStream_t;      // (as hip_runtime_api.h declares it)

namespace mpmpc {

// `count` elements of T at byte `off` of a block: at(base) is the typed pointer, so the element type is stated once, where the
// region is reserved.  part(first, n) names elements first .. first + n - 1 of it - for arrays that a kernel finds back to back
// behind ONE pointer (the seen masks of K0s, the [3][B] results of the scan match), which are therefore one region.
template <class T>
struct Region {
  size_t off = 0, count = 0;
  T* at(char* base) const { return reinterpret_cast<T*>(base + off); }
  size_t bytes() const { return sizeof(T) * count; }
  Region part(size_t first, size_t n) const {
    assert(first + n <= count);
    return Region{off + sizeof(T) * first, n};
  }
};

// Hands out the regions of one block in order.  Every region starts on a multiple of 8 bytes (of the block's base: the
// allocator's alignment is far coarser); a region of no elements takes no bytes and leaves the layout as it was.
class Layout {
 public:
  template <class T>
  Region<T> add(size_t count) {
    static_assert(alignof(T) <= 8, "a region is aligned to 8 bytes");
    const Region<T> r{(end_ + 7) & ~size_t(7), count};
    if (count) end_ = r.off + r.bytes();
    return r;
  }
  size_t bytes() const { return end_; }

 private:
  size_t end_ = 0;
};

// The scratch of one entry point on one device, kept between calls (a call is a set-up step, and without this its cost was
// allocation: 3.5 of 4 ms for a speed profile of a single path).  Every entry point has a table of its own, one scratch per
// device, each behind its own mutex: callers of different entry points or on different devices neither serialise nor free each
// other's block.
// The block is a RAW pointer and is never freed: the tables have static storage, and an owner's destructor at process exit would
// call into a HIP runtime that may already be torn down.
struct SpScratch {
  std::mutex mu;
  size_t bytes = 0;
  char* block = nullptr;
  hipStream_t stream = nullptr;
};
constexpr int SP_MAX_DEVICES = 64;

// At least `need` bytes (call with g.mu held): a block that is large enough stays; else the old one is freed and a new one
// allocated.  A failed allocation leaves the scratch empty - the next call allocates again - and returns the allocator's code.
inline int grow(SpScratch& g, size_t need) {
  if (g.bytes >= need) return 0;
  if (g.block) (void)device_free(g.block);
  g.block = nullptr; g.bytes = 0;
  const int e = device_alloc((void**)&g.block, need);
  if (e) g.block = nullptr;
  else g.bytes = need;
  return e;
}

}  // namespace mpmpc
