// One owner per buffer of device or page-locked host memory.  Host only: no HIP header, no globals - the memory comes
// through four functions that are only declared here; the library's translation unit defines them over the HIP runtime
// (mpmpc_hip.hip), tests/device_buf/device_buf_check.cpp over malloc with an allocation that fails on request.
#pragma once
#include <cstddef>

namespace mpmpc {

// 0 = success, else the allocator's error code (the library's: hipError_t)
int device_alloc(void** p, size_t bytes);
int device_free(void* p);
int pinned_alloc(void** p, size_t bytes);
int pinned_free(void* p);

enum class Mem { Device, Pinned };

// Owns `count` elements of T, or nothing.  Converts to T*: kernel argument lists and copies read as with a raw pointer.
template <class T, Mem KIND = Mem::Device>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), count_(o.count_) { o.p_ = nullptr; o.count_ = 0; }
  Buf& operator=(Buf&& o) noexcept {      // (movable, not copyable: the move operations delete the copies)
    if (this != &o) { reset(); p_ = o.p_; count_ = o.count_; o.p_ = nullptr; o.count_ = 0; }
    return *this;
  }
  ~Buf() { reset(); }
  // frees what it holds, then allocates; on failure it holds nothing and returns the allocator's code
  int alloc(size_t count) {
    reset();
    const int e = KIND == Mem::Device ? device_alloc((void**)&p_, count * sizeof(T)) : pinned_alloc((void**)&p_, count * sizeof(T));
    if (e) p_ = nullptr; else count_ = count;
    return e;
  }
  void reset() {
    if (p_) (void)(KIND == Mem::Device ? device_free(p_) : pinned_free(p_));
    p_ = nullptr; count_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return count_; }

 private:
  T* p_ = nullptr; size_t count_ = 0;
};

// All or nothing: alloc_all(Want{a, na}, Want{b, nb}, ...) frees every member, then allocates them in order; on any failure
// every member is left empty and the code is returned.  "Any member empty" is then the same as "the group is not there".
template <class B> struct Want { B& buf; size_t count; };
template <class B> Want(B&, size_t) -> Want<B>;
template <class... B>
int alloc_all(Want<B>... want) {
  (want.buf.reset(), ...);
  int e = 0;
  ((e = e ? e : want.buf.alloc(want.count)), ...);
  if (e) (want.buf.reset(), ...);
  return e;
}

}  // namespace mpmpc
