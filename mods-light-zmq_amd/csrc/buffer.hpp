// Buf<T, Mem>: the one owner of a device or pinned host allocation of the library - a pointer and its capacity in elements.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace mods {

// where a Buf's memory comes from (stateless)
struct DevMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipFree(p); }
};
struct PinnedMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};
struct MappedMem {   // host memory the device reads and writes in place (hipHostGetDevicePointer gives its device address)
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};

// Move-only.  The capacity is set here and nowhere else: it is what the last successful allocation holds, and 0 after a failed
// one.  Streams, graphs and contexts are the caller's business (common.hpp: reserve_pool / reserve_scratch)
template <typename T, typename Mem = DevMem>
class Buf {
  T *p = nullptr;
  size_t cap = 0;   // elements

 public:
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Buf &operator=(Buf &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
  ~Buf() { release(); }

  T *get() const { return p; }
  operator T *() const { return p; }
  size_t capacity() const { return cap; }
  void swap(Buf &o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
  void release() { if (p) (void)Mem::free(p); p = nullptr; cap = 0; }
  T *detach() { T *r = p; p = nullptr; cap = 0; return r; }   // the caller owns (or deliberately leaks) the allocation

  // Room for `need` elements.  Nothing happens when they fit; otherwise the old allocation is freed (its contents are lost) and
  // one of alloc_elems >= need elements takes its place - how much more than `need` is the caller's growth policy.  On any failure
  // the buffer is empty.  *moved is set when the pointer changed (left alone otherwise)
  hipError_t reserve(size_t need, size_t alloc_elems, bool *moved = nullptr) {
    if (need <= cap) return hipSuccess;
    if (moved) *moved = true;
    if (alloc_elems < need) alloc_elems = need;
    hipError_t e = hipSuccess;
    if (p) { e = Mem::free(p); p = nullptr; cap = 0; }
    void *np = nullptr;
    if (e == hipSuccess) e = Mem::alloc(&np, alloc_elems * sizeof(T));
    if (e != hipSuccess) return e;
    p = static_cast<T *>(np); cap = alloc_elems;
    return hipSuccess;
  }
  hipError_t reserve(size_t need) { return reserve(need, need); }
};

template <typename T> using PinnedBuf = Buf<T, PinnedMem>;
template <typename T> using MappedBuf = Buf<T, MappedMem>;

// Buffers that share one capacity count, as (buffer, elements) pairs: reserve_group(a, na, b, nb, ...) allocates each exactly.
// When one allocation fails the whole group is emptied, so the caller's count - set only after hipSuccess - never claims room
// that one of them lacks
inline void release_group() {}
template <class B, class... Rest> inline void release_group(B &b, size_t, Rest &&...rest) { b.release(); release_group(rest...); }
inline hipError_t reserve_group() { return hipSuccess; }
template <class B, class... Rest> inline hipError_t reserve_group(B &b, size_t elems, Rest &&...rest) {
  hipError_t e = b.reserve(elems);
  if (e == hipSuccess) e = reserve_group(rest...); else release_group(rest...);
  if (e != hipSuccess) b.release();
  return e;
}

}  // namespace mods
