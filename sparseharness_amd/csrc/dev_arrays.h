// dev_arrays.h -- the owner of device arrays that the handles of engine.hip hold: whatever it allocated or adopted is
// released with it, and `bytes` is what the handle's footprint reports.  A graph handle holds one for its arrays and a
// create function a second one for the temporaries of the build, which so go on every return path; a matrix holds one
// per layout, so that dropping a layout is assigning an empty one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

struct DevArrays {
  struct Held { void *p; size_t size; };   // size: the bytes behind p
  std::vector<Held> held;
  size_t bytes = 0;
  DevArrays() = default;
  DevArrays(const DevArrays &) = delete;
  DevArrays &operator=(DevArrays &&o) noexcept {   // (what this one held is released)
    std::swap(held, o.held);
    std::swap(bytes, o.bytes);
    o.release();
    return *this;
  }
  ~DevArrays() { release(); }
  void release() {
    for (const Held &h : held) (void)hipFree(h.p);
    held.clear();
    bytes = 0;
  }
  // The matrix layouts' rule: `nbytes` (slack for the kernels' wide loads included) are allocated and counted; an array
  // of no bytes is no allocation and stays NULL.
  template <class T>
  hipError_t alloc_exact(T **p, size_t nbytes) {
    void *q = nullptr;
    const hipError_t r = hipMalloc(&q, nbytes);
    if (r == hipSuccess && q) adopt(q, nbytes);
    if (r == hipSuccess) *p = (T *)q;
    return r;
  }
  // The graph handles' rule: an array of `nbytes` counts as that; an empty one still gets a few bytes to point at.
  template <class T>
  hipError_t alloc(T **p, int64_t nbytes) {
    const size_t pad = std::max<size_t>((size_t)nbytes, 16) - (size_t)nbytes;
    const hipError_t r = alloc_exact(p, (size_t)nbytes + pad);
    if (r == hipSuccess) bytes -= pad;
    return r;
  }
  // An array allocated elsewhere (plan_gpu.hip) with `nbytes` behind it: owned and counted from here on.
  void adopt(void *p, size_t nbytes) {
    held.push_back({p, nbytes});
    bytes += nbytes;
  }
  size_t size_of(const void *p) const {   // the bytes behind an array held here (0: not held)
    for (const Held &h : held)
      if (h.p == p) return h.size;
    return 0;
  }
  // The entry of `old` holds `fresh` (as many bytes, allocated by the caller) from here on, and `old` is the caller's to
  // free: a placement trial moves an array without the owner losing track.
  void replace(const void *old, void *fresh) {
    for (Held &h : held)
      if (h.p == old) h.p = fresh;
  }
};
