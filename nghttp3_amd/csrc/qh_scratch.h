// qh_scratch.h -- a context's scratch buffers: a pointer, a capacity in bytes,
// grow-only reservation and release.  The allocator is a template parameter,
// so tests/c/scratch_lifecycle.cc drives this code over malloc under a
// sanitizer; qh_api.inc gives it HIP's.
#ifndef QH_SCRATCH_H
#define QH_SCRATCH_H

#include <stddef.h>
#include <stdint.h>

namespace qhs {

enum Kind : uint8_t { kDevice = 0, kPinned = 1 };  // device memory, pinned host memory

struct Scratch {
  void *p = nullptr;
  size_t cap = 0;  // bytes
  Kind kind = kDevice;
};

// The smallest min * 2^k that holds n (n itself where that overflows).
constexpr size_t pow2_at_least(size_t n, size_t min) {
  size_t c = min;
  while (c < n && c <= SIZE_MAX / 2) c *= 2;
  return c < n ? n : c;
}

// A buffer's capacity rule: pow2_at_least(request, min), or with min 0 the
// request itself.
struct Policy {
  size_t min;
};
constexpr Policy kExact{0};
constexpr Policy kPow2MiB{(size_t)1 << 20};

enum { kFailed = -1, kKept = 0, kGrown = 1 };

// At least `bytes` in s, its contents not kept.  kGrown: s.p is a new
// allocation (what its owner keeps in it has to be set up again); kKept: s
// is as it was.  A buffer is never shrunk, and a.quiesce() -- the work that
// may still use the buffer has ended -- precedes the free of a live one.
// kFailed leaves s as it was when quiesce() failed, else empty (null, 0).
// A: bool alloc(void **p, size_t bytes, Kind); void free(void *p, Kind);
//    bool quiesce().
template <class A>
int reserve(A &a, Scratch &s, size_t bytes, Policy pol) {
  if (s.cap >= bytes) return kKept;
  if (s.p) {
    if (!a.quiesce()) return kFailed;
    a.free(s.p, s.kind);
  }
  s.p = nullptr;
  s.cap = 0;
  const size_t cap = pol.min ? pow2_at_least(bytes, pol.min) : bytes;
  if (!a.alloc(&s.p, cap, s.kind)) {
    s.p = nullptr;
    return kFailed;
  }
  s.cap = cap;
  return kGrown;
}

template <class A>
void release(A &a, Scratch &s) {
  if (s.p) a.free(s.p, s.kind);
  s.p = nullptr;
  s.cap = 0;
}

}  // namespace qhs

#endif
