// qh_scratch.h -- a context's scratch buffers: a pointer, a capacity in bytes,
// grow-only reservation and release; and how a buffer is cut into typed
// pieces (Layout) and a host call staged through one (Staged).  The allocator
// and the copy are template parameters, so tests/c/scratch_lifecycle.cc drives
// this code over malloc and memcpy under a sanitizer; qh_api.inc gives it HIP's.
#ifndef QH_SCRATCH_H
#define QH_SCRATCH_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

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

// The round-up of every piece of a buffer: 256 bytes.
constexpr uint64_t align_up(uint64_t bytes) { return (bytes + 255) & ~(uint64_t)255; }

// A buffer cut into typed pieces, each 256-byte aligned from the base.  A
// caller writes its takes once, as a function of a Layout &, and runs it over
// no base for `total` (what to reserve; every pointer null), then over the
// buffer: the same code, so the two cannot disagree.  A piece of no elements
// takes no room; a pad (a kernel's over-read) is a take<uint8_t> of its own.
struct Layout {
  uint8_t *base = nullptr;
  uint64_t total = 0;
  template <class T>
  T *take(uint64_t count) {
    T *const p = base ? reinterpret_cast<T *>(base + total) : nullptr;
    total += align_up(count * sizeof(T));
    return p;
  }
};

// The most pieces with a host side that a call stages
// (qh_plan_fields_dyn_indexed_batch; the two calls of qh_plan_dyn.inc that
// stage a table state and its index assert theirs).
constexpr int kStagePieces = 16;

// A host-memory call's pieces in one device buffer.  Each take is a Layout's
// over no base, kept as a typed offset: once the buffer of `sized.total` bytes
// is reserved and `base` set, s(ref) is the piece.  A piece may have a host
// source (copied in), a host destination (copied back), both or neither; a
// null host pointer or no bytes is no copy.  The copy is the caller's: int
// cp(void *to, const void *from, uint64_t bytes), 0 or an error, which ends it.
struct Staged {
  template <class T>
  struct Ref {
    uint64_t off = 0;
  };
  struct Piece {
    const void *src;
    void *back;
    uint64_t off, bytes;
  };
  Layout sized;
  uint8_t *base = nullptr;
  Piece piece[kStagePieces];
  int npieces = 0;
  template <class T>
  Ref<T> take(uint64_t count, const T *src = nullptr, T *back = nullptr) {
    const Ref<T> r{sized.total};
    sized.take<T>(count);
    if (src || back) {
      if (npieces == kStagePieces) abort();  // (a call with more pieces: raise kStagePieces)
      piece[npieces++] = Piece{src, back, r.off, count * sizeof(T)};
    }
    return r;
  }
  template <class T>
  Ref<T> in(const T *src, uint64_t count) { return take<T>(count, src); }
  template <class T>
  Ref<T> out(T *back, uint64_t count) { return take<T>(count, nullptr, back); }
  template <class T>
  T *operator()(Ref<T> r) const { return reinterpret_cast<T *>(base + r.off); }
  template <class Copy>
  int copy(bool back, Copy &&cp) const {
    for (const Piece *p = piece; p < piece + npieces; ++p) {
      if (!p->bytes || !(back ? p->back != nullptr : p->src != nullptr)) continue;
      const int rv = back ? cp(p->back, (const void *)(base + p->off), p->bytes)
                          : cp((void *)(base + p->off), p->src, p->bytes);
      if (rv) return rv;
    }
    return 0;
  }
};

}  // namespace qhs

#endif
